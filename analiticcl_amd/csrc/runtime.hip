// runtime.hip -- what the engine keeps per device besides the lexicon and the batches, no kernel: the device memory pool and the
// pinned result cache (one policy: block_cache.hpp), the encoder / thread / replica / run streams, the shells of freed batches
// (events + pinned read-back block), the lexicon count that empties a device's pool with its last model, and the kernel timer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "block_cache.hpp"

namespace anx {

#include "kernels_common.hpp"  // (BatchShell)

int device_count(std::string& err) {
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { err = std::string("hipGetDeviceCount: ") + hipGetErrorString(e); return 0; }
  return n;
}

// Device memory pool.  A batch needs several GB of scratch (pair list, per-slot arrays, survivor rows); hipMalloc /
// hipFree of that size cost 100-300 ms per call, far more than the 6 ms the kernels take for a million queries, and
// search mode issues one batch per n-gram order.  Freed blocks are kept per device and handed out again (best fit,
// at most 2x the request + 1 MB); lexicon_released() of the last lexicon on a device returns them to the driver.
// A full cache lets its oldest blocks go, and not to hipFree at once -- it waits for the whole device, and pool_free runs on the
// hot path: a pipeline of fresh batches whose (un-hinted, 7 GB) first runs had filled the cache freed a block per batch and stalled
// its fetch thread behind the runs in flight: 273 instead of 355 M queries/s in bench.py's end-to-end section (round 6).  The next
// cache miss (it pays a hipMalloc anyway) or trim hands them to the driver.
namespace {
// bytes of freed blocks kept per device (MI355X: 288 GB HBM; a 1 M-query batch holds 3-6 GB of scratch).  ANX_POOL_CACHE_MB
// overrides the default; anx_device_pool_trim() hands the cache back to the driver at any time.
// (32 GB until round 6: six un-hinted first runs of a million queries, 7 GB each, outgrew it)
size_t env_mb(const char* name, size_t dflt) { const char* e = getenv(name); const long long v = e ? atoll(e) : -1; return v >= 0 ? (size_t)v << 20 : dflt; }
size_t pool_cache_limit() { static const size_t lim = env_mb("ANX_POOL_CACHE_MB", (size_t)96 << 30); return lim; }
struct DevPool {
  std::mutex mu;
  BlockCache cache{{pool_cache_limit(), (size_t)1 << 20, pool_cache_limit() / 2}};  // every block of this pool, handed out or cached
  int lexicons = 0;
  std::vector<hipStream_t> idle_streams;           // non-blocking streams of the device-side encoder, handed out per call
  hipStream_t run_streams[2] = {nullptr, nullptr}; // the library's own streams for asynchronous runs (batch_run_async)
  unsigned run_counter = 0;
  std::vector<BatchShell> shells;                  // events + pinned read-back blocks of freed batches (batch_free), handed to the next batch
};
DevPool& pool_of(int device) {
  static DevPool pools[64];
  return pools[device >= 0 && device < 64 ? device : 0];
}
DevPool& current_pool() { int dev = 0; (void)hipGetDevice(&dev); return pool_of(dev); }
void free_all(const std::vector<void*>& drop) { for (void* d : drop) (void)hipFree(d); }
}  // namespace

hipError_t pool_malloc(void** p, size_t bytes) {
  DevPool& pl = current_pool();
  bytes = (bytes + 255) & ~(size_t)255;
  std::vector<void*> drop;
  {
    std::lock_guard<std::mutex> g(pl.mu);
    if ((*p = pl.cache.take(bytes))) return hipSuccess;
    pl.cache.reap(drop);
  }
  free_all(drop);
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {  // out of memory: give the cache back and retry once
    drop.clear();
    { std::lock_guard<std::mutex> g(pl.mu); pl.cache.drop_cached(drop); }
    free_all(drop);
    (void)hipGetLastError();
    e = hipMalloc(p, bytes);
    if (e != hipSuccess) return e;
  }
  std::lock_guard<std::mutex> g(pl.mu);
  pl.cache.add(*p, bytes);
  return hipSuccess;
}
void pool_free(void* p) {
  if (!p) return;
  DevPool& pl = current_pool();
  std::vector<void*> drop;
  BlockCache::Given given;
  { std::lock_guard<std::mutex> g(pl.mu); given = pl.cache.give(p, drop); }
  free_all(drop);
  if (given != BlockCache::Given::Kept) (void)hipFree(p);
}
static void shells_destroy(int device);
static void pool_trim(int device) {  // (the current device is `device`)
  DevPool& pl = pool_of(device);
  small_ctxs_destroy(device);  // (first: their blocks go back to the pool that is emptied below)
  std::vector<void*> drop;
  { std::lock_guard<std::mutex> g(pl.mu); pl.cache.drain(drop); }
  free_all(drop);
  shells_destroy(device);
}
void lexicon_registered(int device) { DevPool& pl = pool_of(device); std::lock_guard<std::mutex> g(pl.mu); ++pl.lexicons; }
void lexicon_released(int device) {
  bool last;
  { DevPool& pl = pool_of(device); std::lock_guard<std::mutex> g(pl.mu); last = --pl.lexicons <= 0; }
  if (last) pool_trim(device);  // the last model of this device: hand the cached blocks back to the driver
}

// Pinned host buffers for the downloaded results.  A fresh malloc'd buffer of 141 MB (1 M queries of config 2) is pageable and
// untouched: the D2H copy is staged and page-faults its way through it (~20 ms); a pinned buffer takes the rows at PCIe speed.
// Pinning costs more than the copy, so freed buffers are kept (anx_results_free returns them here) up to ANX_PINNED_CACHE_MB
// (default 2048: a pipeline of 6-8 batches of a million queries in flight, 75-140 MB of rows each, outgrew 1024 and pinned afresh
// for every batch at half the rate); anx_device_pool_trim releases them.  Without a HIP device the buffers are plain malloc blocks,
// known to the cache and never kept.  The oldest leave a full cache first (until the end of round 5 the block that came back was
// dropped instead: a process that had filled the cache with the buffers of one workload -- bench.py after its 1 M-entry lexicon --
// then pinned and unpinned the buffers of the next one on every call: search mode 225-240 instead of 250-280 MB/s).
namespace {
size_t host_cache_limit() { static const size_t lim = env_mb("ANX_PINNED_CACHE_MB", (size_t)2 << 30); return lim; }
struct HostCache {
  std::mutex mu;
  BlockCache cache{{host_cache_limit(), 0, host_cache_limit()}};  // cacheable = pinned
};
HostCache& host_cache() { static HostCache c; return c; }
void host_free_all(const std::vector<void*>& drop) { for (void* q : drop) (void)hipHostFree(q); }
}  // namespace
static std::atomic<uint64_t> g_host_hits{0}, g_host_misses{0}, g_host_miss_bytes{0};
void host_result_cache_stats(uint64_t* hits, uint64_t* misses, uint64_t* miss_bytes) { *hits = g_host_hits.load(); *misses = g_host_misses.load(); *miss_bytes = g_host_miss_bytes.load(); }
void* host_result_alloc(size_t bytes) {
  HostCache& hc = host_cache();
  bytes = (std::max<size_t>(bytes, 64) + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);  // whole MB: a few distinct sizes
  std::vector<void*> drop;
  {
    std::lock_guard<std::mutex> g(hc.mu);
    if (void* p = hc.cache.take(bytes)) { ++g_host_hits; return p; }
    hc.cache.reap(drop);  // a miss pins a fresh block anyway: the evicted ones are released here
  }
  ++g_host_misses;
  g_host_miss_bytes += bytes;
  host_free_all(drop);
  void* p = nullptr;
  bool pinned = hipHostMalloc(&p, bytes, hipHostMallocPortable) == hipSuccess && p;  // portable: the replicas of a multi-device model download into one buffer
  if (!pinned) {
    (void)hipGetLastError();
    p = malloc(bytes);
    if (!p) return nullptr;
  }
  std::lock_guard<std::mutex> g(hc.mu);
  hc.cache.add(p, bytes, pinned);
  return p;
}
bool host_result_is_pinned(void* p) {
  HostCache& hc = host_cache();
  std::lock_guard<std::mutex> g(hc.mu);
  bool pinned = false;
  return hc.cache.known(p, &pinned) && pinned;
}
void host_result_free(void* p) {
  if (!p) return;
  HostCache& hc = host_cache();
  std::vector<void*> drop;
  BlockCache::Given given;
  { std::lock_guard<std::mutex> g(hc.mu); given = hc.cache.give(p, drop); }
  host_free_all(drop);
  if (given == BlockCache::Given::Kept) return;
  if (given == BlockCache::Given::TooLarge) (void)hipHostFree(p);
  else free(p);  // a malloc block (also: rows assembled by anx_find_variants_batch from several device batches)
}
void device_pool_trim(int device) {
  int cur = -1;
  const bool have_cur = hipGetDevice(&cur) == hipSuccess;
  if (hipSetDevice(device) == hipSuccess) pool_trim(device);
  else (void)hipGetLastError();
  if (have_cur && cur != device) (void)hipSetDevice(cur);  // the caller's current device is not ours to change
  HostCache& hc = host_cache();
  std::vector<void*> drop;
  { std::lock_guard<std::mutex> g(hc.mu); hc.cache.drain(drop); }
  host_free_all(drop);
}

// ---- streams --------------------------------------------------------------------------------------------------------------------------
// A private non-blocking stream for one encoder call (encode.hip): on the legacy NULL stream every encode would serialise with
// the in-flight batches of other host threads that run on blocking streams.  Streams are kept per device and reused.
// A thread may bring its own encoder stream (anx_pipeline's encode thread: created together with the pipeline's run streams, so that
// the runtime's least-used-hardware-queue rule puts the three on different queues -- see anx_pipeline_new).
static thread_local hipStream_t t_encoder_stream = nullptr;
// A non-blocking stream on the current device.  high = the device's highest stream priority: the encoder of batch i + 1 (and search
// mode's lattice-build kernels) are chains of ~45 short dependent launches that run beside the scan / scoring kernels of batch i --
// tens of thousands of waves queued on streams of normal priority; at equal priority every launch of the chain waits its turn behind
// them (round 5: the encoder "under" a run took the run's length), at high priority the dispatcher serves its few workgroups first.
// ANX_ENC_PRIORITY=0: normal priority (A/B).
void* make_stream(bool high) {
  hipStream_t s = nullptr;
  int least = 0, greatest = 0;
  if (high && switches().enc_priority && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest < least) {
    if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest) == hipSuccess) return s;
    (void)hipGetLastError();
  }
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return s;
}
void encoder_stream_set_override(void* s) { t_encoder_stream = reinterpret_cast<hipStream_t>(s); }
hipStream_t encoder_stream_acquire(int device) {
  if (t_encoder_stream) return t_encoder_stream;
  DevPool& pl = pool_of(device);
  {
    std::lock_guard<std::mutex> g(pl.mu);
    if (!pl.idle_streams.empty()) { hipStream_t s = pl.idle_streams.back(); pl.idle_streams.pop_back(); return s; }
  }
  return static_cast<hipStream_t>(make_stream(true));  // nullptr = the NULL stream: still correct
}
void encoder_stream_release(int device, hipStream_t s) {
  if (!s || s == t_encoder_stream) return;
  DevPool& pl = pool_of(device);
  std::lock_guard<std::mutex> g(pl.mu);
  pl.idle_streams.push_back(s);
}
// One stream for everything a host thread sends to the device during a stretch of work (a part of a search-mode call: its batches'
// encodes and runs, its lattices): taken from the encoder's pool, installed as the thread's encoder stream, handed back at the end.
void* thread_stream_begin(int device) {
  if (t_encoder_stream) return nullptr;  // the thread brought its own
  DeviceGuard guard;  // (the pool may have to create the stream: on the replica's device, not on the thread's current one)
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  hipStream_t s = encoder_stream_acquire(device);
  t_encoder_stream = s;
  return s;
}
void thread_stream_end(int device, void* s) {
  if (!s) return;
  t_encoder_stream = nullptr;
  encoder_stream_release(device, reinterpret_cast<hipStream_t>(s));
}
// streams of the replicas of a multi-device model (capi.cpp owns them; HIP stays behind this file)
void* stream_create(int device, std::string& err, bool high_priority) {
  DeviceGuard guard;
  void* s = nullptr;
  if (hipSetDevice(device) != hipSuccess || !(s = make_stream(high_priority))) {
    err = std::string("hipStreamCreate: ") + hipGetErrorString(hipGetLastError());
    return nullptr;
  }
  return s;
}
void stream_destroy(int device, void* s) {
  DeviceGuard guard;
  if (!s) return;
  (void)hipSetDevice(device);
  (void)hipStreamDestroy(reinterpret_cast<hipStream_t>(s));
}
// the library's own two streams for asynchronous runs (batch_run_async), alternately; created on first use on the current device = `device`
hipStream_t run_stream_next(int device) {
  DevPool& pl = pool_of(device);
  std::lock_guard<std::mutex> g(pl.mu);
  hipStream_t& slot = pl.run_streams[pl.run_counter++ & 1u];
  if (!slot && hipStreamCreateWithFlags(&slot, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); slot = nullptr; }
  return slot;
}

// ---- shells: events + pinned read-back block of a batch (BatchShell, kernels_common.hpp) ---------------------------------------------
static void shell_destroy(BatchShell& sh) {
  for (auto& e : sh.ev) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : {sh.ev_fs0, sh.ev_fs1, sh.ev_scan0, sh.ev_done, sh.ev_in}) if (e) (void)hipEventDestroy(e);
  if (sh.h_read) (void)hipHostFree(sh.h_read);
  sh = BatchShell{};
}
static int shell_create(BatchShell& sh, size_t pinned_bytes, std::string& err) {
  for (auto& e : sh.ev) HIP_TRY(hipEventCreate(&e));
  HIP_TRY(hipEventCreate(&sh.ev_fs0));
  HIP_TRY(hipEventCreate(&sh.ev_fs1));
  HIP_TRY(hipEventCreate(&sh.ev_scan0));
  HIP_TRY(hipEventCreate(&sh.ev_done));
  HIP_TRY(hipEventCreateWithFlags(&sh.ev_in, hipEventDisableTiming));
  // pinned: the counters the run reads back, and behind them the staging copy of FsCold (a pageable source would make the host
  // wait, in stream order behind the scan just enqueued, until the copy has been staged)
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&sh.h_read), pinned_bytes, hipHostMallocDefault));
  return ANX_OK;
}
// from the device's shells of freed batches, created when there is none (a creation that fails half way destroys what it made)
int shell_acquire(int device, BatchShell& sh, size_t pinned_bytes, std::string& err) {
  DevPool& pl = pool_of(device);
  {
    std::lock_guard<std::mutex> g(pl.mu);
    if (!pl.shells.empty()) { sh = pl.shells.back(); pl.shells.pop_back(); return ANX_OK; }
  }
  const int rc = shell_create(sh, pinned_bytes, err);
  if (rc) shell_destroy(sh);
  return rc;
}
void shell_release(int device, BatchShell& sh) {
  if (!sh.ev_done) return;  // never acquired (an encode that failed early)
  DevPool& pl = pool_of(device);
  std::lock_guard<std::mutex> g(pl.mu);
  pl.shells.push_back(sh);
  sh = BatchShell{};
}
static void shells_destroy(int device) {  // (the current device is `device`)
  DevPool& pl = pool_of(device);
  std::vector<BatchShell> drop;
  { std::lock_guard<std::mutex> g(pl.mu); drop.swap(pl.shells); }
  for (BatchShell& sh : drop) shell_destroy(sh);
}

// ---- kernel timer (engine_internal.h) ---------------------------------------------------------------------------------
namespace {
struct KTimerRec { std::string name; hipEvent_t e0 = nullptr, e1 = nullptr; int device = 0; bool closed = false; };
struct KTimer {
  std::mutex mu;
  std::atomic<bool> on{false};
  std::vector<KTimerRec> pending;
  uint32_t generation = 0;  // of `pending`: part of the handles ktimer_begin hands out
  std::map<std::string, std::pair<double, uint64_t>> acc;
};
KTimer& ktimer() { static KTimer* t = new KTimer; return *t; }
void ktimer_resolve_locked(KTimer& t) {
  for (KTimerRec& r : t.pending) {
    if (r.closed && hipEventSynchronize(r.e1) == hipSuccess) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { auto& a = t.acc[r.name]; a.first += ms; a.second += 1; }
    }
    if (r.e0) (void)hipEventDestroy(r.e0);
    if (r.e1) (void)hipEventDestroy(r.e1);
  }
  t.pending.clear();
  ++t.generation;  // handles of the records just dropped (also unclosed ones of a launch in progress on another thread) are void now
}
}  // namespace
int ktimer_begin(const char* name, hipStream_t st) {
  KTimer& t = ktimer();
  if (!t.on.load(std::memory_order_relaxed)) return -1;
  KTimerRec r;
  r.name = name;
  if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess || hipEventRecord(r.e0, st) != hipSuccess) {
    if (r.e0) (void)hipEventDestroy(r.e0);
    if (r.e1) (void)hipEventDestroy(r.e1);
    return -1;
  }
  std::lock_guard<std::mutex> lk(t.mu);
  if (t.pending.size() >= 0xFFFFu) return -1;
  t.pending.push_back(r);
  return (int)(((t.generation & 0x7FFFu) << 16) | (uint32_t)(t.pending.size() - 1));  // generation + index: stable across kernel_timer_read
}
void ktimer_end(int handle, hipStream_t st) {
  if (handle < 0) return;
  KTimer& t = ktimer();
  std::lock_guard<std::mutex> lk(t.mu);
  const uint32_t idx = (uint32_t)handle & 0xFFFFu;
  if ((((uint32_t)handle >> 16) & 0x7FFFu) != (t.generation & 0x7FFFu) || idx >= t.pending.size()) return;  // the totals were read in between: the record is gone
  KTimerRec& r = t.pending[idx];
  if (hipEventRecord(r.e1, st) == hipSuccess) r.closed = true;
}
void kernel_timer_enable(bool on) {
  KTimer& t = ktimer();
  std::lock_guard<std::mutex> lk(t.mu);
  ktimer_resolve_locked(t);
  t.acc.clear();
  t.on.store(on);
}
bool kernel_timer_read(const char* name, double* total_ms, uint64_t* launches) {
  KTimer& t = ktimer();
  std::lock_guard<std::mutex> lk(t.mu);
  ktimer_resolve_locked(t);
  auto it = t.acc.find(name ? name : "");
  if (it == t.acc.end()) { if (total_ms) *total_ms = 0.0; if (launches) *launches = 0; return false; }
  if (total_ms) *total_ms = it->second.first;
  if (launches) *launches = it->second.second;
  return true;
}

}  // namespace anx
