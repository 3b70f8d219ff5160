// learn.hip -- learn mode's fold ON THE DEVICE (gfx950 / CDNA4).
//
// learn_variants (src/lib.rs:1029-1139) queries every input, flattens the ranked rows in input order and folds them
// into the model: each input string is resolved to a vocabulary id (new strings are appended, ids in order of first mention), the
// frequency of a known string grows by 1 per run of consecutive rows of that string, and every row whose result is not the input
// itself links (result, input) -- ReferenceFor deduplicated by first mention, VariantOf appended every time.  The reference does
// that with one string-hash lookup per row on one host thread; here the same fold is a handful of data-parallel passes over the
// rows where the batch left them in HBM, and the host only appends what comes back (HostModel::learn_apply):
//   k_lf_sections : the compact export sections of the batch's shards (anx_batch_gather_compact layout, all on this device) ->
//                   per input: row count, section, first record
//   k_lf_lookup   : one lane per input with rows: FNV-1a of its bytes, probe of the vocabulary table (hash -> id, every candidate
//                   checked byte by byte against the vocabulary's UTF-8 pool)
//   sort (hash, input) of the strings the table does not know; k_lf_head + max-scan = run starts; k_lf_rep: the first input of a
//                   run with the same BYTES (a hash collision never merges two strings) -> representative; exclusive scan of the
//                   representatives in input order = new ids in order of first mention (k_lf_assign)
//   k_lf_cid / k_lf_runs : inputs with rows in input order; a run starts where the id differs from the previous such input ->
//                   per-id frequency delta (atomics)
//   k_lf_rows     : one lane per input: its rows -> link key (ref << 32 | var) or "no link" (the result is the input itself)
//   stable sort of the link keys (value = flat position) -> k_lf_first marks the first mention of each (ref, var)
//   exclusive scans + k_lf_emit / k_lf_deltas / k_lf_new : the compact arrays the host applies
// The vocabulary table (LearnVocab) is built here from the host's texts on first use and rebuilt when the vocabulary size (or the test
// switch ANX_LEARN_HASH_BITS) changes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "engine_internal.h"

namespace anx {

namespace {
constexpr uint32_t LF_NONE = 0xFFFFFFFFu;     // input without rows: no id
constexpr uint32_t LF_PENDING = 0xFFFFFFFEu;  // input with rows whose string is not in the vocabulary (yet)
constexpr unsigned long long LF_NOKEY = ~0ull;  // sorts behind every real key (hashes have the top bit clear)
constexpr int LF_BLOCK = 256;

// (LF_EMPTY, lf_hash, lf_eq and LearnVocab: engine_internal.h -- eval.hip probes the same table)
inline unsigned grid_of(size_t n) { return (unsigned)std::max<size_t>(1, (n + LF_BLOCK - 1) / LF_BLOCK); }

// vocabulary table: open addressing, linear probing, capacity a power of two >= 2 V (every probe ends at a free slot)
__global__ void k_lv_build(uint32_t V, const uint8_t* __restrict__ pool, const uint32_t* __restrict__ voff, unsigned long long* __restrict__ vh,
                           uint32_t* __restrict__ slots, uint32_t mask, unsigned long long hmask) {
  const uint32_t id = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (id >= V) return;
  const unsigned long long h = lf_hash(pool + voff[id], voff[id + 1] - voff[id], hmask);
  vh[id] = h;
  uint32_t s = (uint32_t)h & mask;
  while (atomicCAS(&slots[s], LF_EMPTY, id) != LF_EMPTY) s = (s + 1) & mask;
}

struct Section { const anx_topk_record* rec; const uint32_t* off; const uint32_t* idx; uint32_t n, lo; };

__global__ void k_lf_sections(Section sec, uint32_t sid, uint32_t n, uint32_t* __restrict__ cnt, uint32_t* __restrict__ src_sec,
                              uint32_t* __restrict__ src_row) {
  const uint32_t j = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (j >= sec.n) return;
  const uint32_t i = sec.idx ? sec.idx[j] : sec.lo + j;
  if (i >= n) return;
  cnt[i] = sec.off[j + 1] - sec.off[j];
  src_sec[i] = sid;
  src_row[i] = sec.off[j];
}

__global__ void k_lf_lookup(uint32_t n, const uint8_t* __restrict__ blob, const uint32_t* __restrict__ soff, const uint32_t* __restrict__ cnt,
                            const uint8_t* __restrict__ pool, const uint32_t* __restrict__ voff, const unsigned long long* __restrict__ vh,
                            const uint32_t* __restrict__ slots, uint32_t mask, unsigned long long hmask, uint32_t* __restrict__ id,
                            unsigned long long* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t i = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (i >= n) return;
  val[i] = i;
  if (cnt[i] == 0) { id[i] = LF_NONE; key[i] = LF_NOKEY; return; }
  const uint8_t* a = blob + soff[i];
  const uint32_t la = soff[i + 1] - soff[i] - 1;  // (each input is followed by a NUL byte)
  const unsigned long long h = lf_hash(a, la, hmask);
  for (uint32_t s = (uint32_t)h & mask;; s = (s + 1) & mask) {
    const uint32_t v = slots[s];
    if (v == LF_EMPTY) break;
    if (vh[v] == h && lf_eq(a, la, pool + voff[v], voff[v + 1] - voff[v])) { id[i] = v; key[i] = LF_NOKEY; return; }
  }
  id[i] = LF_PENDING;
  key[i] = h;
}

__global__ void k_lf_head(uint32_t n, const unsigned long long* __restrict__ skey, uint32_t* __restrict__ head) {
  const uint32_t p = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (p >= n) return;
  head[p] = (p > 0 && skey[p] == skey[p - 1]) ? 0u : p;
}

// sorted position p of an unknown string: the first input of its hash run with the same bytes (the run is in input order: the
// sort is stable and the values started as the identity) is its representative
__global__ void k_lf_rep(uint32_t n, const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ sval, const uint32_t* __restrict__ rstart,
                         const uint8_t* __restrict__ blob, const uint32_t* __restrict__ soff, uint32_t* __restrict__ rep, uint32_t* __restrict__ isnew) {
  const uint32_t p = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (p >= n || skey[p] == LF_NOKEY) return;
  const uint32_t i = sval[p];
  const uint8_t* a = blob + soff[i];
  const uint32_t la = soff[i + 1] - soff[i] - 1;
  uint32_t r = i;
  for (uint32_t q = rstart[p]; q < p; ++q) {
    const uint32_t j = sval[q];
    if (lf_eq(a, la, blob + soff[j], soff[j + 1] - soff[j] - 1)) { r = j; break; }
  }
  rep[i] = r;
  isnew[i] = r == i ? 1u : 0u;
}

__global__ void k_lf_assign(uint32_t n, uint32_t V, const uint32_t* __restrict__ rep, const uint32_t* __restrict__ nidx, uint32_t* __restrict__ id,
                            const uint32_t* __restrict__ cnt, uint32_t* __restrict__ has) {
  const uint32_t i = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (id[i] == LF_PENDING) id[i] = V + nidx[rep[i]];
  has[i] = cnt[i] ? 1u : 0u;
}

__global__ void k_lf_cid(uint32_t n, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ id, const uint32_t* __restrict__ hpos,
                         uint32_t* __restrict__ cid) {
  const uint32_t i = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (i >= n || !cnt[i]) return;
  cid[hpos[i]] = id[i];
}

// a run of one string starts where the previous input WITH ROWS had another id: the reference's `prev != Some(inputstr)` per row
__global__ void k_lf_runs(uint32_t n, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ id, const uint32_t* __restrict__ hpos,
                          const uint32_t* __restrict__ cid, uint32_t* __restrict__ delta) {
  const uint32_t i = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (i >= n || !cnt[i]) return;
  const uint32_t h = hpos[i];
  if (h == 0 || cid[h - 1] != id[i]) atomicAdd(&delta[id[i]], 1u);
}

__global__ void k_lf_rows(uint32_t n, uint32_t R, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ roff, const uint32_t* __restrict__ src_sec,
                          const uint32_t* __restrict__ src_row, const Section* __restrict__ secs, const uint32_t* __restrict__ id,
                          unsigned long long* __restrict__ lkey, uint32_t* __restrict__ lval, uint32_t* __restrict__ cand,
                          uint32_t* __restrict__ rref, uint32_t* __restrict__ rvar, double* __restrict__ rscore) {
  const uint32_t i = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = cnt[i];
  if (!c) return;
  const anx_topk_record* rec = secs[src_sec[i]].rec + src_row[i];
  const uint32_t var = id[i];
  for (uint32_t k = 0; k < c; ++k) {
    const uint32_t r = roff[i] + k;
    if (r >= R) return;
    const anx_topk_record t = rec[k];
    const bool link = t.vocab_id != var;
    lkey[r] = link ? ((unsigned long long)t.vocab_id << 32 | var) : LF_NOKEY;
    lval[r] = r;
    cand[r] = link ? 1u : 0u;
    rref[r] = t.vocab_id;
    rvar[r] = var;
    rscore[r] = t.dist_score;
  }
}

__global__ void k_lf_first(uint32_t R, const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ sval, uint32_t* __restrict__ keep) {
  const uint32_t p = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (p >= R || skey[p] == LF_NOKEY) return;
  if (p == 0 || skey[p - 1] != skey[p]) keep[sval[p]] = 1u;
}

__global__ void k_lf_emit(uint32_t R, const uint32_t* __restrict__ cand, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ vpos,
                          const uint32_t* __restrict__ kpos, const uint32_t* __restrict__ rref, const uint32_t* __restrict__ rvar,
                          const double* __restrict__ rscore, LearnLink* __restrict__ var_of, LearnLink* __restrict__ ref_for) {
  const uint32_t r = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (r >= R || !cand[r]) return;
  const LearnLink l{rref[r], rvar[r], rscore[r], r, 0u};
  var_of[vpos[r]] = l;
  if (keep[r]) ref_for[kpos[r]] = l;
}

__global__ void k_lf_dflag(uint32_t V, const uint32_t* __restrict__ delta, uint32_t* __restrict__ flag) {
  const uint32_t k = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (k < V) flag[k] = delta[k] ? 1u : 0u;
}
__global__ void k_lf_deltas(uint32_t V, const uint32_t* __restrict__ delta, const uint32_t* __restrict__ dpos, uint32_t* __restrict__ fid,
                            uint32_t* __restrict__ fdelta) {
  const uint32_t k = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (k >= V || !delta[k]) return;
  fid[dpos[k]] = k;
  fdelta[dpos[k]] = delta[k];
}
__global__ void k_lf_new(uint32_t n, uint32_t V, const uint32_t* __restrict__ isnew, const uint32_t* __restrict__ nidx, const uint32_t* __restrict__ delta,
                         uint32_t* __restrict__ new_src, uint32_t* __restrict__ new_freq) {
  const uint32_t i = blockIdx.x * LF_BLOCK + threadIdx.x;
  if (i >= n || !isnew[i]) return;
  const uint32_t k = nidx[i];
  new_src[k] = i;
  new_freq[k] = delta[V + k];
}

// device blocks of one call, handed back to the pool when it ends (after its stream is idle)
struct Blocks {
  hipStream_t st = nullptr;
  int device = 0;
  std::vector<void*> v;
  template <typename T>
  int get(T** p, size_t count, std::string& err) {
    HIP_TRY(pool_malloc(reinterpret_cast<void**>(p), std::max<size_t>(count * sizeof(T), 16)));
    v.push_back(*p);
    return ANX_OK;
  }
  ~Blocks() {
    if (st) { (void)hipStreamSynchronize(st); encoder_stream_release(device, st); }
    for (void* p : v) pool_free(p);
  }
};
int scan_excl(const uint32_t* in, uint32_t* out, size_t n, Blocks& b, hipStream_t st, std::string& err) {
  size_t bytes = 0;
  HIP_TRY(rocprim::exclusive_scan(nullptr, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), st));
  char* tmp = nullptr;
  if (int rc = b.get(&tmp, bytes + 16, err)) return rc;
  HIP_TRY(rocprim::exclusive_scan(tmp, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), st));
  return ANX_OK;
}
int scan_max(uint32_t* a, size_t n, Blocks& b, hipStream_t st, std::string& err) {
  size_t bytes = 0;
  HIP_TRY(rocprim::inclusive_scan(nullptr, bytes, a, a, n, rocprim::maximum<uint32_t>(), st));
  char* tmp = nullptr;
  if (int rc = b.get(&tmp, bytes + 16, err)) return rc;
  HIP_TRY(rocprim::inclusive_scan(tmp, bytes, a, a, n, rocprim::maximum<uint32_t>(), st));
  return ANX_OK;
}
int sort64(const unsigned long long* kin, unsigned long long* kout, const uint32_t* vin, uint32_t* vout, size_t n, Blocks& b, hipStream_t st,
           std::string& err) {
  size_t bytes = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, 0, 64, st));
  char* tmp = nullptr;
  if (int rc = b.get(&tmp, bytes + 16, err)) return rc;
  HIP_TRY(rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, n, 0, 64, st));
  return ANX_OK;
}
}  // namespace

void* learn_device_alloc(int device, size_t bytes) {
  void* p = nullptr;
  if (hipSetDevice(device) != hipSuccess || hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}
void learn_device_free(int device, void* p) {
  if (!p) return;
  (void)hipSetDevice(device);
  (void)hipFree(p);
}
bool learn_device_upload(int device, void* dst, const void* src, size_t bytes) {
  if (!bytes) return true;
  if (hipSetDevice(device) != hipSuccess || hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return false; }
  return true;
}

void learn_vocab_free(LearnVocab* t) {
  if (!t) return;
  if (t->device >= 0) (void)hipSetDevice(t->device);
  for (void* p : {(void*)t->pool, (void*)t->voff, (void*)t->vh, (void*)t->slots})
    if (p) (void)hipFree(p);
  delete t;
}

static int learn_vocab_build(const HostModel& m, int device, LearnVocab** cache, hipStream_t st, std::string& err) {
  const size_t V = m.decoder.size();
  const int bits = switches().learn_hash_bits;
  const unsigned long long hmask = bits >= 63 ? 0x7FFFFFFFFFFFFFFFull : (1ull << bits) - 1;
  if (*cache && (*cache)->device == device && (*cache)->V == V && (*cache)->hmask == hmask) return ANX_OK;
  learn_vocab_free(*cache);
  *cache = nullptr;
  if (V >= LF_PENDING) { err = "vocabulary too large for the learn fold"; return ANX_ELIMIT; }
  std::vector<uint32_t> off(V + 1);
  size_t total = 0;
  for (size_t k = 0; k < V; ++k) { off[k] = (uint32_t)total; total += m.decoder[k].text.size(); }
  if (total >= 0xFFFFFFFFull) { err = "vocabulary texts exceed 4 GB"; return ANX_ELIMIT; }
  off[V] = (uint32_t)total;
  std::vector<uint8_t> pool(std::max<size_t>(total, 1));
  for (size_t k = 0; k < V; ++k) memcpy(pool.data() + off[k], m.decoder[k].text.data(), m.decoder[k].text.size());
  size_t cap = 16;
  while (cap < 2 * V) cap <<= 1;
  LearnVocab* t = new LearnVocab();
  t->device = device;
  t->V = V;
  t->mask = (uint32_t)(cap - 1);
  t->hmask = hmask;
  auto body = [&]() -> int {
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->pool), pool.size()));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->voff), (V + 1) * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->vh), std::max<size_t>(V, 1) * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->slots), cap * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(t->pool, pool.data(), pool.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(t->voff, off.data(), (V + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(t->slots, 0xFF, cap * sizeof(uint32_t), st));
    if (V) hipLaunchKernelGGL(k_lv_build, dim3(grid_of(V)), dim3(LF_BLOCK), 0, st, (uint32_t)V, t->pool, t->voff, t->vh, t->slots, t->mask, t->hmask);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));  // (the host copies above are pageable: they must outlive the copies)
    return ANX_OK;
  };
  const int rc = body();
  if (rc) { learn_vocab_free(t); return rc; }
  *cache = t;
  return ANX_OK;
}

int learn_vocab_ensure(const HostModel& m, int device, LearnVocab** cache, hipStream_t st, std::string& err) {
  return learn_vocab_build(m, device, cache, st, err);
}

int learn_fold_device(const HostModel& m, int device, LearnVocab** vocab, const char* blob, const uint32_t* soff, size_t n,
                      const std::vector<LearnSection>& secs, size_t n_rows, LearnFold& out, std::string& err) {
  out = LearnFold();
  if (n == 0) return ANX_OK;
  if (n >= 0x7FFFFFFFull || n_rows >= 0x7FFFFFFFull || soff[n] >= 0xFFFFFFFFull) { err = "learn fold: more than 2^31 inputs / rows"; return ANX_ELIMIT; }
  HIP_TRY(hipSetDevice(device));
  std::vector<Section> hs(secs.size());  // (declared before the blocks: an error path syncs the stream before any host source goes away)
  Blocks b;
  b.device = device;
  b.st = encoder_stream_acquire(device);
  hipStream_t st = b.st;
  if (int rc = learn_vocab_build(m, device, vocab, st, err)) return rc;
  const LearnVocab& t = **vocab;
  const uint32_t V = (uint32_t)t.V, n32 = (uint32_t)n, R = (uint32_t)n_rows;
  const size_t nbytes = soff[n];
  // inputs (bytes + offsets) and the section table
  uint8_t* d_blob = nullptr;
  uint32_t *d_soff = nullptr, *d_cnt = nullptr, *d_sec = nullptr, *d_srow = nullptr, *d_roff = nullptr, *d_id = nullptr, *d_val = nullptr,
           *d_sval = nullptr, *d_head = nullptr, *d_rep = nullptr, *d_isnew = nullptr, *d_nidx = nullptr, *d_has = nullptr, *d_hpos = nullptr,
           *d_cid = nullptr, *d_delta = nullptr;
  unsigned long long *d_key = nullptr, *d_skey = nullptr;
  Section* d_secs = nullptr;
  if (int rc = b.get(&d_blob, nbytes + 1, err)) return rc;
  if (int rc = b.get(&d_soff, n + 1, err)) return rc;
  if (int rc = b.get(&d_secs, secs.size(), err)) return rc;
  for (uint32_t** p : {&d_cnt, &d_sec, &d_srow, &d_roff, &d_id, &d_val, &d_sval, &d_head, &d_rep, &d_isnew, &d_nidx, &d_has, &d_hpos, &d_cid})
    if (int rc = b.get(p, n + 1, err)) return rc;
  if (int rc = b.get(&d_delta, (size_t)V + n, err)) return rc;
  if (int rc = b.get(&d_key, n, err)) return rc;
  if (int rc = b.get(&d_skey, n, err)) return rc;
  std::vector<uint32_t*> d_idx(secs.size(), nullptr);
  for (size_t s = 0; s < secs.size(); ++s) {
    const LearnSection& L = secs[s];
    const size_t off_bytes = ((L.n + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
    hs[s].off = static_cast<const uint32_t*>(L.base);
    hs[s].rec = reinterpret_cast<const anx_topk_record*>(static_cast<const char*>(L.base) + off_bytes);
    hs[s].n = (uint32_t)L.n;
    hs[s].lo = (uint32_t)L.lo;
    hs[s].idx = nullptr;
    if (L.idx) {
      if (int rc = b.get(&d_idx[s], L.n, err)) return rc;
      HIP_TRY(hipMemcpyAsync(d_idx[s], L.idx, L.n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      hs[s].idx = d_idx[s];
    }
  }
  HIP_TRY(hipMemcpyAsync(d_blob, blob, nbytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_soff, soff, (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_secs, hs.data(), hs.size() * sizeof(Section), hipMemcpyHostToDevice, st));
  for (uint32_t* p : {d_cnt, d_isnew, d_has})
    HIP_TRY(hipMemsetAsync(p, 0, (n + 1) * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(d_delta, 0, ((size_t)V + n) * sizeof(uint32_t), st));
  // (a) rows per input, (b) hash + vocabulary lookup
  for (size_t s = 0; s < secs.size(); ++s)
    if (hs[s].n) hipLaunchKernelGGL(k_lf_sections, dim3(grid_of(hs[s].n)), dim3(LF_BLOCK), 0, st, hs[s], (uint32_t)s, n32, d_cnt, d_sec, d_srow);
  if (int rc = scan_excl(d_cnt, d_roff, n + 1, b, st, err)) return rc;
  {  // the row arrays below are sized for the batch's row count: the sections must hold exactly that many
    uint32_t rows = 0;
    HIP_TRY(hipMemcpyAsync(&rows, d_roff + n, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (rows != n_rows) { err = "learn fold: the gathered sections hold " + std::to_string(rows) + " rows, the batch " + std::to_string(n_rows); return ANX_EINVAL; }
  }
  hipLaunchKernelGGL(k_lf_lookup, dim3(grid_of(n)), dim3(LF_BLOCK), 0, st, n32, d_blob, d_soff, d_cnt, t.pool, t.voff, t.vh, t.slots, t.mask,
                     t.hmask, d_id, d_key, d_val);
  // (c) first-occurrence ids of the strings the vocabulary does not hold
  if (int rc = sort64(d_key, d_skey, d_val, d_sval, n, b, st, err)) return rc;
  hipLaunchKernelGGL(k_lf_head, dim3(grid_of(n)), dim3(LF_BLOCK), 0, st, n32, d_skey, d_head);
  if (int rc = scan_max(d_head, n, b, st, err)) return rc;
  hipLaunchKernelGGL(k_lf_rep, dim3(grid_of(n)), dim3(LF_BLOCK), 0, st, n32, d_skey, d_sval, d_head, d_blob, d_soff, d_rep, d_isnew);
  if (int rc = scan_excl(d_isnew, d_nidx, n + 1, b, st, err)) return rc;
  hipLaunchKernelGGL(k_lf_assign, dim3(grid_of(n)), dim3(LF_BLOCK), 0, st, n32, V, d_rep, d_nidx, d_id, d_cnt, d_has);
  // (d) frequency runs
  if (int rc = scan_excl(d_has, d_hpos, n + 1, b, st, err)) return rc;
  hipLaunchKernelGGL(k_lf_cid, dim3(grid_of(n)), dim3(LF_BLOCK), 0, st, n32, d_cnt, d_id, d_hpos, d_cid);
  hipLaunchKernelGGL(k_lf_runs, dim3(grid_of(n)), dim3(LF_BLOCK), 0, st, n32, d_cnt, d_id, d_hpos, d_cid, d_delta);
  // (d) links: candidates, first mention of each (ref, var), compaction in flat order
  unsigned long long *d_lkey = nullptr, *d_slkey = nullptr;
  uint32_t *d_lval = nullptr, *d_slval = nullptr, *d_cand = nullptr, *d_keep = nullptr, *d_vpos = nullptr, *d_kpos = nullptr, *d_rref = nullptr,
           *d_rvar = nullptr, *d_dflag = nullptr, *d_dpos = nullptr, *d_fid = nullptr, *d_fdelta = nullptr, *d_nsrc = nullptr, *d_nfreq = nullptr;
  double* d_rscore = nullptr;
  LearnLink *d_varof = nullptr, *d_reffor = nullptr;
  if (int rc = b.get(&d_lkey, R, err)) return rc;
  if (int rc = b.get(&d_slkey, R, err)) return rc;
  for (uint32_t** p : {&d_lval, &d_slval, &d_cand, &d_keep, &d_vpos, &d_kpos, &d_rref, &d_rvar})
    if (int rc = b.get(p, (size_t)R + 1, err)) return rc;
  for (uint32_t** p : {&d_dflag, &d_dpos, &d_fid, &d_fdelta})
    if (int rc = b.get(p, (size_t)V + 1, err)) return rc;
  if (int rc = b.get(&d_nsrc, n, err)) return rc;
  if (int rc = b.get(&d_nfreq, n, err)) return rc;
  if (int rc = b.get(&d_rscore, R, err)) return rc;
  if (int rc = b.get(&d_varof, R, err)) return rc;
  if (int rc = b.get(&d_reffor, R, err)) return rc;
  for (uint32_t* p : {d_cand, d_keep})
    HIP_TRY(hipMemsetAsync(p, 0, ((size_t)R + 1) * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(d_dflag, 0, ((size_t)V + 1) * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_lf_rows, dim3(grid_of(n)), dim3(LF_BLOCK), 0, st, n32, R, d_cnt, d_roff, d_sec, d_srow, d_secs, d_id, d_lkey, d_lval, d_cand,
                     d_rref, d_rvar, d_rscore);
  if (R) {
    if (int rc = sort64(d_lkey, d_slkey, d_lval, d_slval, R, b, st, err)) return rc;
    hipLaunchKernelGGL(k_lf_first, dim3(grid_of(R)), dim3(LF_BLOCK), 0, st, R, d_slkey, d_slval, d_keep);
  }
  if (int rc = scan_excl(d_cand, d_vpos, (size_t)R + 1, b, st, err)) return rc;
  if (int rc = scan_excl(d_keep, d_kpos, (size_t)R + 1, b, st, err)) return rc;
  if (R) hipLaunchKernelGGL(k_lf_emit, dim3(grid_of(R)), dim3(LF_BLOCK), 0, st, R, d_cand, d_keep, d_vpos, d_kpos, d_rref, d_rvar, d_rscore, d_varof, d_reffor);
  if (V) hipLaunchKernelGGL(k_lf_dflag, dim3(grid_of(V)), dim3(LF_BLOCK), 0, st, V, d_delta, d_dflag);
  if (int rc = scan_excl(d_dflag, d_dpos, (size_t)V + 1, b, st, err)) return rc;
  if (V) hipLaunchKernelGGL(k_lf_deltas, dim3(grid_of(V)), dim3(LF_BLOCK), 0, st, V, d_delta, d_dpos, d_fid, d_fdelta);
  hipLaunchKernelGGL(k_lf_new, dim3(grid_of(n)), dim3(LF_BLOCK), 0, st, n32, V, d_isnew, d_nidx, d_delta, d_nsrc, d_nfreq);
  HIP_TRY(hipGetLastError());
  // sizes, then the compact arrays
  uint32_t tot[5] = {0, 0, 0, 0, 0};  // rows, new entries, VariantOf, ReferenceFor, frequency deltas
  HIP_TRY(hipMemcpyAsync(&tot[0], d_roff + n, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&tot[1], d_nidx + n, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&tot[2], d_vpos + R, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&tot[3], d_kpos + R, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&tot[4], d_dpos + V, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (tot[0] != R || tot[1] > n || tot[2] > R || tot[3] > tot[2] || tot[4] > V) { err = "learn fold: inconsistent totals"; return ANX_EINVAL; }
  out.new_src.resize(tot[1]);
  out.new_freq.resize(tot[1]);
  out.var_of.resize(tot[2]);
  out.ref_for.resize(tot[3]);
  out.freq_id.resize(tot[4]);
  out.freq_delta.resize(tot[4]);
  if (tot[1]) {
    HIP_TRY(hipMemcpyAsync(out.new_src.data(), d_nsrc, tot[1] * 4ull, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out.new_freq.data(), d_nfreq, tot[1] * 4ull, hipMemcpyDeviceToHost, st));
  }
  if (tot[2]) HIP_TRY(hipMemcpyAsync(out.var_of.data(), d_varof, tot[2] * sizeof(LearnLink), hipMemcpyDeviceToHost, st));
  if (tot[3]) HIP_TRY(hipMemcpyAsync(out.ref_for.data(), d_reffor, tot[3] * sizeof(LearnLink), hipMemcpyDeviceToHost, st));
  if (tot[4]) {
    HIP_TRY(hipMemcpyAsync(out.freq_id.data(), d_fid, tot[4] * 4ull, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out.freq_delta.data(), d_fdelta, tot[4] * 4ull, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  return ANX_OK;
}

}  // namespace anx
