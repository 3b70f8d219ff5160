// engine_internal.h -- shared by the HIP translation units of the engine (engine.hip, runtime.hip, results.hip, encode.hip, ...); include after hip_runtime.h
#pragma once
#include <cstdlib>
#include <cstring>
#include "engine.h"
#include "sig_hash.h"

// in a function that returns a code and has a std::string err
#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      err = std::string(#expr) + ": " + hipGetErrorString(_e);                                 \
      return ANX_ENODEVICE;                                                                    \
    }                                                                                          \
  } while (0)

namespace anx {

// a tile probes the hash table instead of walking its window when the ball is cheaper (a probe step costs ~3 walk steps) and
// no group sum is large enough to overflow the byte-wise add of an offset
__host__ __device__ inline bool tile_probes(uint32_t balln, uint32_t window, unsigned long long sig) {
  if (balln == 0 || (unsigned long long)balln * 3ull >= window) return false;
  for (int g = 0; g < 8; ++g)
    if (((sig >> (8 * g)) & 0xFFu) > 120u) return false;
  return true;
}
inline bool probe_enabled() { return !switches().scan_walk_flat; }

// ---- runtime.hip: what the engine keeps per device, no kernel -----------------------------------------------------------------------------
// Kernel timer (off unless anx_debug_kernel_timer(1)): HIP events around the launches of the kernels that dominate the
// configurations bench.py reports (k_scan_bits, k_filter_score, k_conf_script, k_lattice), on the launch stream; resolved lazily
// when the totals are read.  ktimer_begin returns a handle (or -1 when off) for ktimer_end.
int ktimer_begin(const char* name, hipStream_t st);
void ktimer_end(int handle, hipStream_t st);
// per-device scratch pool: freed blocks are kept for the next batch
hipError_t pool_malloc(void** p, size_t bytes);
void pool_free(void* p);
// the lexicons resident on a device: the last one to leave empties the device's pool (idle small-call contexts, cached blocks, shells)
void lexicon_registered(int device);
void lexicon_released(int device);   // (the current device is `device`)
// the idle contexts of the small call (engine.hip small_path.hpp, where they are made): destroyed before a pool is emptied
void small_ctxs_destroy(int device);
// a non-blocking stream on the current device (high: at the device's highest priority), or nullptr
void* make_stream(bool high);
// non-blocking stream for one call of the device-side encoder (kept per device, reused)
hipStream_t encoder_stream_acquire(int device);
void encoder_stream_release(int device, hipStream_t s);
// the library's own two streams for asynchronous runs, alternately (the current device is `device`); nullptr: none
hipStream_t run_stream_next(int device);
// events + pinned read-back block (pinned_bytes) of a batch: from the shells of the device's freed batches, created when there is none
struct BatchShell;
int shell_acquire(int device, BatchShell& sh, size_t pinned_bytes, std::string& err);
void shell_release(int device, BatchShell& sh);
// The calling thread's current HIP device is not ours to change: entry points that run on a CALLER's thread (model upload / free,
// stream create / destroy, pool trim) switch to the replica's device and put the caller's back when they return.
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); } }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// confusable weighting on the device (conf.hip)
struct DeviceConf;
void conf_free(DeviceConf*);
int conf_launch(const HostModel& m, const DeviceLexicon* dl, Batch* b, hipStream_t st, bool early, uint32_t row_cap, std::string& err);
// The same chain for the small call (small_path.hpp): the context's fixed buffers instead of a Batch's, so no allocation, no memset
// command (ctr is among the words k_small_tiles clears) and no sort library -- k_small_conf_order, one block, stands in for
// k_conf_key + k_conf_iota + the radix sort.  Four launches: screen, order, script, apply.
struct SurvRow;
struct DevRow;
struct SmallConf {
  double* weight = nullptr;        // [row_cap] per row slot
  uint2* need = nullptr;           // [row_cap] (row slot, query) that need an edit script: never more than there are rows
  uint32_t* key = nullptr;         // [row_cap] shape key per list entry
  uint32_t* order = nullptr;       // [row_cap] list positions by shape key
  uint32_t* ctr = nullptr;         // [8]: [0] list length, [1] rows the device could not weight
  uint32_t* work = nullptr;        // k_conf_script's working set for work_blocks one-wave blocks
  uint32_t work_blocks = 0;
};
struct SmallConfRun {
  uint32_t nq, row_cap;
  bool early;
  const uint32_t *soff, *r_count, *overflow, *q_orig;
  const uint8_t* text;             // the inputs on the device (SmallEnc::text / textoff)
  const uint32_t* textoff;
  SurvRow* c_rows;
  DevRow* r_rows;
  double cutoff_threshold;
  float freq_weight;
};
size_t conf_small_work_bytes(uint32_t blocks);
int conf_launch_small(const HostModel& m, const DeviceLexicon* dl, hipStream_t st, const SmallConf& cb, const SmallConfRun& r, uint32_t* r_count, std::string& err);
// the signature adjacency lists built on the device (adjacency.hip); host copies of its table and headers for the host encoder
int adjacency_build_device(DeviceLexicon* d, const LexiconImage& img, int closure, size_t budget_bytes, AdjIndex& stats, std::string& err);
int adjacency_host_copies(const DeviceLexicon* d, std::string& err);
// search mode's LM tables of a replica (lattice.hip)
struct DeviceLm;
void lm_free(DeviceLm*);
// device-side query encoder (encode.hip): fills the query and tile arrays of `b` from the packed inputs
int batch_encode_device(const HostModel& m, const DeviceLexicon* dl, Batch* b, const char* blob, size_t blob_bytes, const uint32_t* off, size_t n,
                        const anx_params& p, std::string& err, bool blob_on_device = false, bool after_stream = false, void* src_stream = nullptr);

// ---- the small call: device buffers of its encoder (engine.hip small_find owns them; encode.hip launches the kernels) -----------------
struct Tile;
struct SmallEnc {
  uint8_t* codes = nullptr;
  uint32_t *meta = nullptr, *bits = nullptr, *kind = nullptr, *cv = nullptr, *blk = nullptr, *perm = nullptr;
  unsigned long long *key = nullptr, *sig = nullptr;
  uint4 *q_rec = nullptr, *q_rows = nullptr;
  uint32_t *q_bits = nullptr, *q_cv = nullptr, *q_meta = nullptr, *q_orig = nullptr, *qexact = nullptr, *s_kind = nullptr;
  unsigned long long* s_sig = nullptr;
  Tile* tiles = nullptr;  // [slots * inputs] (8 * SMALL_MAX in all): slot of (query s, part) = part * n + s
  // confusable models: k_enc_strings<true> leaves the bytes it staged in LDS, and the offsets, on the device (conf.hip reads them: no copy
  // command, no byte-wise walk of pinned host memory).  Input i = text[textoff[i] .. textoff[i + 1] - 1).  nullptr: not kept
  uint8_t* text = nullptr;
  uint32_t* textoff = nullptr;
};
struct SmallZero { uint32_t* p[8]; uint32_t n[8]; };  // arrays k_small_tiles clears before the run (unused entries: n = 0)
// k_enc_strings -> k_enc_gather (identity order) -> k_small_tiles on `st`: no allocation, no host wait.  blob / off may be pinned host
// memory (read over PCIe; stage_lds: every block of k_enc_strings first copies its strings into LDS, inputs of <= 64 bytes).  qw: 16-byte words per query row (from the host's bound of the longest input)
int small_encode_launch(const HostModel& m, const DeviceLexicon* dl, const SmallEnc& e, const uint8_t* blob, const uint32_t* off, uint32_t n, uint32_t qw,
                        const anx_params& p, const SmallZero& z, uint32_t slots, bool stage_lds, const uint32_t* host_off, hipStream_t st, std::string& err);  // host_off: the offsets as the HOST reads them (stage_lds: the blocks' byte ranges go into the kernel arguments)  // slots: tile slots per query (>= 8)
int small_iota(uint32_t* perm, uint32_t n, hipStream_t st);
// Where the encoder puts the codes of string i: the bytes of string i and its separator are >= symbols + 1, and rounding every start up
// to a dword plus one dword per string keeps the regions disjoint (start(i+1) - start(i) is a multiple of 4 that is >= symbols + 2).
// The buffer holds blob bytes + 4 n + 16.
__host__ __device__ inline uint32_t code_off(uint32_t off_i, uint32_t i) { return ((off_i + 3u) & ~3u) + 4u * i; }

// ---- anx_score_pairs (pairs.hip): caller-chosen pairs, scored by the model's measures ---------------------------------------------------
// the normaliser alone over n strings on the device (encode.hip): of `e` the fields codes, meta, bits, sig, kind, cv, key, blk are used
int pairs_encode_launch(const HostModel& m, const DeviceLexicon* dl, const SmallEnc& e, const uint8_t* blob, const uint32_t* off, uint32_t n, hipStream_t st,
                        std::string& err);
// anx_score_pairs_weighted: the confusable weights of a chunk's pairs (conf.hip k_pairs_conf_screen + k_pairs_conf_script), enqueued on
// `st` behind the pair kernels.  Both sides are read from the chunk's uploaded blob (string p and string n + p); the pattern tables are
// the replica's (uploaded on first use, without the vocabulary copy the batch path keeps).  work: conf_small_work_bytes(work_blocks).
constexpr uint32_t PAIRS_CF_BLOCKS = 2048;  // one-wave blocks of k_pairs_conf_script at most (it strides): 2048 x 371 KB = 760 MB for a full chunk
struct PairConfRun {
  uint32_t n;
  const uint8_t* blob;
  const uint32_t* off;             // [2 n + 1]
  const anx_pair_score* rec;       // [n] the records the pair kernels wrote
  double* weight;                  // [n]: 1.0, the weight, or NaN = left to the host
  uint32_t* need;                  // [n]
  uint32_t* ctr;                   // [4]: [0] pairs listed for a script, [1] pairs left to the host
  uint32_t* work;
  uint32_t work_blocks;
  uint32_t* sort;                  // [3 n]: shape keys | sorted keys | the list in shape-key order
  void* sort_tmp;                  // conf_pairs_sort_tmp_bytes(n)
  size_t sort_tmp_bytes;
};
size_t conf_pairs_sort_tmp_bytes(uint32_t n);
int conf_launch_pairs(const HostModel& m, const DeviceLexicon* dl, hipStream_t st, const PairConfRun& r, std::string& err);
// What the confusable sweep (csweep.hip) uses of conf.hip.  conf_vocab_view: the replica's copy of the vocabulary (code points,
// offsets [V + 1], presence bits [V]) and the alphabetic ranges, uploaded on first use -- the vocabulary half of what conf_launch
// ensures, for a model that owns no list.  conf_sort_enqueue: conf_launch_pairs' radix pass over 13 key bits (tmp of
// conf_pairs_sort_tmp_bytes(n)).  conf_apply_late_enqueue: k_conf_apply_late (weight, stable re-sort, cutoff, new count) over rows
// ranked by rank_rows_enqueue: weight[soff[s] + j] belongs to ranked row j of query s.
struct ConfVocabView {
  const uint32_t* v_pool; const uint32_t* v_off; const cdiff::CharSet* v_cs; uint32_t nvocab;
  const uint32_t (*alpha)[2]; uint32_t nalpha;
};
int conf_vocab_view(const HostModel& m, const DeviceLexicon* dl, ConfVocabView* v, std::string& err);
int conf_sort_enqueue(void* tmp, size_t tmp_bytes, const uint32_t* keys, uint32_t* keys_out, const uint32_t* vals, uint32_t* vals_out, uint32_t n, hipStream_t st,
                      std::string& err);
void conf_apply_late_enqueue(hipStream_t st, uint32_t nq, uint32_t row_cap, const uint32_t* soff, DevRow* r_rows, const double* weight, const uint32_t* overflow,
                             double cutoff_threshold, float freq_weight, uint32_t* r_count);
// pairs_encode_launch with the caller's thresholds behind meta's k / d bits (anx_evaluate_gold reads them there)
int pairs_encode_launch_thr(const HostModel& m, const DeviceLexicon* dl, const SmallEnc& e, const uint8_t* blob, const uint32_t* off, uint32_t n,
                            const anx_params& thr, hipStream_t st, std::string& err);
// Pool blocks that go back to the current device's pool together.  The owner calls release() once nothing enqueued may still use them
// (it waits for its stream first): a call (PairScratch), a group of the weight sweep, a set of the sweep.
struct PoolBlocks {
  std::vector<void*> v;
  template <typename T>
  int get(T** p, size_t count, std::string& err) {
    void* q = nullptr;
    const size_t bytes = count * sizeof(T) < 16 ? 16 : count * sizeof(T);
    const hipError_t e = pool_malloc(&q, bytes);
    if (e != hipSuccess) { err = std::string("pool_malloc: ") + hipGetErrorString(e); return ANX_ENODEVICE; }
    v.push_back(q);
    *p = static_cast<T*>(q);
    return ANX_OK;
  }
  void release() {
    for (void* q : v) pool_free(q);
    v.clear();
  }
};
// pool blocks and pinned host blocks of one call released together, and the private stream of the call
struct PairScratch {
  PoolBlocks blocks;
  std::vector<void*> host;
  int device;
  hipStream_t st;
  explicit PairScratch(int dev) : device(dev), st(encoder_stream_acquire(dev)) {}
  PairScratch(const PairScratch&) = delete;
  PairScratch& operator=(const PairScratch&) = delete;
  template <typename T>
  int get(T** p, size_t count, std::string& err) { return blocks.get(p, count, err); }
  void* pinned(size_t bytes) {
    void* q = host_result_alloc(bytes < 16 ? 16 : bytes);
    if (q) host.push_back(q);
    return q;
  }
  // nothing enqueued by this call may still use the blocks when they return to their pools (an error path has not waited yet)
  ~PairScratch() {
    (void)hipStreamSynchronize(st);
    blocks.release();
    for (void* q : host) host_result_free(q);
    encoder_stream_release(device, st);
  }
};
// The front half of score_pairs_chunk (pairs.hip): staging, one upload, the encoder over the 2 n strings and the pair kernels, all
// enqueued on sc.st; the records stay on the device.  thr: the thresholds behind meta's k / d bits (nullptr: Absolute(0), nobody reads them).
struct PairsOnDevice {
  const uint8_t* blob = nullptr;   // the 2 n strings: a of pair i = string i, its b = string n + i
  const uint32_t* off = nullptr;   // [2 n + 1]
  SmallEnc e;                      // codes, meta, bits, kind, cv, key, sig, blk
  anx_pair_score* out = nullptr;   // [n]
};
int pairs_chunk_enqueue(const HostModel& m, const DeviceLexicon* dl, const PairSpan* a, const PairSpan* b, size_t n, const anx_params* thr, PairScratch& sc,
                        PairsOnDevice& pd, std::string& err);

// ---- results.hip: what the weight sweep (reweigh.hip) uses of the rows' way off the device ------------------------------------------------
// the measures behind the rows of a shard's gathered section, on the gather's device (next to batch_fetch_measures_into)
int batch_gather_measures(const HostModel& m, const DeviceLexicon* dl, const Batch* b, int dst_device, void* dst, size_t capacity, void* stream, std::string& err);
// dl->vocab_ent (vocabulary id -> lexicon entry), built on first use as anx_batch_fetch_measures builds it; waits on st
int replica_vocab_entries(const HostModel& m, const DeviceLexicon* dl, hipStream_t st, std::string& err);
// ---- engine.hip: what results.hip and reweigh.hip use of the run's translation unit ------------------------------------------------------
// the run's exclusive prefix sum (kernels_prefix.hpp): out[n + 1]; tmp: prefix_scan_tmp_bytes(n); copy: nullptr or a second array for out[0 .. n)
size_t prefix_scan_tmp_bytes(size_t n);
int prefix_scan_enqueue(const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* tmp, hipStream_t st, uint32_t* copy);
// launch_rank (launch_plan.hpp) for rows of a model without variant lists and without segments: k_rank<true | false> as a run launches it
struct RankPlain { double cutoff_threshold; uint64_t max_matches; float freq_weight; int have_freq; };
void rank_rows_enqueue(const RankPlain& r, hipStream_t st, uint32_t nq, const uint32_t* soff, const SurvRow* c_rows, const uint32_t* qmaxfreq, double* t_key, DevRow* r_rows,
                       uint32_t* r_count, uint32_t row_cap, const uint32_t* overflow);

// ---- the vocabulary table of learn mode and anx_evaluate_gold (built by learn.hip): text hash -> id -----------------------------------------
struct LearnVocab {
  int device = -1;
  size_t V = 0;
  uint8_t* pool = nullptr;
  uint32_t* voff = nullptr;
  unsigned long long* vh = nullptr;
  uint32_t* slots = nullptr;
  uint32_t mask = 0;
  unsigned long long hmask = 0;  // what lf_hash keeps of FNV-1a (the table's hashes and the lookups' must agree)
};
constexpr uint32_t LF_EMPTY = 0xFFFFFFFFu;    // free table slot
// FNV-1a under hmask: its low 63 bits, or fewer under the test switch ANX_LEARN_HASH_BITS (collisions on demand)
__device__ inline unsigned long long lf_hash(const uint8_t* p, uint32_t len, unsigned long long hmask) {
  unsigned long long h = 1469598103934665603ull;
  for (uint32_t i = 0; i < len; ++i) { h ^= p[i]; h *= 1099511628211ull; }
  return h & hmask;
}
__device__ inline bool lf_eq(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb) {
  if (la != lb) return false;
  for (uint32_t i = 0; i < la; ++i)
    if (a[i] != b[i]) return false;
  return true;
}
// the table of `m`'s vocabulary on `device` in *cache: built on first use, rebuilt when the vocabulary size or ANX_LEARN_HASH_BITS changed
// (the caller holds the learn lock); waits on `st`
int learn_vocab_ensure(const HostModel& m, int device, LearnVocab** cache, hipStream_t st, std::string& err);

}  // namespace anx
