// sweep.hip -- anx_evaluate_sweep: several parameter sets over the same (input, gold) pairs, the summary reduced on the device (gfx950 / CDNA4).
//
// What anx_evaluate_gold computes for ONE parameter set splits into a part that does not depend on the set and a part that does:
//   once per chunk (sweep_chunk_begin, resident until sweep_chunk_end):
//     pairs_chunk_enqueue (pairs.hip) : one upload of the 2 n strings, k_enc_strings WITHOUT thresholds (as anx_score_pairs runs it: meta
//                       holds the symbol count, the clamped k / d follow from it per set), the pair kernels
//     k_sweep_lookup  : one lane per gold string: learn mode's vocabulary table -> gold id or none (eval.hip's probe)
//     the upload of the vocabulary flags
//   once per set (sweep_chunk_set; the ranked rows under that set were gathered onto this device by sweep_capi.cpp):
//     k_sweep_sections: per input: row count, section, first record
//     k_sweep_rows    : flat over the gathered rows, rank of the gold row by atomicMin
//     k_sweep_classify: one lane per pair: the record k_eval_classify writes, with k / d clamped from the set's thresholds and the
//                       symbol count (dev_clamp_threshold restated), stored only when the caller asked for records; then the
//                       reduction: the block collects the 78 counters of anx_gold_summary in LDS (76 32-bit cells, two 64-bit
//                       cells for rr_fixed and n_results: 320 bytes), the waves add ballot counts and shuffle sums, and after the
//                       barrier one 64-bit integer atomicAdd per non-zero counter goes to the set's summary in HBM.  Integers only: the
//                       result does not depend on the order in which the blocks arrive.
//   and a download of 624 bytes per set (+ 32 n when the records are asked for).
// The classification restates eval.hip's (as kernels_explain.hpp restates the pair DL): eval.hip keeps its kernels, launches and bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "sweep.h"

namespace anx {

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      err = std::string(#expr) + ": " + hipGetErrorString(_e);                                 \
      return ANX_ENODEVICE;                                                                    \
    }                                                                                          \
  } while (0)

#include "kernels_common.hpp"

namespace {
constexpr uint32_t SW_NONE = 0xFFFFFFFFu;  // no such vocabulary item / no such row
constexpr int SW_BLOCK = 256;
constexpr uint32_t SW_COUNTERS = sizeof(anx_gold_summary) / sizeof(uint64_t);  // 78, in the struct's order
constexpr uint32_t SW_CELLS32 = SW_COUNTERS - 2;                               // all but rr_fixed and n_results
// counter index = offset in anx_gold_summary / 8
constexpr uint32_t SW_N = 0, SW_KNOWN = 1, SW_REASON = 2, SW_HIST = 10, SW_RR = 74, SW_NRES = 75, SW_GAINED = 76, SW_LOST = 77;
static_assert(SW_COUNTERS == 78 && SW_HIST + ANX_GOLD_RANK_BINS == SW_RR, "the counters follow anx_gold_summary's layout");
inline unsigned grid_of(size_t n) { return (unsigned)std::max<size_t>(1, (n + SW_BLOCK - 1) / SW_BLOCK); }

std::atomic<uint64_t> g_stats[SWEEP_NSTATS];
}  // namespace

void sweep_stats_add(int which, uint64_t v) {
  if (which >= 0 && which < SWEEP_NSTATS) g_stats[which].fetch_add(v, std::memory_order_relaxed);
}
void sweep_stats(uint64_t out[SWEEP_NSTATS]) {
  for (int i = 0; i < SWEEP_NSTATS; ++i) out[i] = g_stats[i].load(std::memory_order_relaxed);
}

struct SweepSection { const anx_topk_record* rec; const uint32_t* off; const uint32_t* idx; uint32_t n, lo, rows; };

__global__ __launch_bounds__(SW_BLOCK) void k_sweep_sections(SweepSection sec, uint32_t sid, uint32_t n, uint32_t* __restrict__ cnt,
                                                             uint32_t* __restrict__ src_sec, uint32_t* __restrict__ src_row) {
  const uint32_t j = blockIdx.x * SW_BLOCK + threadIdx.x;
  if (j >= sec.n) return;
  const uint32_t i = sec.idx ? sec.idx[j] : sec.lo + j;
  if (i >= n) return;
  const uint32_t r0 = sec.off[j], r1 = sec.off[j + 1];
  if (r1 < r0 || r1 > sec.rows) return;  // (offsets that do not describe this section: the input keeps no rows)
  cnt[i] = r1 - r0;
  src_sec[i] = sid;
  src_row[i] = r0;
}

// gold string i = string n + i of the chunk's blob
__global__ __launch_bounds__(SW_BLOCK) void k_sweep_lookup(uint32_t n, const uint8_t* __restrict__ blob, const uint32_t* __restrict__ off,
                                                           const uint8_t* __restrict__ pool, const uint32_t* __restrict__ voff,
                                                           const unsigned long long* __restrict__ vh, const uint32_t* __restrict__ slots, uint32_t mask,
                                                           unsigned long long hmask, uint32_t* __restrict__ gid) {
  const uint32_t i = blockIdx.x * SW_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint8_t* a = blob + off[n + i];
  const uint32_t la = off[n + i + 1u] - off[n + i] - 1u;  // (each string is followed by a NUL byte)
  const unsigned long long h = lf_hash(a, la, hmask);
  uint32_t found = SW_NONE;
  for (uint32_t s = (uint32_t)h & mask, step = 0; step <= mask; s = (s + 1) & mask, ++step) {
    const uint32_t v = slots[s];
    if (v == LF_EMPTY) break;
    if (vh[v] == h && lf_eq(a, la, pool + voff[v], voff[v + 1] - voff[v])) { found = v; break; }
  }
  gid[i] = found;
}

__global__ __launch_bounds__(SW_BLOCK) void k_sweep_rows(SweepSection sec, uint32_t n, const uint32_t* __restrict__ gid, uint32_t* __restrict__ rank) {
  const uint32_t r = blockIdx.x * SW_BLOCK + threadIdx.x;
  if (r >= sec.rows || sec.n == 0u) return;
  const uint32_t vocab = sec.rec[r].vocab_id;
  // the last j in [0, sec.n) with off[j] <= r: inputs without rows share their offset with the next one and are stepped over
  uint32_t lo = 0, hi = sec.n - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (sec.off[mid] <= r) lo = mid;
    else hi = mid - 1u;
  }
  const uint32_t r0 = sec.off[lo];
  if (r0 > r) return;
  const uint32_t i = sec.idx ? sec.idx[lo] : sec.lo + lo;
  if (i >= n) return;
  const uint32_t g = gid[i];
  if (g != SW_NONE && g == vocab) atomicMin(&rank[i], r - r0);
}

struct SweepKArgs {
  uint32_t n;
  const uint32_t* meta;             // [2 n] k_enc_strings: symbols | .. ; 0 = empty or more than 255 symbols (the k / d bits are not used)
  const uint32_t* kind;             // [2 n] 0: the count vector is in cv; else it follows from the planes
  const uint32_t* cv;               // [2 n][NP]
  const uint4* bits;                // [2 n] thermometer planes
  const unsigned long long* sig;    // [2 n]
  int NP;
  const anx_pair_score* pair;       // [n]
  const uint32_t *gid, *rank, *cnt, *src_sec, *src_row;
  const SweepSection* secs;
  const uint8_t* vflags;            // [V] ANX_VOCAB_* bits per vocabulary item
  uint32_t V;
  const uint4* sigtab;              // the lexicon's signature table and classes (DeviceLexicon::sig, cls_planes)
  const uint32_t* siglen_begin;
  const uint32_t* cls_planes;
  uint32_t cstride;
  anx_threshold kth, dth;           // the set's max_anagram_distance / max_edit_distance
  int stop_exact;
  double score_threshold;
  uint8_t* at1_base;                // [n] gold at rank 0 under sets[0]
  int baseline;                     // this pass is sets[0]'s: it writes at1_base
  unsigned long long* summary;      // [SW_COUNTERS] the set's anx_gold_summary on the device
  uint4* out;                       // [n][2] the records, or nullptr
};

// host_model.cpp clamp_threshold, as encode.hip's dev_clamp_threshold
__device__ inline uint32_t sw_clamp_threshold(const anx_threshold& t, int len, int absolute_max) {
  if (t.kind == ANX_RATIO || t.kind == ANX_RATIO_WITH_LIMIT) {
    const float v = floorf((float)len * t.ratio);
    const int x = v < 0.0f ? 0 : v > 255.0f ? 255 : (int)v;
    const int lim = t.kind == ANX_RATIO ? absolute_max : (int)t.value;
    return (uint32_t)(x < lim ? x : lim);
  }
  const int half = len / 2 < 255 ? len / 2 : 255;
  return (uint32_t)((int)t.value < half ? (int)t.value : half);
}
// dword w of the count vector (4 symbol slots, a byte each) of a string whose counts are all <= 4, from its thermometer planes (as encode.hip)
__device__ inline uint32_t sw_cv_word_of_planes(const uint4 pl, uint32_t w) {
  uint32_t word = 0;
  if (w < 8u) {
#pragma unroll
    for (uint32_t y = 0; y < 4u; ++y) {
      const uint32_t sl = 4u * w + y;
      word |= (((pl.x >> sl) & 1u) + ((pl.y >> sl) & 1u) + ((pl.z >> sl) & 1u) + ((pl.w >> sl) & 1u)) << (8u * y);
    }
  }
  return word;
}
__device__ inline uint32_t sw_cv_word(const SweepKArgs& k, uint32_t s, uint32_t kind, const uint4 pl, uint32_t w) {
  return kind ? sw_cv_word_of_planes(pl, w) : k.cv[(size_t)s * (size_t)k.NP + w];
}
// floor(2^32 / (rank + 1)) in 32-bit arithmetic for rank >= 1: 2^32 = 0xFFFFFFFF + 1
__device__ inline unsigned long long sw_rr_fixed(uint32_t rank) {
  if (rank == 0u) return 1ull << 32;
  const uint32_t d = rank + 1u, q = 0xFFFFFFFFu / d, r = 0xFFFFFFFFu - q * d;
  return (unsigned long long)(q + (r + 1u == d ? 1u : 0u));
}
__device__ inline unsigned long long sw_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
  return v;
}

__global__ __launch_bounds__(SW_BLOCK) void k_sweep_classify(SweepKArgs k) {
  __shared__ unsigned long long s_wide[2];   // rr_fixed, n_results
  __shared__ uint32_t s_cell[SW_CELLS32];    // the other counters in the struct's order, gained / lost behind the histogram
  for (uint32_t x = threadIdx.x; x < SW_CELLS32; x += SW_BLOCK) s_cell[x] = 0u;
  if (threadIdx.x < 2u) s_wide[threadIdx.x] = 0ull;
  __syncthreads();
  const uint32_t i = blockIdx.x * SW_BLOCK + threadIdx.x;
  const bool live = i < k.n;
  uint32_t reason = 8u, g = SW_NONE, rk = SW_NONE, cnt = 0u;  // (reason 8: a lane behind the last pair counts nowhere)
  if (live) {
    const anx_pair_score pr = k.pair[i];
    g = k.gid[i]; rk = k.rank[i]; cnt = k.cnt[i];
    const SweepSection sec = cnt ? k.secs[k.src_sec[i]] : SweepSection{};
    const uint32_t row0 = cnt ? k.src_row[i] : 0u;
    const uint32_t top = cnt ? sec.rec[row0].vocab_id : SW_NONE;
    const uint32_t ma = pr.status == ANX_OK ? k.meta[i] : 0u;
    const uint32_t len = ma & 0xFFu;
    const uint32_t kk = ma ? sw_clamp_threshold(k.kth, (int)len, kMaxAnagramDistance) : 0u;
    const uint32_t dd = ma ? sw_clamp_threshold(k.dth, (int)len, kMaxEditDistance) : 0u;
    double score = pr.score;
    if (rk != SW_NONE && rk < cnt) {
      reason = ANX_GOLD_RANKED;
      score = sec.rec[row0 + rk].dist_score;
    } else if (pr.status != ANX_OK) {
      reason = ANX_GOLD_STATUS;
    } else if (g == SW_NONE || g >= k.V || !(k.vflags[g] & ANX_VOCAB_INDEXED) || (k.vflags[g] & ANX_VOCAB_TRANSPARENT)) {
      reason = ANX_GOLD_NOT_A_RESULT;
    } else {
      // L1 of the two count vectors: NP x v_sad_u8 over the packed bytes, k_scan_sad's test
      const uint32_t ka = k.kind[i], kg = k.kind[k.n + i];
      const uint4 pa = k.bits[i], pg = k.bits[k.n + i];
      uint32_t l1 = 0;
      for (uint32_t w = 0; w < (uint32_t)k.NP; ++w) l1 = __builtin_amdgcn_sad_u8(sw_cv_word(k, i, ka, pa, w), sw_cv_word(k, k.n + i, kg, pg, w), l1);
      bool exact_stop = false;
      if (k.stop_exact && l1 != 0u) {  // the input's own anagram class: the run of its signature in its charcount range, then the count vectors
        const unsigned long long sig = k.sig[i];
        int lo = (int)k.siglen_begin[len], hi = (int)k.siglen_begin[len + 1u] - 1;
        while (lo <= hi && !exact_stop) {
          const int mid = (lo + hi) >> 1;
          const uint4 r = k.sigtab[mid];  // {sig lo, sig hi, first class, classes}
          const unsigned long long v = (unsigned long long)r.x | (unsigned long long)r.y << 32;
          if (sig < v) hi = mid - 1;
          else if (sig > v) lo = mid + 1;
          else {
            for (uint32_t c = r.z; c < r.z + r.w && !exact_stop; ++c) {
              bool eq = true;
              for (uint32_t w = 0; w < (uint32_t)k.NP; ++w) eq = eq && k.cls_planes[(size_t)w * k.cstride + c] == sw_cv_word(k, i, ka, pa, w);
              exact_stop = eq;
            }
            break;
          }
        }
      }
      if (exact_stop) reason = ANX_GOLD_EXACT_STOP;
      else if (l1 > kk || l1 >= (uint32_t)pr.len_a + (uint32_t)pr.len_b) reason = ANX_GOLD_ANAGRAM;
      else if ((uint32_t)pr.ld > dd) reason = ANX_GOLD_EDIT;
      else if (!(pr.score >= k.score_threshold)) reason = ANX_GOLD_THRESHOLD;
      else reason = ANX_GOLD_CROPPED;
    }
    if (k.out) {
      const unsigned long long sb = (unsigned long long)__double_as_longlong(score);
      const uint32_t rank_word = reason == ANX_GOLD_RANKED ? rk : 0xFFFFFFFFu;  // int32 -1
      k.out[2 * (size_t)i] = make_uint4(g, rank_word, cnt, top);
      k.out[2 * (size_t)i + 1] = make_uint4((uint32_t)sb, (uint32_t)(sb >> 32), (uint32_t)pr.ld | kk << 16 | dd << 24,
                                            ((uint32_t)(int)pr.status & 0xFFu) | reason << 8);
    }
  }
  // ---- the reduction: ballot counts and shuffle sums per wave -> LDS -> one atomic per non-zero counter and block ----
  const bool ranked = reason == ANX_GOLD_RANKED;
  const bool at1 = ranked && rk == 0u;
  bool base1 = at1;
  if (live) {
    if (k.baseline) k.at1_base[i] = at1 ? 1 : 0;
    else base1 = k.at1_base[i] != 0;
  }
  const bool lane0 = (threadIdx.x & 63u) == 0u;
  const uint32_t c_live = (uint32_t)__popcll(__ballot(live)), c_known = (uint32_t)__popcll(__ballot(live && g != SW_NONE));
  const uint32_t c_at1 = (uint32_t)__popcll(__ballot(at1));
  const uint32_t c_gained = (uint32_t)__popcll(__ballot(at1 && !base1)), c_lost = (uint32_t)__popcll(__ballot(live && !at1 && base1));
  if (lane0) {
    if (c_live) atomicAdd(&s_cell[SW_N], c_live);
    if (c_known) atomicAdd(&s_cell[SW_KNOWN], c_known);
    if (c_at1) atomicAdd(&s_cell[SW_HIST], c_at1);
    if (c_gained) atomicAdd(&s_cell[SW_GAINED - 2u], c_gained);
    if (c_lost) atomicAdd(&s_cell[SW_LOST - 2u], c_lost);
  }
#pragma unroll
  for (uint32_t r = 0; r < 8u; ++r) {
    const uint32_t c = (uint32_t)__popcll(__ballot(reason == r));
    if (lane0 && c) atomicAdd(&s_cell[SW_REASON + r], c);
  }
  if (ranked && rk != 0u) atomicAdd(&s_cell[SW_HIST + min(rk, (uint32_t)ANX_GOLD_RANK_BINS - 1u)], 1u);
  const unsigned long long w_rr = sw_wave_sum(ranked ? sw_rr_fixed(rk) : 0ull), w_res = sw_wave_sum((unsigned long long)cnt);
  if (lane0) {
    if (w_rr) atomicAdd(&s_wide[0], w_rr);
    if (w_res) atomicAdd(&s_wide[1], w_res);
  }
  __syncthreads();
  if (threadIdx.x < SW_COUNTERS) {
    const uint32_t t = threadIdx.x;
    const unsigned long long v = t < SW_RR ? (unsigned long long)s_cell[t] : t <= SW_NRES ? s_wide[t - SW_RR] : (unsigned long long)s_cell[t - 2u];
    if (v) atomicAdd(&k.summary[t], v);
  }
}

struct SweepChunk {
  const HostModel* m = nullptr;
  const DeviceLexicon* dl = nullptr;
  size_t n = 0;
  PairScratch sc;
  PairsOnDevice pd;
  std::vector<uint8_t> vflags;        // host source of an upload: lives as long as the stream may read it
  uint32_t *d_gid = nullptr, *d_per_set = nullptr;  // d_per_set: [4 n] cnt | section | first row | rank
  uint8_t *d_vflags = nullptr, *d_at1 = nullptr;
  unsigned long long* d_sum = nullptr;
  uint4* d_out = nullptr;
  char* h_down = nullptr;             // pinned: the summary | the records
  explicit SweepChunk(int dev) : sc(dev) {}
};

int sweep_chunk_begin(const HostModel& m, const DeviceLexicon* dl, LearnVocab** vocab, const PairSpan* a, const PairSpan* gold, size_t n, bool want_records,
                      SweepChunk** out, std::string& err) {
  static_assert(sizeof(anx_gold_eval) == 2 * sizeof(uint4), "the record leaves as two 16-byte stores");
  *out = nullptr;
  if (!dl) { err = "model is not resident on a device"; return ANX_ENODEVICE; }
  if (n == 0 || n > PAIRS_CHUNK) { err = "sweep_chunk_begin: a chunk holds 1 .. 2^20 pairs"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(dl->device));
  SweepChunk* c = new SweepChunk(dl->device);
  struct Guard { SweepChunk* c; ~Guard() { if (c) sweep_chunk_end(c); } } guard{c};
  c->m = &m; c->dl = dl; c->n = n;
  c->vflags.assign(std::max<size_t>(m.decoder.size(), 1), 0);
  for (size_t v = 0; v < m.decoder.size(); ++v) c->vflags[v] = m.decoder[v].vocabtype;
  hipStream_t st = c->sc.st;
  if (int rc = learn_vocab_ensure(m, dl->device, vocab, st, err)) return rc;
  const LearnVocab& t = **vocab;
  if (t.V != m.decoder.size()) { err = "sweep_chunk_begin: the vocabulary table is not this model's"; return ANX_EINVAL; }
  if (int rc = pairs_chunk_enqueue(m, dl, a, gold, n, nullptr, c->sc, c->pd, err)) return rc;
  sweep_stats_add(SWEEP_PAIR_PASSES, 1);
  int rc;
  if ((rc = c->sc.get(&c->d_gid, n, err)) || (rc = c->sc.get(&c->d_per_set, 4 * n, err)) || (rc = c->sc.get(&c->d_vflags, c->vflags.size(), err)) ||
      (rc = c->sc.get(&c->d_at1, n, err)) || (rc = c->sc.get(&c->d_sum, SW_COUNTERS, err)) || (want_records && (rc = c->sc.get(&c->d_out, 2 * n, err))))
    return rc;
  c->h_down = static_cast<char*>(c->sc.pinned(sizeof(anx_gold_summary) + (want_records ? n * sizeof(anx_gold_eval) : 0)));
  if (!c->h_down) { err = "out of host memory"; return ANX_EINVAL; }
  HIP_TRY(hipMemcpyAsync(c->d_vflags, c->vflags.data(), c->vflags.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(c->d_at1, 0, n, st));
  {
    const int kt = ktimer_begin("k_sweep_lookup", st);
    hipLaunchKernelGGL(k_sweep_lookup, dim3(grid_of(n)), dim3(SW_BLOCK), 0, st, (uint32_t)n, c->pd.blob, c->pd.off, t.pool, t.voff, t.vh, t.slots, t.mask, t.hmask,
                       c->d_gid);
    ktimer_end(kt, st);
  }
  HIP_TRY(hipGetLastError());
  sweep_stats_add(SWEEP_LOOKUPS, 1);
  guard.c = nullptr;
  *out = c;
  return ANX_OK;
}

int sweep_chunk_set(SweepChunk* c, const anx_params& p, bool baseline, const std::vector<LearnSection>& secs, const std::vector<size_t>& sec_rows,
                    anx_gold_summary* sum, anx_gold_eval* out, std::string& err) {
  static_assert(sizeof(anx_gold_summary) == SW_COUNTERS * sizeof(unsigned long long), "the summary is its counters");
  const size_t n = c->n;
  if (secs.size() != sec_rows.size()) { err = "sweep_chunk_set: sections and row counts differ"; return ANX_EINVAL; }
  if (out && !c->d_out) { err = "sweep_chunk_set: the chunk keeps no record buffer"; return ANX_EINVAL; }
  for (size_t s = 0; s < secs.size(); ++s)
    if (sec_rows[s] >= 0x7FFFFFFFull || secs[s].n > n || (!secs[s].idx && secs[s].lo + secs[s].n > n)) { err = "sweep_chunk_set: a section beyond the chunk"; return ANX_EINVAL; }
  const DeviceLexicon* dl = c->dl;
  HIP_TRY(hipSetDevice(dl->device));  // (the batch runs in between may have left another replica's device current)
  hipStream_t st = c->sc.st;
  const uint32_t n32 = (uint32_t)n;
  // the set's own blocks: the section table and the index lists; back to the pool when the set is done (a sweep has up to 256 sets)
  std::vector<SweepSection> hs(secs.size());
  std::vector<void*> mine;
  struct Release { std::vector<void*>& v; hipStream_t st; ~Release() { (void)hipStreamSynchronize(st); for (void* q : v) pool_free(q); } } release{mine, st};
  auto get = [&](void** q, size_t bytes) -> int {
    const hipError_t e = pool_malloc(q, std::max<size_t>(bytes, 16));
    if (e != hipSuccess) { err = std::string("pool_malloc: ") + hipGetErrorString(e); return ANX_ENODEVICE; }
    mine.push_back(*q);
    return ANX_OK;
  };
  void* d_secs_v = nullptr;
  if (int rc = get(&d_secs_v, secs.size() * sizeof(SweepSection))) return rc;
  SweepSection* d_secs = static_cast<SweepSection*>(d_secs_v);
  for (size_t s = 0; s < secs.size(); ++s) {
    const LearnSection& L = secs[s];
    const size_t off_bytes = ((L.n + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
    hs[s].off = static_cast<const uint32_t*>(L.base);
    hs[s].rec = reinterpret_cast<const anx_topk_record*>(static_cast<const char*>(L.base) + off_bytes);
    hs[s].n = (uint32_t)L.n;
    hs[s].lo = (uint32_t)L.lo;
    hs[s].rows = (uint32_t)sec_rows[s];
    hs[s].idx = nullptr;
    if (L.idx && L.n) {
      void* d_idx = nullptr;
      if (int rc = get(&d_idx, L.n * sizeof(uint32_t))) return rc;
      HIP_TRY(hipMemcpyAsync(d_idx, L.idx, L.n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      hs[s].idx = static_cast<const uint32_t*>(d_idx);
    }
  }
  if (!hs.empty()) HIP_TRY(hipMemcpyAsync(d_secs, hs.data(), hs.size() * sizeof(SweepSection), hipMemcpyHostToDevice, st));
  uint32_t *d_cnt = c->d_per_set, *d_sec = d_cnt + n, *d_srow = d_sec + n, *d_rank = d_srow + n;
  HIP_TRY(hipMemsetAsync(d_cnt, 0, 3 * n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(d_rank, 0xFF, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(c->d_sum, 0, sizeof(anx_gold_summary), st));
  for (size_t s = 0; s < hs.size(); ++s)
    if (hs[s].n) hipLaunchKernelGGL(k_sweep_sections, dim3(grid_of(hs[s].n)), dim3(SW_BLOCK), 0, st, hs[s], (uint32_t)s, n32, d_cnt, d_sec, d_srow);
  {
    const int kt = ktimer_begin("k_sweep_rows", st);
    for (size_t s = 0; s < hs.size(); ++s)
      if (hs[s].n && hs[s].rows) hipLaunchKernelGGL(k_sweep_rows, dim3(grid_of(hs[s].rows)), dim3(SW_BLOCK), 0, st, hs[s], n32, c->d_gid, d_rank);
    ktimer_end(kt, st);
  }
  const PairsOnDevice& pd = c->pd;
  SweepKArgs k{};
  k.n = n32; k.meta = pd.e.meta; k.kind = pd.e.kind; k.cv = pd.e.cv; k.bits = reinterpret_cast<const uint4*>(pd.e.bits); k.sig = pd.e.sig;
  k.NP = dl->nplanes; k.pair = pd.out;
  k.gid = c->d_gid; k.rank = d_rank; k.cnt = d_cnt; k.src_sec = d_sec; k.src_row = d_srow; k.secs = d_secs;
  k.vflags = c->d_vflags; k.V = (uint32_t)c->m->decoder.size();
  k.sigtab = dl->sig; k.siglen_begin = dl->alpha.siglen_begin; k.cls_planes = dl->cls_planes; k.cstride = dl->cstride;
  k.kth = p.max_anagram_distance; k.dth = p.max_edit_distance;
  k.stop_exact = p.stop_at_exact_match ? 1 : 0;
  k.score_threshold = p.score_threshold;
  k.at1_base = c->d_at1; k.baseline = baseline ? 1 : 0;
  k.summary = c->d_sum;
  k.out = out ? c->d_out : nullptr;
  {
    const int kt = ktimer_begin("k_sweep_classify", st);
    hipLaunchKernelGGL(k_sweep_classify, dim3(grid_of(n)), dim3(SW_BLOCK), 0, st, k);
    ktimer_end(kt, st);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c->h_down, c->d_sum, sizeof(anx_gold_summary), hipMemcpyDeviceToHost, st));
  if (out) HIP_TRY(hipMemcpyAsync(c->h_down + sizeof(anx_gold_summary), c->d_out, n * sizeof(anx_gold_eval), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  sweep_stats_add(SWEEP_BYTES_DOWN, sizeof(anx_gold_summary) + (out ? n * sizeof(anx_gold_eval) : 0));
  const uint64_t* got = reinterpret_cast<const uint64_t*>(c->h_down);
  uint64_t* acc = reinterpret_cast<uint64_t*>(sum);
  for (uint32_t j = 0; j < SW_COUNTERS; ++j) acc[j] += got[j];
  if (out) memcpy(out, c->h_down + sizeof(anx_gold_summary), n * sizeof(anx_gold_eval));
  return ANX_OK;
}

int sweep_chunk_pairs(SweepChunk* c, anx_pair_score* pairs, std::string& err) {
  HIP_TRY(hipSetDevice(c->dl->device));
  const size_t bytes = c->n * sizeof(anx_pair_score);
  void* h = c->sc.pinned(bytes);
  if (!h) { err = "out of host memory"; return ANX_EINVAL; }
  HIP_TRY(hipMemcpyAsync(h, c->pd.out, bytes, hipMemcpyDeviceToHost, c->sc.st));
  HIP_TRY(hipStreamSynchronize(c->sc.st));
  sweep_stats_add(SWEEP_BYTES_DOWN, bytes);
  memcpy(pairs, h, bytes);
  return ANX_OK;
}

void sweep_chunk_view(const SweepChunk* c, SweepChunkView* v) {
  *v = SweepChunkView{c->m, c->dl, c->n, c->sc.st, c->pd.e.meta, c->pd.e.kind, c->pd.e.cv, c->pd.e.bits, c->pd.e.sig, c->pd.out, c->d_gid, c->d_vflags, c->d_at1};
}

void sweep_chunk_end(SweepChunk* c) {
  if (!c) return;
  (void)hipSetDevice(c->dl->device);  // (the scratch returns its blocks to the current device's pool)
  delete c;
}

}  // namespace anx
