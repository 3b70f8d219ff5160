// eval.hip -- anx_evaluate_gold: where a gold answer ended up in the ranked rows, and which stage lost it (gfx950 / CDNA4).
//
// The caller has pairs (input, correct form).  The ranked rows of the inputs are on this device already, as compact export sections
// in input order (eval_capi.cpp ran the batch pipeline and gathered every shard here: anx_batch_gather_compact_via, the layout learn
// mode folds).  This file joins them with what the engine can say about the direct pair, without a host round trip in between:
//   pairs_chunk_enqueue (pairs.hip) : one upload of the chunk's 2 n strings, k_enc_strings with the CALLER's thresholds (count vectors or
//                     thermometer planes, signature, symbols and the clamped k / d in meta), the pair kernels (unbounded Damerau-
//                     Levenshtein, score) -- the records stay on the device
//   k_eval_sections : per input: row count, section, first record (one lane per input of a section)
//   k_eval_lookup   : one lane per gold string: FNV-1a of its bytes, probe of learn mode's vocabulary table (LearnVocab, k_lf_lookup's
//                     probe: every candidate is checked byte by byte) -> gold id or none
//   k_eval_rows     : FLAT over the gathered rows of a section, the lanes of a wave on consecutive records (coalesced): each lane finds
//                     its input by binary search in the section's offsets (the upper levels are shared by the whole wave: cache hits) and,
//                     where the record's vocabulary id is the input's gold id, writes rank = row - off[input] with atomicMin (rows
//                     are deduplicated: the min is a guard only)
//   k_eval_classify : one lane per input: n_results / top row from the offsets, L1 of the two packed u8 count vectors (NP x v_sad_u8:
//                     k_scan_sad's candidate test), the input's exact anagram class (the binary search k_enc_gather runs), the gold
//                     item's type flags, the pair record -> reason; the 32-byte record leaves as two 16-byte stores
// and one download of 32 n bytes (+ 24 n when the pair records are asked for).  Every buffer is a block of the device pool, the
// stream one of the encoder's pool; nothing outlives the call but the vocabulary table (under learn mode's lock).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.h"

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
constexpr uint32_t EV_NONE = 0xFFFFFFFFu;  // no such vocabulary item / no such row
constexpr int EV_BLOCK = 256;
inline unsigned grid_of(size_t n) { return (unsigned)std::max<size_t>(1, (n + EV_BLOCK - 1) / EV_BLOCK); }
}  // namespace

struct EvalSection { const anx_topk_record* rec; const uint32_t* off; const uint32_t* idx; uint32_t n, lo, rows; };

__global__ __launch_bounds__(EV_BLOCK) void k_eval_sections(EvalSection sec, uint32_t sid, uint32_t n, uint32_t* __restrict__ cnt,
                                                            uint32_t* __restrict__ src_sec, uint32_t* __restrict__ src_row) {
  const uint32_t j = blockIdx.x * EV_BLOCK + threadIdx.x;
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
__global__ __launch_bounds__(EV_BLOCK) void k_eval_lookup(uint32_t n, const uint8_t* __restrict__ blob, const uint32_t* __restrict__ off,
                                                          const uint8_t* __restrict__ pool, const uint32_t* __restrict__ voff,
                                                          const unsigned long long* __restrict__ vh, const uint32_t* __restrict__ slots, uint32_t mask,
                                                          unsigned long long hmask, uint32_t* __restrict__ gid) {
  const uint32_t i = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint8_t* a = blob + off[n + i];
  const uint32_t la = off[n + i + 1u] - off[n + i] - 1u;  // (each string is followed by a NUL byte)
  const unsigned long long h = lf_hash(a, la, hmask);
  uint32_t found = EV_NONE;
  for (uint32_t s = (uint32_t)h & mask, step = 0; step <= mask; s = (s + 1) & mask, ++step) {
    const uint32_t v = slots[s];
    if (v == LF_EMPTY) break;
    if (vh[v] == h && lf_eq(a, la, pool + voff[v], voff[v + 1] - voff[v])) { found = v; break; }
  }
  gid[i] = found;
}

__global__ __launch_bounds__(EV_BLOCK) void k_eval_rows(EvalSection sec, uint32_t n, const uint32_t* __restrict__ gid, uint32_t* __restrict__ rank) {
  const uint32_t r = blockIdx.x * EV_BLOCK + threadIdx.x;
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
  if (g != EV_NONE && g == vocab) atomicMin(&rank[i], r - r0);
}

struct EvalKArgs {
  uint32_t n;
  const uint32_t* off;              // [2 n + 1] byte offsets of the chunk's strings
  const uint32_t* meta;             // [2 n] k_enc_strings: symbols | k << 8 | d << 16 | ..; 0 = empty or more than 255 symbols
  const uint32_t* kind;             // [2 n] 0: the count vector is in cv; else it follows from the planes
  const uint32_t* cv;               // [2 n][NP]
  const uint4* bits;                // [2 n] thermometer planes
  const unsigned long long* sig;    // [2 n]
  int NP;
  const anx_pair_score* pair;       // [n]
  const uint32_t *gid, *rank, *cnt, *src_sec, *src_row;
  const EvalSection* secs;
  const uint8_t* vflags;            // [V] ANX_VOCAB_* bits per vocabulary item
  uint32_t V;
  const uint4* sigtab;              // the lexicon's signature table and classes (DeviceLexicon::sig, cls_planes)
  const uint32_t* siglen_begin;
  const uint32_t* cls_planes;
  uint32_t cstride;
  int stop_exact;
  double score_threshold;
  uint4* out;                       // [n][2]
};

// dword w of the count vector (4 symbol slots, a byte each) of a string whose counts are all <= 4, from its thermometer planes (as encode.hip)
__device__ inline uint32_t ev_cv_word_of_planes(const uint4 pl, uint32_t w) {
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
__device__ inline uint32_t ev_cv_word(const EvalKArgs& k, uint32_t s, uint32_t kind, const uint4 pl, uint32_t w) {
  return kind ? ev_cv_word_of_planes(pl, w) : k.cv[(size_t)s * (size_t)k.NP + w];
}

__global__ __launch_bounds__(EV_BLOCK) void k_eval_classify(EvalKArgs k) {
  const uint32_t i = blockIdx.x * EV_BLOCK + threadIdx.x;
  if (i >= k.n) return;
  const anx_pair_score pr = k.pair[i];
  const uint32_t g = k.gid[i], rk = k.rank[i], cnt = k.cnt[i];
  const EvalSection sec = cnt ? k.secs[k.src_sec[i]] : EvalSection{};
  const uint32_t row0 = cnt ? k.src_row[i] : 0u;
  const uint32_t top = cnt ? sec.rec[row0].vocab_id : EV_NONE;
  const uint32_t ma = pr.status == ANX_OK ? k.meta[i] : 0u;
  const uint32_t kk = (ma >> 8) & 0xFFu, dd = (ma >> 16) & 0xFFu;
  double score = pr.score;
  uint32_t reason;
  if (rk != EV_NONE && rk < cnt) {
    reason = ANX_GOLD_RANKED;
    score = sec.rec[row0 + rk].dist_score;
  } else if (pr.status != ANX_OK) {
    reason = ANX_GOLD_STATUS;
  } else if (g == EV_NONE || g >= k.V || !(k.vflags[g] & ANX_VOCAB_INDEXED) || (k.vflags[g] & ANX_VOCAB_TRANSPARENT)) {
    reason = ANX_GOLD_NOT_A_RESULT;
  } else {
    // L1 of the two count vectors: NP x v_sad_u8 over the packed bytes, k_scan_sad's test
    const uint32_t ka = k.kind[i], kg = k.kind[k.n + i];
    const uint4 pa = k.bits[i], pg = k.bits[k.n + i];
    uint32_t l1 = 0;
    for (uint32_t w = 0; w < (uint32_t)k.NP; ++w) l1 = __builtin_amdgcn_sad_u8(ev_cv_word(k, i, ka, pa, w), ev_cv_word(k, k.n + i, kg, pg, w), l1);
    bool exact_stop = false;
    if (k.stop_exact && l1 != 0u) {  // the input's own anagram class: the run of its signature in its charcount range, then the count vectors
      const uint32_t len = ma & 0xFFu;
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
            for (uint32_t w = 0; w < (uint32_t)k.NP; ++w) eq = eq && k.cls_planes[(size_t)w * k.cstride + c] == ev_cv_word(k, i, ka, pa, w);
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
  const unsigned long long sb = (unsigned long long)__double_as_longlong(score);
  const uint32_t rank_word = reason == ANX_GOLD_RANKED ? rk : 0xFFFFFFFFu;  // int32 -1
  k.out[2 * (size_t)i] = make_uint4(g, rank_word, cnt, top);
  k.out[2 * (size_t)i + 1] = make_uint4((uint32_t)sb, (uint32_t)(sb >> 32), (uint32_t)pr.ld | kk << 16 | dd << 24,
                                        ((uint32_t)(int)pr.status & 0xFFu) | reason << 8);
}

void* eval_device_alloc(int device, size_t bytes) {
  void* p = nullptr;
  if (hipSetDevice(device) != hipSuccess || pool_malloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}
void eval_device_free(int device, void* p) {
  if (!p) return;
  (void)hipSetDevice(device);
  pool_free(p);
}

int evaluate_chunk(const HostModel& m, const DeviceLexicon* dl, LearnVocab** vocab, const PairSpan* a, const PairSpan* gold, size_t n, const anx_params& p,
                   const std::vector<LearnSection>& secs, const std::vector<size_t>& sec_rows, anx_gold_eval* out, anx_pair_score* pairs, std::string& err) {
  static_assert(sizeof(anx_gold_eval) == 2 * sizeof(uint4), "the record leaves as two 16-byte stores");
  if (n == 0) return ANX_OK;
  if (!dl) { err = "model is not resident on a device"; return ANX_ENODEVICE; }
  if (n > PAIRS_CHUNK) { err = "evaluate_chunk: more than 2^20 pairs"; return ANX_EINVAL; }
  if (secs.size() != sec_rows.size()) { err = "evaluate_chunk: sections and row counts differ"; return ANX_EINVAL; }
  for (size_t s = 0; s < secs.size(); ++s)
    if (sec_rows[s] >= 0x7FFFFFFFull || secs[s].n > n || (!secs[s].idx && secs[s].lo + secs[s].n > n)) { err = "evaluate_chunk: a section beyond the chunk"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(dl->device));
  // (host sources of the uploads below: declared before the scratch, whose destructor waits for the stream on every path)
  std::vector<EvalSection> hs(secs.size());
  std::vector<uint8_t> vflags(std::max<size_t>(m.decoder.size(), 1), 0);
  for (size_t v = 0; v < m.decoder.size(); ++v) vflags[v] = m.decoder[v].vocabtype;
  PairScratch sc(dl->device);
  hipStream_t st = sc.st;
  if (int rc = learn_vocab_ensure(m, dl->device, vocab, st, err)) return rc;
  const LearnVocab& t = **vocab;
  if (t.V != m.decoder.size()) { err = "evaluate_chunk: the vocabulary table is not this model's"; return ANX_EINVAL; }
  const uint32_t n32 = (uint32_t)n;
  PairsOnDevice pd;
  if (int rc = pairs_chunk_enqueue(m, dl, a, gold, n, &p, sc, pd, err)) return rc;
  uint32_t *d_gid = nullptr, *d_rank = nullptr, *d_cnt = nullptr, *d_sec = nullptr, *d_srow = nullptr;
  uint8_t* d_vflags = nullptr;
  EvalSection* d_secs = nullptr;
  uint4* d_out = nullptr;
  for (uint32_t** q : {&d_gid, &d_rank, &d_cnt, &d_sec, &d_srow})
    if (int rc = sc.get(q, n, err)) return rc;
  if (int rc = sc.get(&d_vflags, vflags.size(), err)) return rc;
  if (int rc = sc.get(&d_secs, secs.size(), err)) return rc;
  if (int rc = sc.get(&d_out, 2 * n, err)) return rc;
  char* h_out = static_cast<char*>(sc.pinned(n * sizeof(anx_gold_eval) + (pairs ? n * sizeof(anx_pair_score) : 0)));
  if (!h_out) { err = "out of host memory"; return ANX_EINVAL; }
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
      uint32_t* d_idx = nullptr;
      if (int rc = sc.get(&d_idx, L.n, err)) return rc;
      HIP_TRY(hipMemcpyAsync(d_idx, L.idx, L.n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      hs[s].idx = d_idx;
    }
  }
  if (!hs.empty()) HIP_TRY(hipMemcpyAsync(d_secs, hs.data(), hs.size() * sizeof(EvalSection), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_vflags, vflags.data(), vflags.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_cnt, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(d_sec, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(d_srow, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(d_rank, 0xFF, n * sizeof(uint32_t), st));
  for (size_t s = 0; s < hs.size(); ++s)
    if (hs[s].n) hipLaunchKernelGGL(k_eval_sections, dim3(grid_of(hs[s].n)), dim3(EV_BLOCK), 0, st, hs[s], (uint32_t)s, n32, d_cnt, d_sec, d_srow);
  {
    const int kt = ktimer_begin("k_eval_lookup", st);
    hipLaunchKernelGGL(k_eval_lookup, dim3(grid_of(n)), dim3(EV_BLOCK), 0, st, n32, pd.blob, pd.off, t.pool, t.voff, t.vh, t.slots, t.mask, t.hmask, d_gid);
    ktimer_end(kt, st);
  }
  {
    const int kt = ktimer_begin("k_eval_rows", st);
    for (size_t s = 0; s < hs.size(); ++s)
      if (hs[s].n && hs[s].rows) hipLaunchKernelGGL(k_eval_rows, dim3(grid_of(hs[s].rows)), dim3(EV_BLOCK), 0, st, hs[s], n32, d_gid, d_rank);
    ktimer_end(kt, st);
  }
  EvalKArgs k{};
  k.n = n32; k.off = pd.off; k.meta = pd.e.meta; k.kind = pd.e.kind; k.cv = pd.e.cv; k.bits = reinterpret_cast<const uint4*>(pd.e.bits); k.sig = pd.e.sig;
  k.NP = dl->nplanes; k.pair = pd.out;
  k.gid = d_gid; k.rank = d_rank; k.cnt = d_cnt; k.src_sec = d_sec; k.src_row = d_srow; k.secs = d_secs;
  k.vflags = d_vflags; k.V = (uint32_t)m.decoder.size();
  k.sigtab = dl->sig; k.siglen_begin = dl->alpha.siglen_begin; k.cls_planes = dl->cls_planes; k.cstride = dl->cstride;
  k.stop_exact = p.stop_at_exact_match ? 1 : 0;
  k.score_threshold = p.score_threshold;
  k.out = d_out;
  {
    const int kt = ktimer_begin("k_eval_classify", st);
    hipLaunchKernelGGL(k_eval_classify, dim3(grid_of(n)), dim3(EV_BLOCK), 0, st, k);
    ktimer_end(kt, st);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h_out, d_out, n * sizeof(anx_gold_eval), hipMemcpyDeviceToHost, st));
  if (pairs) HIP_TRY(hipMemcpyAsync(h_out + n * sizeof(anx_gold_eval), pd.out, n * sizeof(anx_pair_score), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  memcpy(out, h_out, n * sizeof(anx_gold_eval));
  if (pairs) memcpy(pairs, h_out + n * sizeof(anx_gold_eval), n * sizeof(anx_pair_score));
  return ANX_OK;
}

}  // namespace anx
