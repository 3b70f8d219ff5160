// kernels_gold.hpp -- why a gold answer was ranked or lost: the device side that anx_evaluate_gold (eval.hip), anx_evaluate_sweep
// (sweep.hip) and anx_evaluate_sweep_weights (reweigh.hip) share.  Device functions and plain structs only: every kernel stays in its
// file under its own name (k_eval_* / k_sweep_* / k_rw_*), so the names the tests, the tools and the kernel timer know do not move.
// Included inside namespace anx after engine_internal.h and kernels_common.hpp; gfx950 only.
#pragma once

constexpr uint32_t GOLD_NONE = 0xFFFFFFFFu;  // no such vocabulary item / no such row
constexpr int GOLD_BLOCK = 256;              // threads per block of every kernel built from these bodies
constexpr uint32_t GOLD_LATER = 0xFFu;       // gold_pre_reason: the pair passes every test that needs no rows (THRESHOLD or CROPPED, the caller's)

// one compact export section on the device: inputs (= pairs of the chunk) lo + j, or idx[j], j < n; rows off[j] .. off[j + 1] of rec
struct GoldSection { const anx_topk_record* rec; const uint32_t* off; const uint32_t* idx; uint32_t n, lo, rows; };

// the last j in [0, sec.n) with off[j] <= r (sec.n != 0): inputs without rows share their offset with the next one and are stepped over
__device__ __forceinline__ uint32_t gold_section_slot(const GoldSection& sec, uint32_t r) {
  uint32_t lo = 0, hi = sec.n - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (sec.off[mid] <= r) lo = mid;
    else hi = mid - 1u;
  }
  return lo;
}

// ---- the bodies of k_eval_sections / k_eval_lookup / k_eval_rows and their k_sweep_* twins ------------------------------------------------
// per input: row count, section, first record (one lane per input of a section)
__device__ __forceinline__ void gold_sections_body(const GoldSection& sec, uint32_t sid, uint32_t n, uint32_t* __restrict__ cnt, uint32_t* __restrict__ src_sec,
                                                   uint32_t* __restrict__ src_row) {
  const uint32_t j = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  if (j >= sec.n) return;
  const uint32_t i = sec.idx ? sec.idx[j] : sec.lo + j;
  if (i >= n) return;
  const uint32_t r0 = sec.off[j], r1 = sec.off[j + 1];
  if (r1 < r0 || r1 > sec.rows) return;  // (offsets that do not describe this section: the input keeps no rows)
  cnt[i] = r1 - r0;
  src_sec[i] = sid;
  src_row[i] = r0;
}
// one lane per gold string (string n + i of the chunk's blob): FNV-1a of its bytes, probe of learn mode's vocabulary table -> gold id or none
__device__ __forceinline__ void gold_lookup_body(uint32_t n, const uint8_t* __restrict__ blob, const uint32_t* __restrict__ off, const uint8_t* __restrict__ pool,
                                                 const uint32_t* __restrict__ voff, const unsigned long long* __restrict__ vh, const uint32_t* __restrict__ slots,
                                                 uint32_t mask, unsigned long long hmask, uint32_t* __restrict__ gid) {
  const uint32_t i = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint8_t* a = blob + off[n + i];
  const uint32_t la = off[n + i + 1u] - off[n + i] - 1u;  // (each string is followed by a NUL byte)
  const unsigned long long h = lf_hash(a, la, hmask);
  uint32_t found = GOLD_NONE;
  for (uint32_t s = (uint32_t)h & mask, step = 0; step <= mask; s = (s + 1) & mask, ++step) {
    const uint32_t v = slots[s];
    if (v == LF_EMPTY) break;
    if (vh[v] == h && lf_eq(a, la, pool + voff[v], voff[v + 1] - voff[v])) { found = v; break; }
  }
  gid[i] = found;
}
// flat over the gathered rows of a section: where the record's vocabulary id is its input's gold id, rank = row - off[input] by atomicMin
__device__ __forceinline__ void gold_rows_body(const GoldSection& sec, uint32_t n, const uint32_t* __restrict__ gid, uint32_t* __restrict__ rank) {
  const uint32_t r = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  if (r >= sec.rows || sec.n == 0u) return;
  const uint32_t vocab = sec.rec[r].vocab_id;
  const uint32_t j = gold_section_slot(sec, r);
  const uint32_t r0 = sec.off[j];
  if (r0 > r) return;
  const uint32_t i = sec.idx ? sec.idx[j] : sec.lo + j;
  if (i >= n) return;
  const uint32_t g = gid[i];
  if (g != GOLD_NONE && g == vocab) atomicMin(&rank[i], r - r0);
}

// ---- the reasons that need no ranked rows ---------------------------------------------------------------------------------------------------
// what the engine knows about the direct pairs (input i, gold i) of a chunk: the encoder's arrays over the 2 n strings (the gold of
// pair i is string n + i), the pair records, the gold ids, the vocabulary's type flags and the lexicon's anagram classes
struct GoldPairSide {
  uint32_t n;
  const uint32_t* meta;             // [2 n] k_enc_strings: symbols | ..; 0 = empty or more than 255 symbols
  const uint32_t* kind;             // [2 n] 0: the count vector is in cv; else it follows from the planes
  const uint32_t* cv;               // [2 n][NP]
  const uint4* bits;                // [2 n] thermometer planes
  const unsigned long long* sig;    // [2 n]
  int NP;
  const anx_pair_score* pair;       // [n]
  const uint32_t* gid;              // [n] gold id or GOLD_NONE
  const uint8_t* vflags;            // [V] ANX_VOCAB_* bits per vocabulary item
  uint32_t V;
  const uint4* sigtab;              // the lexicon's signature table and classes (DeviceLexicon::sig, cls_planes)
  const uint32_t* siglen_begin;
  const uint32_t* cls_planes;
  uint32_t cstride;
  int stop_exact;
};
// dword w of the count vector of string s
__device__ __forceinline__ uint32_t gold_cv_word(const GoldPairSide& k, uint32_t s, uint32_t kind, const uint4 pl, uint32_t w) {
  return kind ? cv_word_of_planes(pl, w) : k.cv[(size_t)s * (size_t)k.NP + w];
}
// The ladder STATUS -> NOT_A_RESULT -> EXACT_STOP -> ANAGRAM -> EDIT for pair i whose gold was not among its ranked rows, under the
// clamped thresholds kk / dd; GOLD_LATER when the pair passes all of them.  pr = k.pair[i].
__device__ __forceinline__ uint32_t gold_pre_reason(const GoldPairSide& k, uint32_t i, const anx_pair_score& pr, uint32_t kk, uint32_t dd) {
  if (pr.status != ANX_OK) return ANX_GOLD_STATUS;
  const uint32_t g = k.gid[i];
  if (g == GOLD_NONE || g >= k.V || !(k.vflags[g] & ANX_VOCAB_INDEXED) || (k.vflags[g] & ANX_VOCAB_TRANSPARENT)) return ANX_GOLD_NOT_A_RESULT;
  // L1 of the two count vectors: NP x v_sad_u8 over the packed bytes, k_scan_sad's test
  const uint32_t ka = k.kind[i], kg = k.kind[k.n + i];
  const uint4 pa = k.bits[i], pg = k.bits[k.n + i];
  uint32_t l1 = 0;
  for (uint32_t w = 0; w < (uint32_t)k.NP; ++w) l1 = __builtin_amdgcn_sad_u8(gold_cv_word(k, i, ka, pa, w), gold_cv_word(k, k.n + i, kg, pg, w), l1);
  bool exact_stop = false;
  if (k.stop_exact && l1 != 0u) {  // the input's own anagram class: the run of its signature in its charcount range, then the count vectors
    const uint32_t len = k.meta[i] & 0xFFu;
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
          for (uint32_t w = 0; w < (uint32_t)k.NP; ++w) eq = eq && k.cls_planes[(size_t)w * k.cstride + c] == gold_cv_word(k, i, ka, pa, w);
          exact_stop = eq;
        }
        break;
      }
    }
  }
  if (exact_stop) return ANX_GOLD_EXACT_STOP;
  if (l1 > kk || l1 >= (uint32_t)pr.len_a + (uint32_t)pr.len_b) return ANX_GOLD_ANAGRAM;
  if ((uint32_t)pr.ld > dd) return ANX_GOLD_EDIT;
  return GOLD_LATER;
}

// the 32-byte anx_gold_eval of pair i as two 16-byte stores
__device__ __forceinline__ void gold_store_record(uint4* __restrict__ out, uint32_t i, uint32_t g, uint32_t rk, uint32_t cnt, uint32_t top, double score, uint32_t ld,
                                                  uint32_t kk, uint32_t dd, int status, uint32_t reason) {
  const unsigned long long sb = (unsigned long long)__double_as_longlong(score);
  const uint32_t rank_word = reason == ANX_GOLD_RANKED ? rk : 0xFFFFFFFFu;  // int32 -1
  out[2 * (size_t)i] = make_uint4(g, rank_word, cnt, top);
  out[2 * (size_t)i + 1] = make_uint4((uint32_t)sb, (uint32_t)(sb >> 32), ld | kk << 16 | dd << 24, ((uint32_t)status & 0xFFu) | reason << 8);
}

// ---- the reduction to an anx_gold_summary ---------------------------------------------------------------------------------------------------
// The block collects the 78 counters in LDS (76 32-bit cells, two 64-bit cells for rr_fixed and n_results: 320 bytes), the waves add
// ballot counts and shuffle sums, and after the barrier one 64-bit integer atomicAdd per non-zero counter goes to the summary in HBM.
// Integers only: the result does not depend on the order in which the blocks arrive.
constexpr uint32_t GOLD_COUNTERS = sizeof(anx_gold_summary) / sizeof(uint64_t);  // 78, in the struct's order
constexpr uint32_t GOLD_CELLS32 = GOLD_COUNTERS - 2;                             // all but rr_fixed and n_results
// counter index = offset in anx_gold_summary / 8
constexpr uint32_t GOLD_N = 0, GOLD_KNOWN = 1, GOLD_REASON = 2, GOLD_HIST = 10, GOLD_RR = 74, GOLD_NRES = 75, GOLD_GAINED = 76, GOLD_LOST = 77;
static_assert(GOLD_COUNTERS == 78 && GOLD_HIST + ANX_GOLD_RANK_BINS == GOLD_RR, "the counters follow anx_gold_summary's layout");
struct GoldCells {
  unsigned long long wide[2];   // rr_fixed, n_results
  uint32_t cell[GOLD_CELLS32];  // the other counters in the struct's order, gained / lost behind the histogram
};
// floor(2^32 / (rank + 1)) in 32-bit arithmetic for rank >= 1: 2^32 = 0xFFFFFFFF + 1
__device__ __forceinline__ unsigned long long gold_rr_fixed(uint32_t rank) {
  if (rank == 0u) return 1ull << 32;
  const uint32_t d = rank + 1u, q = 0xFFFFFFFFu / d, r = 0xFFFFFFFFu - q * d;
  return (unsigned long long)(q + (r + 1u == d ? 1u : 0u));
}
__device__ __forceinline__ unsigned long long gold_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o);
  return v;
}
// Every thread of the block calls begin before it classifies its pair and end after it.  s: the block's cells in LDS.
__device__ __forceinline__ void gold_summary_begin(GoldCells& s) {
  for (uint32_t x = threadIdx.x; x < GOLD_CELLS32; x += GOLD_BLOCK) s.cell[x] = 0u;
  if (threadIdx.x < 2u) s.wide[threadIdx.x] = 0ull;
  __syncthreads();
}
// live: the thread has a pair, i; a thread behind the last pair passes reason 8, g and rk GOLD_NONE, cnt 0 and counts nowhere.
// at1_base: [n] gold at rank 0 under set 0, written by the baseline pass and compared with by the others (gained / lost).
__device__ __forceinline__ void gold_summary_end(GoldCells& s, bool live, uint32_t i, uint32_t reason, uint32_t g, uint32_t rk, uint32_t cnt, uint8_t* at1_base,
                                                 int baseline, unsigned long long* summary) {
  const bool ranked = reason == ANX_GOLD_RANKED;
  const bool at1 = ranked && rk == 0u;
  bool base1 = at1;
  if (live) {
    if (baseline) at1_base[i] = at1 ? 1 : 0;
    else base1 = at1_base[i] != 0;
  }
  const bool lane0 = (threadIdx.x & 63u) == 0u;
  const uint32_t c_live = (uint32_t)__popcll(__ballot(live)), c_known = (uint32_t)__popcll(__ballot(live && g != GOLD_NONE));
  const uint32_t c_at1 = (uint32_t)__popcll(__ballot(at1));
  const uint32_t c_gained = (uint32_t)__popcll(__ballot(at1 && !base1)), c_lost = (uint32_t)__popcll(__ballot(live && !at1 && base1));
  if (lane0) {
    if (c_live) atomicAdd(&s.cell[GOLD_N], c_live);
    if (c_known) atomicAdd(&s.cell[GOLD_KNOWN], c_known);
    if (c_at1) atomicAdd(&s.cell[GOLD_HIST], c_at1);
    if (c_gained) atomicAdd(&s.cell[GOLD_GAINED - 2u], c_gained);
    if (c_lost) atomicAdd(&s.cell[GOLD_LOST - 2u], c_lost);
  }
#pragma unroll
  for (uint32_t r = 0; r < 8u; ++r) {
    const uint32_t c = (uint32_t)__popcll(__ballot(reason == r));
    if (lane0 && c) atomicAdd(&s.cell[GOLD_REASON + r], c);
  }
  if (ranked && rk != 0u) atomicAdd(&s.cell[GOLD_HIST + min(rk, (uint32_t)ANX_GOLD_RANK_BINS - 1u)], 1u);
  const unsigned long long w_rr = gold_wave_sum(ranked ? gold_rr_fixed(rk) : 0ull), w_res = gold_wave_sum((unsigned long long)cnt);
  if (lane0) {
    if (w_rr) atomicAdd(&s.wide[0], w_rr);
    if (w_res) atomicAdd(&s.wide[1], w_res);
  }
  __syncthreads();
  if (threadIdx.x < GOLD_COUNTERS) {
    const uint32_t t = threadIdx.x;
    const unsigned long long v = t < GOLD_RR ? (unsigned long long)s.cell[t] : t <= GOLD_NRES ? s.wide[t - GOLD_RR] : (unsigned long long)s.cell[t - 2u];
    if (v) atomicAdd(&summary[t], v);
  }
}
