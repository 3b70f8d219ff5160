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
// The kernels' bodies, the reasons that need no rows and the record's stores are kernels_gold.hpp's, the section table and the flags
// gold_host.hpp's: sweep.hip and reweigh.hip answer the same question for many sets through the same definitions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.h"

namespace anx {

#include "kernels_common.hpp"
#include "kernels_gold.hpp"
#include "gold_host.hpp"

// (the bodies: kernels_gold.hpp; sweep.hip runs the same ones under its own names)
__global__ __launch_bounds__(GOLD_BLOCK) void k_eval_sections(GoldSection sec, uint32_t sid, uint32_t n, uint32_t* __restrict__ cnt,
                                                              uint32_t* __restrict__ src_sec, uint32_t* __restrict__ src_row) {
  gold_sections_body(sec, sid, n, cnt, src_sec, src_row);
}
__global__ __launch_bounds__(GOLD_BLOCK) void k_eval_lookup(uint32_t n, const uint8_t* __restrict__ blob, const uint32_t* __restrict__ off,
                                                            const uint8_t* __restrict__ pool, const uint32_t* __restrict__ voff,
                                                            const unsigned long long* __restrict__ vh, const uint32_t* __restrict__ slots, uint32_t mask,
                                                            unsigned long long hmask, uint32_t* __restrict__ gid) {
  gold_lookup_body(n, blob, off, pool, voff, vh, slots, mask, hmask, gid);
}
__global__ __launch_bounds__(GOLD_BLOCK) void k_eval_rows(GoldSection sec, uint32_t n, const uint32_t* __restrict__ gid, uint32_t* __restrict__ rank) {
  gold_rows_body(sec, n, gid, rank);
}

struct EvalKArgs {
  GoldPairSide side;                // meta: k_enc_strings ran with the caller's thresholds, symbols | k << 8 | d << 16 | ..
  const uint32_t* off;              // [2 n + 1] byte offsets of the chunk's strings
  const uint32_t *rank, *cnt, *src_sec, *src_row;
  const GoldSection* secs;
  double score_threshold;
  uint4* out;                       // [n][2]
};

__global__ __launch_bounds__(GOLD_BLOCK) void k_eval_classify(EvalKArgs k) {
  const uint32_t i = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  if (i >= k.side.n) return;
  const anx_pair_score pr = k.side.pair[i];
  const uint32_t g = k.side.gid[i], rk = k.rank[i], cnt = k.cnt[i];
  const GoldSection sec = cnt ? k.secs[k.src_sec[i]] : GoldSection{};
  const uint32_t row0 = cnt ? k.src_row[i] : 0u;
  const uint32_t top = cnt ? sec.rec[row0].vocab_id : GOLD_NONE;
  const uint32_t ma = pr.status == ANX_OK ? k.side.meta[i] : 0u;
  const uint32_t kk = (ma >> 8) & 0xFFu, dd = (ma >> 16) & 0xFFu;
  double score = pr.score;
  uint32_t reason;
  if (rk != GOLD_NONE && rk < cnt) {
    reason = ANX_GOLD_RANKED;
    score = sec.rec[row0 + rk].dist_score;
  } else {
    reason = gold_pre_reason(k.side, i, pr, kk, dd);
    if (reason == GOLD_LATER) reason = !(pr.score >= k.score_threshold) ? ANX_GOLD_THRESHOLD : ANX_GOLD_CROPPED;
  }
  gold_store_record(k.out, i, g, rk, cnt, top, score, pr.ld, kk, dd, pr.status, reason);
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
  HIP_TRY(hipSetDevice(dl->device));
  // (host sources of the uploads below: declared before the scratch, whose destructor waits for the stream on every path)
  std::vector<GoldSection> hs;
  std::vector<uint8_t> vflags;
  gold_vflags(m, vflags);
  PairScratch sc(dl->device);
  hipStream_t st = sc.st;
  GoldSection* d_secs = nullptr;
  if (int rc = gold_sections_upload("evaluate_chunk", secs, sec_rows, n, sc.blocks, st, hs, &d_secs, err)) return rc;
  if (int rc = learn_vocab_ensure(m, dl->device, vocab, st, err)) return rc;
  const LearnVocab& t = **vocab;
  if (t.V != m.decoder.size()) { err = "evaluate_chunk: the vocabulary table is not this model's"; return ANX_EINVAL; }
  const uint32_t n32 = (uint32_t)n;
  PairsOnDevice pd;
  if (int rc = pairs_chunk_enqueue(m, dl, a, gold, n, &p, sc, pd, err)) return rc;
  uint32_t *d_gid = nullptr, *d_rank = nullptr, *d_cnt = nullptr, *d_sec = nullptr, *d_srow = nullptr;
  uint8_t* d_vflags = nullptr;
  uint4* d_out = nullptr;
  for (uint32_t** q : {&d_gid, &d_rank, &d_cnt, &d_sec, &d_srow})
    if (int rc = sc.get(q, n, err)) return rc;
  if (int rc = sc.get(&d_vflags, vflags.size(), err)) return rc;
  if (int rc = sc.get(&d_out, 2 * n, err)) return rc;
  char* h_out = static_cast<char*>(sc.pinned(n * sizeof(anx_gold_eval) + (pairs ? n * sizeof(anx_pair_score) : 0)));
  if (!h_out) { err = "out of host memory"; return ANX_EINVAL; }
  HIP_TRY(hipMemcpyAsync(d_vflags, vflags.data(), vflags.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_cnt, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(d_sec, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(d_srow, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(d_rank, 0xFF, n * sizeof(uint32_t), st));
  for (size_t s = 0; s < hs.size(); ++s)
    if (hs[s].n) hipLaunchKernelGGL(k_eval_sections, dim3(gold_grid(hs[s].n)), dim3(GOLD_BLOCK), 0, st, hs[s], (uint32_t)s, n32, d_cnt, d_sec, d_srow);
  {
    const int kt = ktimer_begin("k_eval_lookup", st);
    hipLaunchKernelGGL(k_eval_lookup, dim3(gold_grid(n)), dim3(GOLD_BLOCK), 0, st, n32, pd.blob, pd.off, t.pool, t.voff, t.vh, t.slots, t.mask, t.hmask, d_gid);
    ktimer_end(kt, st);
  }
  {
    const int kt = ktimer_begin("k_eval_rows", st);
    for (size_t s = 0; s < hs.size(); ++s)
      if (hs[s].n && hs[s].rows) hipLaunchKernelGGL(k_eval_rows, dim3(gold_grid(hs[s].rows)), dim3(GOLD_BLOCK), 0, st, hs[s], n32, d_gid, d_rank);
    ktimer_end(kt, st);
  }
  EvalKArgs k{};
  GoldPairSide& d = k.side;
  d.n = n32; d.meta = pd.e.meta; d.kind = pd.e.kind; d.cv = pd.e.cv; d.bits = reinterpret_cast<const uint4*>(pd.e.bits); d.sig = pd.e.sig;
  d.NP = dl->nplanes; d.pair = pd.out; d.gid = d_gid; d.vflags = d_vflags; d.V = (uint32_t)m.decoder.size();
  d.sigtab = dl->sig; d.siglen_begin = dl->alpha.siglen_begin; d.cls_planes = dl->cls_planes; d.cstride = dl->cstride;
  d.stop_exact = p.stop_at_exact_match ? 1 : 0;
  k.off = pd.off;
  k.rank = d_rank; k.cnt = d_cnt; k.src_sec = d_sec; k.src_row = d_srow; k.secs = d_secs;
  k.score_threshold = p.score_threshold;
  k.out = d_out;
  {
    const int kt = ktimer_begin("k_eval_classify", st);
    hipLaunchKernelGGL(k_eval_classify, dim3(gold_grid(n)), dim3(GOLD_BLOCK), 0, st, k);
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
