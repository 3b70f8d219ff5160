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
//                       symbol count (dev_clamp_threshold, the encoder's), stored only when the caller asked for records; then the
//                       reduction: the block collects the 78 counters of anx_gold_summary in LDS (76 32-bit cells, two 64-bit
//                       cells for rr_fixed and n_results: 320 bytes), the waves add ballot counts and shuffle sums, and after the
//                       barrier one 64-bit integer atomicAdd per non-zero counter goes to the set's summary in HBM.  Integers only: the
//                       result does not depend on the order in which the blocks arrive.
//   and a download of 624 bytes per set (+ 32 n when the records are asked for).
// The sections, lookup and rows bodies, the reasons that need no rows, the record and the reduction are kernels_gold.hpp's, which
// eval.hip and reweigh.hip use too: one definition each.  The kernels keep their own names here, and eval.hip its launches and bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "sweep.h"

namespace anx {

#include "kernels_common.hpp"
#include "kernels_gold.hpp"
#include "gold_host.hpp"

namespace {
std::atomic<uint64_t> g_stats[SWEEP_NSTATS];
}  // namespace

void sweep_stats_add(int which, uint64_t v) {
  if (which >= 0 && which < SWEEP_NSTATS) g_stats[which].fetch_add(v, std::memory_order_relaxed);
}
void sweep_stats(uint64_t out[SWEEP_NSTATS]) {
  for (int i = 0; i < SWEEP_NSTATS; ++i) out[i] = g_stats[i].load(std::memory_order_relaxed);
}

// (the bodies: kernels_gold.hpp; eval.hip runs the same ones under its own names)
__global__ __launch_bounds__(GOLD_BLOCK) void k_sweep_sections(GoldSection sec, uint32_t sid, uint32_t n, uint32_t* __restrict__ cnt,
                                                               uint32_t* __restrict__ src_sec, uint32_t* __restrict__ src_row) {
  gold_sections_body(sec, sid, n, cnt, src_sec, src_row);
}
__global__ __launch_bounds__(GOLD_BLOCK) void k_sweep_lookup(uint32_t n, const uint8_t* __restrict__ blob, const uint32_t* __restrict__ off,
                                                             const uint8_t* __restrict__ pool, const uint32_t* __restrict__ voff,
                                                             const unsigned long long* __restrict__ vh, const uint32_t* __restrict__ slots, uint32_t mask,
                                                             unsigned long long hmask, uint32_t* __restrict__ gid) {
  gold_lookup_body(n, blob, off, pool, voff, vh, slots, mask, hmask, gid);
}
__global__ __launch_bounds__(GOLD_BLOCK) void k_sweep_rows(GoldSection sec, uint32_t n, const uint32_t* __restrict__ gid, uint32_t* __restrict__ rank) {
  gold_rows_body(sec, n, gid, rank);
}

struct SweepKArgs {
  GoldPairSide side;                // meta: k_enc_strings ran without thresholds (its k / d bits are not used)
  const uint32_t *rank, *cnt, *src_sec, *src_row;
  const GoldSection* secs;
  anx_threshold kth, dth;           // the set's max_anagram_distance / max_edit_distance
  double score_threshold;
  uint8_t* at1_base;                // [n] gold at rank 0 under sets[0]
  int baseline;                     // this pass is sets[0]'s: it writes at1_base
  unsigned long long* summary;      // [GOLD_COUNTERS] the set's anx_gold_summary on the device
  uint4* out;                       // [n][2] the records, or nullptr
};

__global__ __launch_bounds__(GOLD_BLOCK) void k_sweep_classify(SweepKArgs k) {
  __shared__ GoldCells s_cells;
  gold_summary_begin(s_cells);
  const uint32_t i = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  const bool live = i < k.side.n;
  uint32_t reason = 8u, g = GOLD_NONE, rk = GOLD_NONE, cnt = 0u;  // (reason 8: a lane behind the last pair counts nowhere)
  if (live) {
    const anx_pair_score pr = k.side.pair[i];
    g = k.side.gid[i]; rk = k.rank[i]; cnt = k.cnt[i];
    const GoldSection sec = cnt ? k.secs[k.src_sec[i]] : GoldSection{};
    const uint32_t row0 = cnt ? k.src_row[i] : 0u;
    const uint32_t top = cnt ? sec.rec[row0].vocab_id : GOLD_NONE;
    const uint32_t ma = pr.status == ANX_OK ? k.side.meta[i] : 0u;
    const uint32_t len = ma & 0xFFu;
    const uint32_t kk = ma ? (uint32_t)dev_clamp_threshold(k.kth, (int)len, kMaxAnagramDistance) : 0u;
    const uint32_t dd = ma ? (uint32_t)dev_clamp_threshold(k.dth, (int)len, kMaxEditDistance) : 0u;
    double score = pr.score;
    if (rk != GOLD_NONE && rk < cnt) {
      reason = ANX_GOLD_RANKED;
      score = sec.rec[row0 + rk].dist_score;
    } else {
      reason = gold_pre_reason(k.side, i, pr, kk, dd);
      if (reason == GOLD_LATER) reason = !(pr.score >= k.score_threshold) ? ANX_GOLD_THRESHOLD : ANX_GOLD_CROPPED;
    }
    if (k.out) gold_store_record(k.out, i, g, rk, cnt, top, score, pr.ld, kk, dd, pr.status, reason);
  }
  gold_summary_end(s_cells, live, i, reason, g, rk, cnt, k.at1_base, k.baseline, k.summary);
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
  gold_vflags(m, c->vflags);
  hipStream_t st = c->sc.st;
  if (int rc = learn_vocab_ensure(m, dl->device, vocab, st, err)) return rc;
  const LearnVocab& t = **vocab;
  if (t.V != m.decoder.size()) { err = "sweep_chunk_begin: the vocabulary table is not this model's"; return ANX_EINVAL; }
  if (int rc = pairs_chunk_enqueue(m, dl, a, gold, n, nullptr, c->sc, c->pd, err)) return rc;
  sweep_stats_add(SWEEP_PAIR_PASSES, 1);
  int rc;
  if ((rc = c->sc.get(&c->d_gid, n, err)) || (rc = c->sc.get(&c->d_per_set, 4 * n, err)) || (rc = c->sc.get(&c->d_vflags, c->vflags.size(), err)) ||
      (rc = c->sc.get(&c->d_at1, n, err)) || (rc = c->sc.get(&c->d_sum, GOLD_COUNTERS, err)) || (want_records && (rc = c->sc.get(&c->d_out, 2 * n, err))))
    return rc;
  c->h_down = static_cast<char*>(c->sc.pinned(sizeof(anx_gold_summary) + (want_records ? n * sizeof(anx_gold_eval) : 0)));
  if (!c->h_down) { err = "out of host memory"; return ANX_EINVAL; }
  HIP_TRY(hipMemcpyAsync(c->d_vflags, c->vflags.data(), c->vflags.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(c->d_at1, 0, n, st));
  {
    const int kt = ktimer_begin("k_sweep_lookup", st);
    hipLaunchKernelGGL(k_sweep_lookup, dim3(gold_grid(n)), dim3(GOLD_BLOCK), 0, st, (uint32_t)n, c->pd.blob, c->pd.off, t.pool, t.voff, t.vh, t.slots, t.mask, t.hmask,
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
  const size_t n = c->n;
  if (out && !c->d_out) { err = "sweep_chunk_set: the chunk keeps no record buffer"; return ANX_EINVAL; }
  const DeviceLexicon* dl = c->dl;
  HIP_TRY(hipSetDevice(dl->device));  // (the batch runs in between may have left another replica's device current)
  hipStream_t st = c->sc.st;
  const uint32_t n32 = (uint32_t)n;
  // the set's own blocks: the section table and the index lists; back to the pool when the set is done (a sweep has up to 256 sets)
  std::vector<GoldSection> hs;
  PoolBlocks mine;
  struct Release { PoolBlocks& b; hipStream_t st; ~Release() { (void)hipStreamSynchronize(st); b.release(); } } release{mine, st};
  GoldSection* d_secs = nullptr;
  if (int rc = gold_sections_upload("sweep_chunk_set", secs, sec_rows, n, mine, st, hs, &d_secs, err)) return rc;
  uint32_t *d_cnt = c->d_per_set, *d_sec = d_cnt + n, *d_srow = d_sec + n, *d_rank = d_srow + n;
  HIP_TRY(hipMemsetAsync(d_cnt, 0, 3 * n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(d_rank, 0xFF, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(c->d_sum, 0, sizeof(anx_gold_summary), st));
  for (size_t s = 0; s < hs.size(); ++s)
    if (hs[s].n) hipLaunchKernelGGL(k_sweep_sections, dim3(gold_grid(hs[s].n)), dim3(GOLD_BLOCK), 0, st, hs[s], (uint32_t)s, n32, d_cnt, d_sec, d_srow);
  {
    const int kt = ktimer_begin("k_sweep_rows", st);
    for (size_t s = 0; s < hs.size(); ++s)
      if (hs[s].n && hs[s].rows) hipLaunchKernelGGL(k_sweep_rows, dim3(gold_grid(hs[s].rows)), dim3(GOLD_BLOCK), 0, st, hs[s], n32, c->d_gid, d_rank);
    ktimer_end(kt, st);
  }
  const PairsOnDevice& pd = c->pd;
  SweepKArgs k{};
  GoldPairSide& d = k.side;
  d.n = n32; d.meta = pd.e.meta; d.kind = pd.e.kind; d.cv = pd.e.cv; d.bits = reinterpret_cast<const uint4*>(pd.e.bits); d.sig = pd.e.sig;
  d.NP = dl->nplanes; d.pair = pd.out; d.gid = c->d_gid; d.vflags = c->d_vflags; d.V = (uint32_t)c->m->decoder.size();
  d.sigtab = dl->sig; d.siglen_begin = dl->alpha.siglen_begin; d.cls_planes = dl->cls_planes; d.cstride = dl->cstride;
  d.stop_exact = p.stop_at_exact_match ? 1 : 0;
  k.rank = d_rank; k.cnt = d_cnt; k.src_sec = d_sec; k.src_row = d_srow; k.secs = d_secs;
  k.kth = p.max_anagram_distance; k.dth = p.max_edit_distance;
  k.score_threshold = p.score_threshold;
  k.at1_base = c->d_at1; k.baseline = baseline ? 1 : 0;
  k.summary = c->d_sum;
  k.out = out ? c->d_out : nullptr;
  {
    const int kt = ktimer_begin("k_sweep_classify", st);
    hipLaunchKernelGGL(k_sweep_classify, dim3(gold_grid(n)), dim3(GOLD_BLOCK), 0, st, k);
    ktimer_end(kt, st);
  }
  HIP_TRY(hipGetLastError());
  size_t bytes = 0;
  if (int rc = gold_set_download(c->h_down, c->d_sum, c->d_out, n, st, sum, out, &bytes, err)) return rc;
  sweep_stats_add(SWEEP_BYTES_DOWN, bytes);
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
  *v = SweepChunkView{c->m, c->dl, c->n, c->sc.st, c->pd.e.meta, c->pd.e.kind, c->pd.e.cv, c->pd.e.bits, c->pd.e.sig, c->pd.out, c->d_gid, c->d_vflags, c->d_at1, c->pd.blob, c->pd.off};
}

void sweep_chunk_end(SweepChunk* c) {
  if (!c) return;
  (void)hipSetDevice(c->dl->device);  // (the scratch returns its blocks to the current device's pool)
  delete c;
}

}  // namespace anx
