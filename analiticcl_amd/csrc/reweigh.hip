// reweigh.hip -- anx_evaluate_sweep_weights: score weights (and max_matches / score_threshold / cutoff_threshold / freq_weight) swept over
// gold pairs WITHOUT a batch run per set (gfx950 / CDNA4).
//
// The candidate set of an input is fixed by k, d and StopAtExactMatch; the five measures of every candidate are integers; max_freq is
// taken over every instance before the score threshold (src/lib.rs:1454-1462).  The weights enter at src/lib.rs:1443-1452 and in what
// follows: the score threshold, the sort, the crop, the cutoff.  So one base run per (k, d, stop) -- the batch path with max_matches 0,
// no cutoff, no frequency weight and a score threshold nothing falls below -- yields every instance with ld <= d, and explain's kernels
// (kernels_explain.hpp) their measures.  From there, on the chunk's device:
//   once per group (reweigh_group_begin):
//     k_rw_base     : flat over a section's rows, the lanes on consecutive 16-byte records: the row's pair by the binary search
//                     k_eval_rows runs (gold_section_slot, kernels_gold.hpp), vocab_id -> entry (DeviceLexicon::vocab_ent) -> {entry order, absolute frequency}; keeps 16 bytes of
//                     {pair, order, frequency, vocabulary id} and 8 bytes of packed measures per row, and the pair's largest frequency
//                     with one atomicMax per run of equal pairs in a wave
//     k_rw_pre      : a lane per pair: the reasons that do not depend on the weights (STATUS .. EDIT: gold_pre_reason, the function
//                     k_eval_classify and k_sweep_classify call) and the clamped k / d, one word
//   once per set (reweigh_group_set):
//     k_rw_score    : flat over the rows: the f64 score under the set's weights (score_finish restated term by term, as
//                     kernels_explain.hpp xm_score: same association, w_sum in launch_plan.hpp's order, the w_sum == 1.0 shortcut,
//                     DeviceLexicon::quot for x, L <= 32; -ffp-contract=off), the threshold test, kept rows counted per pair with one
//                     atomic per run of equal pairs in a wave
//     the exclusive scan of kernels_prefix.hpp over the counts (engine.hip prefix_scan_enqueue)
//     k_rw_fill     : the kept rows as SurvRow {score, order << 20, vocabulary id, frequency, no via} at soff[pair] + cursor
//     k_rank        : engine.hip's own kernel through launch_rank (rank_rows_enqueue): sort, crop, tie rule and cutoff are NOT restated
//     k_rw_classify : a lane per pair: rank of gold, n_results and the top row from the pair's ranked rows, THRESHOLD from the direct
//                     pair's score under the set's weights, the record when asked for (gold_store_record), then the reduction
//                     k_sweep_classify runs (gold_summary_begin / _end: LDS counters, one 64-bit integer atomic per non-zero
//                     counter and block; no float atomics)
//   and one download of 624 bytes per set (+ 32 n with the records).  No host round trip between a set's first launch and its download.
// Every append is bounds-checked against the scan's own offsets and the row buffer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "reweigh.h"

namespace anx {

#include "kernels_common.hpp"
#include "kernels_gold.hpp"
#include "gold_host.hpp"
#include "reweigh_shared.hpp"

namespace {
std::atomic<uint64_t> g_stats[RW_NSTATS];
}  // namespace

void reweigh_stats_add(int which, uint64_t v) {
  if (which >= 0 && which < RW_NSTATS) g_stats[which].fetch_add(v, std::memory_order_relaxed);
}
void reweigh_stats(uint64_t out[RW_NSTATS]) {
  for (int i = 0; i < RW_NSTATS; ++i) out[i] = g_stats[i].load(std::memory_order_relaxed);
}

// one compact export section of the base run with the measures of its rows
struct RwSection : GoldSection { const uint4* meas; };

struct RwBaseArgs {
  RwSection sec;
  uint32_t row0;                 // where the section's rows start in the group's arrays
  uint32_t n, R;                 // pairs of the chunk; rows of the group
  const uint32_t* vocab_ent;     // [V] vocabulary id -> entry
  uint32_t V, nentries;
  const EntRec* ent_rec;
  int have_freq;
  uint4* info;                   // [R] {pair, entry order, frequency (1 without have_freq), vocabulary id}; pair 0xFFFFFFFF: no row
  uint2* meas;                   // [R] {ld | lcs << 8 | prefix << 16 | suffix << 24, len_input | samecase << 8}
  uint32_t* maxf;                // [n] largest frequency of the pair's rows
};
__global__ __launch_bounds__(GOLD_BLOCK) void k_rw_base(RwBaseArgs k) {
  const uint32_t r = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  const RwSection& sec = k.sec;
  uint32_t pair = GOLD_NONE, freq = 0u;
  const bool inside = r < sec.rows && sec.n != 0u && k.row0 + r < k.R;
  if (inside) {
    const uint32_t lo = gold_section_slot(sec, r);
    const uint32_t i = sec.idx ? sec.idx[lo] : sec.lo + lo;
    const uint32_t vocab = sec.rec[r].vocab_id;
    uint32_t e = vocab < k.V ? k.vocab_ent[vocab] : GOLD_NONE;
    uint4 inf = make_uint4(GOLD_NONE, 0u, 0u, vocab);
    uint2 mm = make_uint2(0u, 0u);
    if (sec.off[lo] <= r && r < sec.off[lo + 1u] && i < k.n && e < k.nentries) {  // (a ranked row always has an entry)
      const EntRec er = k.ent_rec[e];
      const uint4 m = sec.meas[r];  // anx_row_measures: {score lo, score hi, ld | lcs | prefix | suffix, len_input | len_entry | anagram | flags}
      pair = i;
      freq = k.have_freq ? er.freq : 1u;
      inf = make_uint4(i, er.order, freq, vocab);
      mm = make_uint2(m.z, (m.w & 0xFFu) | ((m.w >> 24) & 1u) << 8);
    }
    k.info[k.row0 + r] = inf;
    k.meas[k.row0 + r] = mm;
  }
  // the pair's largest frequency: an inclusive segmented max over the run, one atomic by the run's last lane
  const uint32_t lane = threadIdx.x & 63u;
  const RwRun run = rw_run(pair);
  uint32_t mf = freq;
#pragma unroll
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)mf, o);
    if (lane >= run.start + o) mf = max(mf, u);
  }
  if (lane == run.end && pair != GOLD_NONE && mf) atomicMax(&k.maxf[pair], mf);
}

struct RwSetArgs {
  uint32_t n, R;
  const uint4* info;
  const uint2* meas;
  RwWeights w;
  double score_threshold;
  double* score;                 // [R]
  uint32_t* cnt;                 // [n] kept rows per pair
  const uint32_t* soff;          // [n + 1] exclusive scan of cnt
  uint32_t* cur;                 // [n] starts as soff[0 .. n)
  uint4* c_rows;                 // [row_cap] SurvRow as two 16-byte words
  uint32_t row_cap;
};
__global__ __launch_bounds__(GOLD_BLOCK) void k_rw_score(RwSetArgs k) {
  const uint32_t r = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  uint32_t pair = GOLD_NONE;
  bool keep = false;
  if (r < k.R) {
    pair = k.info[r].x;
    double s = 0.0;
    if (pair < k.n) {
      const uint2 m = k.meas[r];
      s = rw_score(k.w, m.y & 0xFFu, m.x & 0xFFu, (m.x >> 8) & 0xFFu, (m.x >> 16) & 0xFFu, m.x >> 24, (m.y >> 8) & 1u);
      keep = s >= k.score_threshold;  // src/lib.rs:1475
    } else pair = GOLD_NONE;
    k.score[r] = s;
  }
  const RwRun run = rw_run(pair);
  const uint32_t c = (uint32_t)__popcll(__ballot(keep) & run.lanes);
  if ((threadIdx.x & 63u) == run.end && pair != GOLD_NONE && c) atomicAdd(&k.cnt[pair], c);
}
__global__ __launch_bounds__(GOLD_BLOCK) void k_rw_fill(RwSetArgs k) {
  const uint32_t r = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint4 inf = make_uint4(GOLD_NONE, 0u, 0u, 0u);
  double s = 0.0;
  bool keep = false;
  if (r < k.R) {
    inf = k.info[r];
    if (inf.x < k.n) {
      s = k.score[r];
      keep = s >= k.score_threshold;  // (the test k_rw_score counted with, on the value it stored)
    } else inf.x = GOLD_NONE;
  }
  const RwRun run = rw_run(inf.x);
  const unsigned long long km = __ballot(keep) & run.lanes;
  uint32_t base = 0;
  if (lane == run.start && km) base = atomicAdd(&k.cur[inf.x], (uint32_t)__popcll(km));
  base = (uint32_t)__shfl((int)base, (int)run.start);
  if (!keep) return;
  const uint32_t pos = base + (uint32_t)__popcll(km & ((1ull << lane) - 1ull));
  if (pos >= k.soff[inf.x + 1u] || pos >= k.row_cap) return;  // (cannot happen: the offsets are the scan of these very counts)
  const unsigned long long sb = (unsigned long long)__double_as_longlong(s), ord = (unsigned long long)inf.y << 20;
  k.c_rows[2 * (size_t)pos] = make_uint4((uint32_t)sb, (uint32_t)(sb >> 32), (uint32_t)ord, (uint32_t)(ord >> 32));
  k.c_rows[2 * (size_t)pos + 1] = make_uint4(inf.w, inf.z, GOLD_NONE, 0u);  // {vocab, freq, no via, pad}
}

// ---- the direct pairs: the reasons that do not depend on the weights ----------------------------------------------------------------------
struct RwPreArgs {
  GoldPairSide side;             // meta: k_enc_strings ran without thresholds
  anx_threshold kth, dth;
  uint32_t* pre;                 // [n] reason (GOLD_LATER: none of them; THRESHOLD or CROPPED, per set) | k << 8 | d << 16
};
__global__ __launch_bounds__(GOLD_BLOCK) void k_rw_pre(RwPreArgs k) {
  const uint32_t i = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  if (i >= k.side.n) return;
  const anx_pair_score pr = k.side.pair[i];
  const uint32_t ma = pr.status == ANX_OK ? k.side.meta[i] : 0u;
  const uint32_t len = ma & 0xFFu;
  const uint32_t kk = ma ? (uint32_t)dev_clamp_threshold(k.kth, (int)len, kMaxAnagramDistance) : 0u;
  const uint32_t dd = ma ? (uint32_t)dev_clamp_threshold(k.dth, (int)len, kMaxEditDistance) : 0u;
  k.pre[i] = gold_pre_reason(k.side, i, pr, kk, dd) | kk << 8 | dd << 16;
}

// ---- per set: the record and the reduction ------------------------------------------------------------------------------------------------
struct RwClassArgs {
  uint32_t n, row_cap;
  const anx_pair_score* pair;
  const uint32_t *gid, *pre, *soff, *r_count;
  const DevRow* r_rows;
  RwWeights w;
  double score_threshold;
  uint8_t* at1_base;             // [n] gold at rank 0 under set 0
  int baseline;
  unsigned long long* summary;   // [GOLD_COUNTERS]
  uint4* out;                    // [n][2] the records, or nullptr
};
__global__ __launch_bounds__(GOLD_BLOCK) void k_rw_classify(RwClassArgs k) {
  __shared__ GoldCells s_cells;
  gold_summary_begin(s_cells);
  const uint32_t i = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  const bool live = i < k.n;
  uint32_t reason = 8u, g = GOLD_NONE, rk = GOLD_NONE, cnt = 0u;  // (reason 8: a lane behind the last pair counts nowhere)
  if (live) {
    const anx_pair_score pr = k.pair[i];
    g = k.gid[i];
    const uint32_t row0 = k.soff[i], room = min(k.soff[i + 1u], k.row_cap) - min(row0, k.row_cap);
    cnt = min(k.r_count[i], room);  // (k_rank never writes more rows than the pair has kept)
    const DevRow* rows = k.r_rows + row0;
    const uint32_t top = cnt ? rows[0].vocab_id : GOLD_NONE;
    if (g != GOLD_NONE)
      for (uint32_t j = 0; j < cnt; ++j)
        if (rows[j].vocab_id == g) { rk = j; break; }
    const uint32_t pw = k.pre[i];
    // the direct pair's score under the set's weights, from the measures the pair kernels left (0 for a pair with a status)
    double score = pr.status == ANX_OK ? rw_score(k.w, pr.len_a, pr.ld, pr.lcs, pr.prefixlen, pr.suffixlen, pr.samecase) : 0.0;
    if (rk != GOLD_NONE) {
      reason = ANX_GOLD_RANKED;
      score = rows[rk].dist_score;
    } else if ((pw & 0xFFu) != GOLD_LATER) {
      reason = pw & 0xFFu;
    } else if (!(score >= k.score_threshold)) {
      reason = ANX_GOLD_THRESHOLD;
    } else {
      reason = ANX_GOLD_CROPPED;
    }
    if (k.out) gold_store_record(k.out, i, g, rk, cnt, top, score, pr.ld, (pw >> 8) & 0xFFu, (pw >> 16) & 0xFFu, pr.status, reason);
  }
  gold_summary_end(s_cells, live, i, reason, g, rk, cnt, k.at1_base, k.baseline, k.summary);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
size_t reweigh_group_rows(const RwGroup* g) { return g->R; }

void reweigh_group_end(RwGroup* g) {
  if (!g) return;
  (void)hipSetDevice(g->v.dl->device);
  (void)hipStreamSynchronize(reinterpret_cast<hipStream_t>(g->v.stream));  // nothing of the group may still use the blocks
  g->blocks.release();
  if (g->h_down) host_result_free(g->h_down);
  delete g;
}

int reweigh_group_begin(const SweepChunkView& v, const anx_params& group, const std::vector<LearnSection>& secs, const std::vector<size_t>& sec_rows,
                        const std::vector<const anx_row_measures*>& sec_meas, bool want_records, RwGroup** out, std::string& err) {
  static_assert(sizeof(SurvRow) == 2 * sizeof(uint4) && sizeof(anx_row_measures) == sizeof(uint4) && sizeof(anx_gold_eval) == 2 * sizeof(uint4), "record layouts");
  *out = nullptr;
  const size_t n = v.n;
  if (secs.size() != sec_rows.size() || secs.size() != sec_meas.size()) { err = "reweigh_group_begin: sections, row counts and measures differ"; return ANX_EINVAL; }
  size_t R = 0;
  for (size_t s = 0; s < secs.size(); ++s) {
    R += sec_rows[s];
    if (R >= 0x7FFFFFFFull) { err = "weight sweep: more than 2^31 base rows in a chunk"; return ANX_ELIMIT; }
  }
  const DeviceLexicon* dl = v.dl;
  HIP_TRY(hipSetDevice(dl->device));  // (the batch runs in between may have left another replica's device current)
  hipStream_t st = reinterpret_cast<hipStream_t>(v.stream);
  if (const int rc = replica_vocab_entries(*v.m, dl, st, err)) return rc;
  std::vector<GoldSection> hs;  // the sections as k_rw_base reads them: each goes into its launch by value
  RwGroup* g = new RwGroup;
  struct Guard { RwGroup* g; ~Guard() { if (g) reweigh_group_end(g); } } guard{g};
  g->v = v; g->n = n; g->R = R;
  const size_t Rc = std::max<size_t>(R, 1);
  int rc;
  if ((rc = g->get(&g->info, Rc, err)) || (rc = g->get(&g->meas, Rc, err)) || (rc = g->get(&g->score, Rc, err)) || (rc = g->get(&g->t_key, Rc, err)) ||
      (rc = g->get(&g->c_rows, Rc, err)) || (rc = g->get(&g->r_rows, Rc, err)) || (rc = g->get(&g->cnt, n, err)) || (rc = g->get(&g->soff, n + 1, err)) ||
      (rc = g->get(&g->cur, n, err)) || (rc = g->get(&g->maxf, n, err)) || (rc = g->get(&g->r_count, n, err)) || (rc = g->get(&g->pre, n, err)) ||
      (rc = g->get(&g->ovf, 4, err)) || (rc = g->get(&g->d_sum, GOLD_COUNTERS, err)) || (want_records && (rc = g->get(&g->d_out, 2 * n, err))))
    return rc;
  uint8_t* tmp = nullptr;
  if ((rc = g->get(&tmp, prefix_scan_tmp_bytes(n), err))) return rc;
  g->tmp = reinterpret_cast<uint32_t*>(tmp);
  if ((rc = gold_sections_upload("reweigh_group_begin", secs, sec_rows, n, g->blocks, st, hs, nullptr, err))) return rc;
  g->h_down = host_result_alloc(sizeof(anx_gold_summary) + (want_records ? n * sizeof(anx_gold_eval) : 0));
  if (!g->h_down) { err = "out of host memory"; return ANX_EINVAL; }
  HIP_TRY(hipMemsetAsync(g->maxf, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(g->ovf, 0, 4 * sizeof(uint32_t), st));
  const uint32_t n32 = (uint32_t)n;
  size_t row0 = 0;
  {
    const int kt = ktimer_begin("k_rw_base", st);
    for (size_t s = 0; s < secs.size(); ++s) {
      RwBaseArgs k{};
      k.sec = RwSection{hs[s], reinterpret_cast<const uint4*>(sec_meas[s])};
      k.row0 = (uint32_t)row0; k.n = n32; k.R = (uint32_t)R;
      k.vocab_ent = dl->vocab_ent; k.V = dl->vocab_ent_n; k.nentries = dl->nentries; k.ent_rec = dl->ent_rec; k.have_freq = v.m->have_freq ? 1 : 0;
      k.info = g->info; k.meas = g->meas; k.maxf = g->maxf;
      if (k.sec.n && k.sec.rows) hipLaunchKernelGGL(k_rw_base, dim3(gold_grid(k.sec.rows)), dim3(GOLD_BLOCK), 0, st, k);
      row0 += sec_rows[s];
    }
    ktimer_end(kt, st);
  }
  RwPreArgs p{};
  GoldPairSide& d = p.side;
  d.n = n32; d.meta = v.meta; d.kind = v.kind; d.cv = v.cv; d.bits = reinterpret_cast<const uint4*>(v.bits); d.sig = v.sig;
  d.NP = dl->nplanes; d.pair = v.pair; d.gid = v.gid; d.vflags = v.vflags; d.V = (uint32_t)v.m->decoder.size();
  d.sigtab = dl->sig; d.siglen_begin = dl->alpha.siglen_begin; d.cls_planes = dl->cls_planes; d.cstride = dl->cstride;
  d.stop_exact = group.stop_at_exact_match ? 1 : 0;
  p.kth = group.max_anagram_distance; p.dth = group.max_edit_distance;
  p.pre = g->pre;
  {
    const int kt = ktimer_begin("k_rw_pre", st);
    hipLaunchKernelGGL(k_rw_pre, dim3(gold_grid(n)), dim3(GOLD_BLOCK), 0, st, p);
    ktimer_end(kt, st);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));  // the sections and the host index lists may go when this returns
  guard.g = nullptr;
  *out = g;
  return ANX_OK;
}

// The end of a set, for reweigh_group_set and for the confusable sweep (csweep.hip): the pairs classified from the ranked rows in
// r_rows / r_count, THRESHOLD from the direct pair's score under w, the reduction, the download and its wait.  d_sum was cleared on the stream.
int reweigh_group_finish(RwGroup* g, const anx_params& p, const anx_weights& w, bool baseline, anx_gold_summary* sum, anx_gold_eval* out, size_t* bytes, std::string& err) {
  const SweepChunkView& v = g->v;
  const size_t n = g->n, R = g->R;
  hipStream_t st = reinterpret_cast<hipStream_t>(v.stream);
  RwClassArgs c{};
  c.n = (uint32_t)n; c.row_cap = (uint32_t)R; c.pair = v.pair; c.gid = v.gid; c.pre = g->pre; c.soff = g->soff; c.r_count = g->r_count; c.r_rows = g->r_rows;
  c.w = RwWeights{w.ld, w.lcs, w.prefix, w.suffix, w.casew, w.ld + w.lcs + w.prefix + w.suffix + w.casew, v.dl->quot};  // w_sum: src/types.rs:69-73, as launch_plan.hpp
  c.score_threshold = p.score_threshold; c.at1_base = v.at1; c.baseline = baseline ? 1 : 0; c.summary = g->d_sum; c.out = out ? g->d_out : nullptr;
  {
    const int kt = ktimer_begin("k_rw_classify", st);
    hipLaunchKernelGGL(k_rw_classify, dim3(gold_grid(n)), dim3(GOLD_BLOCK), 0, st, c);
    ktimer_end(kt, st);
  }
  HIP_TRY(hipGetLastError());
  return gold_set_download(static_cast<char*>(g->h_down), g->d_sum, g->d_out, n, st, sum, out, bytes, err);
}

int reweigh_group_set(RwGroup* g, const anx_params& p, const anx_weights& w, bool baseline, anx_gold_summary* sum, anx_gold_eval* out, std::string& err) {
  if (out && !g->d_out) { err = "reweigh_group_set: the group keeps no record buffer"; return ANX_EINVAL; }
  const SweepChunkView& v = g->v;
  const size_t n = g->n, R = g->R;
  HIP_TRY(hipSetDevice(v.dl->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(v.stream);
  HIP_TRY(hipMemsetAsync(g->cnt, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(g->r_count, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(g->d_sum, 0, sizeof(anx_gold_summary), st));
  RwSetArgs k{};
  k.n = (uint32_t)n; k.R = (uint32_t)R; k.info = g->info; k.meas = g->meas;
  k.w = RwWeights{w.ld, w.lcs, w.prefix, w.suffix, w.casew, w.ld + w.lcs + w.prefix + w.suffix + w.casew, v.dl->quot};  // w_sum: src/types.rs:69-73, as launch_plan.hpp
  k.score_threshold = p.score_threshold;
  k.score = g->score; k.cnt = g->cnt; k.soff = g->soff; k.cur = g->cur; k.c_rows = reinterpret_cast<uint4*>(g->c_rows); k.row_cap = (uint32_t)R;
  if (R) {
    const int kt = ktimer_begin("k_rw_score", st);
    hipLaunchKernelGGL(k_rw_score, dim3(gold_grid(R)), dim3(GOLD_BLOCK), 0, st, k);
    ktimer_end(kt, st);
  }
  if (prefix_scan_enqueue(g->cnt, (uint32_t)n, g->soff, g->tmp, st, g->cur)) { err = "weight sweep: the prefix sum could not be enqueued"; return ANX_ENODEVICE; }
  if (R) {
    const int kt = ktimer_begin("k_rw_fill", st);
    hipLaunchKernelGGL(k_rw_fill, dim3(gold_grid(R)), dim3(GOLD_BLOCK), 0, st, k);
    ktimer_end(kt, st);
  }
  {
    const int kt = ktimer_begin("k_rank (weight sweep)", st);
    rank_rows_enqueue(RankPlain{p.cutoff_threshold, p.max_matches, p.freq_weight, v.m->have_freq ? 1 : 0}, st, (uint32_t)n, g->soff, g->c_rows, g->maxf, g->t_key, g->r_rows,
                      g->r_count, (uint32_t)R, g->ovf);
    ktimer_end(kt, st);
  }
  size_t bytes = 0;
  if (int rc = reweigh_group_finish(g, p, w, baseline, sum, out, &bytes, err)) return rc;
  reweigh_stats_add(RW_BYTES_DOWN, bytes);
  reweigh_stats_add(RW_ROWS_RESCORED, R);
  return ANX_OK;
}

}  // namespace anx
