// fit.hip -- anx_fit_confusable_weights: the weights of candidate confusable patterns fitted by greedy coordinate ascent over gold
// pairs, every trial of a round in ONE launch per chunk (gfx950 / CDNA4).  Late mode only.
//
// In late mode the reference crops the ranked list first, then multiplies the list's weights into the rows that survived the crop,
// re-sorts those rows stably and applies the cutoff (src/lib.rs:1535-1622); csweep.hip does the same with k_rank without a cutoff and
// k_conf_apply_late.  So the cropped list of an input does not depend on the weights, every weight assignment is a re-rank of the same
// few rows, and only a pair whose gold is in its cropped list can be RANKED under any assignment.  Per chunk, behind the confusable
// sweep's base run, masks and unweighted late ranking (csweep_group_rank_late; k_conf_apply_late has NOT run):
//   k_fit_gold   : a lane per pair: the slot of the row whose vocabulary id is the pair's gold id among its cropped rows, or none; the
//                  pair's row count, 0 without a gold slot
//   the exclusive scan of those counts (prefix_scan_enqueue): where the pair's rows lie in the compact block
//   k_fit_state  : a lane per compact slot: its pair by a binary search over the offsets, the ranked row's {dist_score, freq_score} and
//                  the mask of its base row (found by its vocabulary id in the pair's range of base rows, as k_cs_slot_w finds it)
// after which the group, the base rows and the sections go: 24 bytes per slot and 12 per pair stay, for every chunk of the call.
// Per round and chunk:
//   k_fit_trials : a lane per pair (grid-stride).  U = the OR of the pair's masks.  The pair's result under the current weights once,
//                  then one result per (pattern j in U, grid weight g != cur[j]).  A result is what k_conf_apply_late plus
//                  k_rw_classify give: the row weight ((1.0 * w_a) * w_b) * .. over the mask's bits in ascending pattern order,
//                  dist_score *= weight only when weight != 1.0, the stable re-sort only when some weight != 1.0, and then gold's
//                  rank by COUNTING -- the rows before gold that gold is not strictly before, plus the rows behind gold that are
//                  strictly before it (conf_before, conf_rank.hpp; a stable insertion sort under a strict weak order puts gold
//                  there) -- and the cutoff against the list's first row, the row nothing is strictly before.  No per-lane array.
//                  The block keeps 64-bit LDS counters {at1, ranked, rr_fixed} of the current totals, of the current results of the
//                  pairs pattern j touches, and of the trial results of those pairs; after the barrier one 64-bit integer atomicAdd
//                  per non-zero cell goes to HBM (gold_summary_end's pattern).  Integers only: no order of arrival changes a result.
// The host forms total[j][g] = current - touched_current[j] + touched_trial[j][g]; one download of at most 26 KB per round.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "fit.h"

namespace anx {

#include "kernels_common.hpp"
#include "kernels_gold.hpp"
#include "gold_host.hpp"
#include "conf_rank.hpp"

namespace {
std::atomic<uint64_t> g_stats[FIT_NSTATS];
}  // namespace

void fit_stats_add(int which, uint64_t v) {
  if (which >= 0 && which < FIT_NSTATS) g_stats[which].fetch_add(v, std::memory_order_relaxed);
}
void fit_stats(uint64_t out[FIT_NSTATS]) {
  for (int i = 0; i < FIT_NSTATS; ++i) out[i] = g_stats[i].load(std::memory_order_relaxed);
}

constexpr uint32_t FIT_MAXP = 64, FIT_MAXG = ANX_FIT_MAX_GRID;
constexpr uint32_t FIT_NOPATTERN = 64;   // fit_weight's j: no pattern is replaced
constexpr uint32_t FIT_MAX_BLOCKS = 1024;  // k_fit_trials strides: fewer blocks, fewer atomics to HBM per cell

struct FitSlot { double dist, freq; unsigned long long mask; };  // one row of a cropped list, 24 bytes

// ---- per chunk: the state ---------------------------------------------------------------------------------------------------------------
struct FitStateArgs {
  uint32_t n, R;                   // pairs; the capacity of r_rows and the number of base rows
  const uint4* info;               // [R] {pair, ., ., vocabulary id}
  const unsigned long long* mask;  // [R]
  const uint32_t *rbeg, *rend, *soff, *r_count, *gid;
  const DevRow* r_rows;
  uint32_t *pcnt, *pgold;          // [n] rows of the pair in the state (0: gold is not in its cropped list); gold's slot
  const uint32_t* poff;            // [n + 1] exclusive scan of pcnt
  FitSlot* slots;                  // [total]
  uint32_t total;
  uint32_t* ctr;                   // [0] pairs with a gold slot
};
__global__ __launch_bounds__(GOLD_BLOCK) void k_fit_gold(FitStateArgs k) {
  const uint32_t i = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  bool found = false;
  if (i < k.n) {
    const uint32_t row0 = k.soff[i], room = min(k.soff[i + 1u], k.R) - min(row0, k.R);
    const uint32_t cnt = min(k.r_count[i], room), g = k.gid[i];  // (k_rw_classify's bound: k_rank never writes more rows than the pair has kept)
    uint32_t slot = GOLD_NONE;
    if (g != GOLD_NONE)
      for (uint32_t j = 0; j < cnt; ++j)
        if (k.r_rows[row0 + j].vocab_id == g) { slot = j; break; }
    found = slot != GOLD_NONE;
    k.pgold[i] = slot;
    k.pcnt[i] = found ? cnt : 0u;
  }
  const uint32_t c = (uint32_t)__popcll(__ballot(found));
  if ((threadIdx.x & 63u) == 0u && c) atomicAdd(&k.ctr[0], c);
}
__global__ __launch_bounds__(GOLD_BLOCK) void k_fit_state(FitStateArgs k) {
  const uint32_t x = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  if (x >= k.total) return;
  uint32_t lo = 0, hi = k.n;  // the last pair with poff[pair] <= x: the one whose rows hold slot x
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (k.poff[mid] <= x) lo = mid; else hi = mid;
  }
  FitSlot s{0.0, 0.0, 0ull};
  const uint32_t j = x - k.poff[lo], src = k.soff[lo] + j;
  if (j < k.pcnt[lo] && src < k.R) {
    const DevRow row = k.r_rows[src];
    s.dist = row.dist_score; s.freq = row.freq_score;
    const uint32_t e = min(k.rend[lo], k.R);
    for (uint32_t r = k.rbeg[lo]; r < e; ++r) {  // the base row of the ranked row: same pair, same vocabulary id (k_cs_slot_w)
      const uint4 inf = k.info[r];
      if (inf.x == lo && inf.w == row.vocab_id) { s.mask = k.mask[r]; break; }
    }
  }
  k.slots[x] = s;
}

// ---- per round: every trial of every pair -------------------------------------------------------------------------------------------------
struct FitTrialArgs {
  uint32_t n, total;
  const FitSlot* slots;
  const uint32_t *poff, *pcnt, *pgold;
  const double *cur, *grid;        // [np], [ng] on the device
  uint32_t np, ng;
  double cutoff_threshold;
  float freq_weight;
  unsigned long long* cells;       // [3 + 3 np + 3 np ng]: current totals | touched current [np][3] | touched trial [np][ng][3]
};
// cs_weight (csweep.hip) with pattern j's weight replaced by wj: ((1.0 * w_a) * w_b) * .., ascending pattern order
__device__ __forceinline__ double fit_weight(const double* s_w, unsigned long long mask, uint32_t j, double wj) {
  double w = 1.0;
  for (unsigned long long m = mask; m; m &= m - 1ull) {
    const uint32_t b = (uint32_t)__ffsll((long long)m) - 1u;
    w *= b == j ? wj : s_w[b];
  }
  return w;
}
// the row as k_conf_apply_late leaves it before the sort: dist_score *= weight only when weight != 1.0
__device__ __forceinline__ DevRow fit_row(const FitSlot& s, const double* s_w, uint32_t j, double wj, bool* any) {
  DevRow r{0u, 0u, s.dist, s.freq};
  const double w = fit_weight(s_w, s.mask, j, wj);
  if (w != 1.0) { r.dist_score *= w; *any = true; }
  return r;
}
// Is gold still in the list after the weights, the stable re-sort and the cutoff, and at which rank?  v: the pair's n cropped rows.
__device__ inline bool fit_eval(const FitSlot* __restrict__ v, uint32_t n, uint32_t gold, const double* s_w, uint32_t j, double wj, double cutoff, float fw, uint32_t* rank) {
  bool any = false, unused = false;
  DevRow best = fit_row(v[0], s_w, j, wj, &any);  // the list's first row after the sort: the earliest row nothing is strictly before
  uint32_t bi = 0;
  for (uint32_t i = 1; i < n; ++i) {
    const DevRow r = fit_row(v[i], s_w, j, wj, &any);
    if (conf_before(r, best, fw)) { best = r; bi = i; }
  }
  const bool cuts = cutoff >= 1.0;  // src/lib.rs:1597-1611
  if (!any) {  // no weight differs from 1.0: the list stays as k_rank left it
    *rank = gold;
    if (!cuts) return true;
    const double thr = conf_vr_score(fit_row(v[0], s_w, j, wj, &unused), fw) / cutoff;
    for (uint32_t i = 1; i <= gold; ++i)
      if (conf_vr_score(fit_row(v[i], s_w, j, wj, &unused), fw) <= thr) return false;
    return true;
  }
  const DevRow G = fit_row(v[gold], s_w, j, wj, &unused);
  const double thr = conf_vr_score(best, fw) / cutoff;
  uint32_t rk = 0;
  bool cut = gold != bi && conf_vr_score(G, fw) <= thr;
  for (uint32_t i = 0; i < n; ++i) {
    if (i == gold) continue;
    const DevRow r = fit_row(v[i], s_w, j, wj, &unused);
    const bool ahead = i < gold ? !conf_before(G, r, fw) : conf_before(r, G, fw);
    if (ahead) {
      ++rk;
      if (i != bi && conf_vr_score(r, fw) <= thr) cut = true;  // the list ends at the first row behind its head that the cutoff takes
    }
  }
  *rank = rk;
  return !cuts || !cut;
}
__device__ __forceinline__ void fit_count(unsigned long long* cell, bool kept, uint32_t rank) {
  if (!kept) return;
  if (rank == 0u) atomicAdd(&cell[0], 1ull);
  atomicAdd(&cell[1], 1ull);
  atomicAdd(&cell[2], gold_rr_fixed(rank));
}
__global__ __launch_bounds__(GOLD_BLOCK) void k_fit_trials(FitTrialArgs k) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fit_lds[];
  const uint32_t ncells = 3u + 3u * k.np + 3u * k.np * k.ng;
  unsigned long long* s_cells = reinterpret_cast<unsigned long long*>(fit_lds);
  double* s_cur = reinterpret_cast<double*>(s_cells + ncells);  // [FIT_MAXP]
  double* s_grid = s_cur + FIT_MAXP;                            // [FIT_MAXG]
  for (uint32_t x = threadIdx.x; x < ncells; x += GOLD_BLOCK) s_cells[x] = 0ull;
  if (threadIdx.x < FIT_MAXP) s_cur[threadIdx.x] = threadIdx.x < k.np ? k.cur[threadIdx.x] : 1.0;
  if (threadIdx.x < FIT_MAXG) s_grid[threadIdx.x] = threadIdx.x < k.ng ? k.grid[threadIdx.x] : 1.0;
  __syncthreads();
  const unsigned long long live = k.np >= 64u ? ~0ull : (1ull << k.np) - 1ull;
  unsigned long long t_at1 = 0ull, t_ranked = 0ull, t_rr = 0ull;  // this lane's share of the current totals
  for (uint32_t i = blockIdx.x * GOLD_BLOCK + threadIdx.x; i < k.n; i += gridDim.x * GOLD_BLOCK) {
    const uint32_t cnt = k.pcnt[i];
    if (cnt == 0u) continue;  // gold is not in the cropped list: no weight ranks it
    const uint32_t gold = k.pgold[i], off = k.poff[i];
    if (gold >= cnt || off > k.total || cnt > k.total - off) continue;  // (cannot happen: the offsets are the scan of these counts)
    const FitSlot* __restrict__ v = k.slots + off;
    unsigned long long U = 0ull;
    for (uint32_t r = 0; r < cnt; ++r) U |= v[r].mask;
    U &= live;
    uint32_t rk = 0;
    const bool kept = fit_eval(v, cnt, gold, s_cur, FIT_NOPATTERN, 1.0, k.cutoff_threshold, k.freq_weight, &rk);
    if (kept) {
      t_at1 += rk == 0u ? 1ull : 0ull;
      t_ranked += 1ull;
      t_rr += gold_rr_fixed(rk);
    }
    for (unsigned long long m = U; m; m &= m - 1ull) {
      const uint32_t j = (uint32_t)__ffsll((long long)m) - 1u;
      fit_count(s_cells + 3u + 3u * j, kept, rk);
      for (uint32_t g = 0; g < k.ng; ++g) {
        const double wj = s_grid[g];
        if (wj == s_cur[j]) continue;  // not a trial
        uint32_t trk = 0;
        const bool tkept = fit_eval(v, cnt, gold, s_cur, j, wj, k.cutoff_threshold, k.freq_weight, &trk);
        fit_count(s_cells + 3u + 3u * k.np + 3u * (j * k.ng + g), tkept, trk);
      }
    }
  }
  t_at1 = gold_wave_sum(t_at1); t_ranked = gold_wave_sum(t_ranked); t_rr = gold_wave_sum(t_rr);
  if ((threadIdx.x & 63u) == 0u) {
    if (t_at1) atomicAdd(&s_cells[0], t_at1);
    if (t_ranked) atomicAdd(&s_cells[1], t_ranked);
    if (t_rr) atomicAdd(&s_cells[2], t_rr);
  }
  __syncthreads();
  for (uint32_t x = threadIdx.x; x < ncells; x += GOLD_BLOCK) {
    const unsigned long long c = s_cells[x];
    if (c) atomicAdd(&k.cells[x], c);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
struct FitChunk {
  uint32_t n = 0, total = 0;
  FitSlot* slots = nullptr;
  uint32_t *poff = nullptr, *pcnt = nullptr, *pgold = nullptr;
};
struct FitCall {
  const DeviceLexicon* dl = nullptr;
  hipStream_t st = nullptr;
  PoolBlocks blocks;               // the grid, the current weights, the cells and every chunk's state
  std::vector<FitChunk> chunks;
  uint32_t np = 0, ng = 0, ncells = 0;
  double grid[FIT_MAXG] = {};
  double *d_grid = nullptr, *d_cur = nullptr;
  unsigned long long* d_cells = nullptr;
  char* h_pin = nullptr;           // pinned: the current weights going up [FIT_MAXP] | the cells coming down
};

void fit_call_end(FitCall* c) {
  if (!c) return;
  (void)hipSetDevice(c->dl->device);
  if (c->st) {
    (void)hipStreamSynchronize(c->st);  // nothing of the call may still use the blocks
    encoder_stream_release(c->dl->device, c->st);
  }
  c->blocks.release();
  if (c->h_pin) host_result_free(c->h_pin);
  delete c;
}

int fit_call_begin(const DeviceLexicon* dl, uint32_t n_patterns, const double* grid, uint32_t n_grid, FitCall** out, std::string& err) {
  *out = nullptr;
  if (!dl) { err = "model is not resident on a device"; return ANX_ENODEVICE; }
  if (n_patterns == 0 || n_patterns > FIT_MAXP || n_grid == 0 || n_grid > FIT_MAXG) { err = "confusable fit: 1 .. 64 patterns, 1 .. 16 grid weights"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(dl->device));
  FitCall* c = new FitCall;
  struct Guard { FitCall* c; ~Guard() { if (c) fit_call_end(c); } } guard{c};
  c->dl = dl; c->np = n_patterns; c->ng = n_grid; c->ncells = 3u + 3u * n_patterns + 3u * n_patterns * n_grid;
  memcpy(c->grid, grid, n_grid * sizeof(double));
  c->st = encoder_stream_acquire(dl->device);
  if (!c->st) { err = "confusable fit: no stream"; return ANX_ENODEVICE; }
  int rc;
  if ((rc = c->blocks.get(&c->d_grid, FIT_MAXG, err)) || (rc = c->blocks.get(&c->d_cur, FIT_MAXP, err)) || (rc = c->blocks.get(&c->d_cells, c->ncells, err))) return rc;
  c->h_pin = static_cast<char*>(host_result_alloc(FIT_MAXP * sizeof(double) + c->ncells * sizeof(unsigned long long)));
  if (!c->h_pin) { err = "out of host memory"; return ANX_EINVAL; }
  HIP_TRY(hipMemcpy(c->d_grid, c->grid, n_grid * sizeof(double), hipMemcpyHostToDevice));
  guard.c = nullptr;
  *out = c;
  return ANX_OK;
}

int fit_chunk_add(FitCall* c, const CsRankedView& v, std::string& err) {
  if (v.dl != c->dl) { err = "confusable fit: the chunk lies on another replica"; return ANX_EINVAL; }
  if (v.n == 0 || v.n > PAIRS_CHUNK || v.R >= 0x7FFFFFFFull) { err = "confusable fit: a chunk of 1 .. 2^20 pairs and fewer than 2^31 rows"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(c->dl->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(v.stream);  // the chunk's: behind its rank
  const size_t n = v.n;
  FitChunk ch;
  ch.n = (uint32_t)n;
  uint32_t* ctr = nullptr;
  int rc;
  if ((rc = c->blocks.get(&ch.poff, n + 1, err)) || (rc = c->blocks.get(&ch.pcnt, n, err)) || (rc = c->blocks.get(&ch.pgold, n, err)) || (rc = c->blocks.get(&ctr, 4, err))) return rc;
  HIP_TRY(hipMemsetAsync(ctr, 0, 4 * sizeof(uint32_t), st));
  FitStateArgs k{};
  k.n = ch.n; k.R = (uint32_t)v.R; k.info = static_cast<const uint4*>(v.info); k.mask = v.mask; k.rbeg = v.rbeg; k.rend = v.rend; k.soff = v.soff;
  k.r_count = v.r_count; k.gid = v.gid; k.r_rows = v.r_rows; k.pcnt = ch.pcnt; k.pgold = ch.pgold; k.poff = ch.poff; k.ctr = ctr;
  {
    const int kt = ktimer_begin("k_fit_gold", st);
    hipLaunchKernelGGL(k_fit_gold, dim3(gold_grid(n)), dim3(GOLD_BLOCK), 0, st, k);
    ktimer_end(kt, st);
  }
  if (prefix_scan_enqueue(ch.pcnt, ch.n, ch.poff, v.scan_tmp, st, nullptr)) { err = "confusable fit: the prefix sum could not be enqueued"; return ANX_ENODEVICE; }
  uint32_t h[2] = {0u, 0u};  // slots, pairs with a gold slot
  HIP_TRY(hipMemcpyAsync(&h[0], ch.poff + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&h[1], ctr, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h[0] > v.R || h[1] > n) { err = "confusable fit: the state counts more rows than were ranked"; return ANX_EINVAL; }
  ch.total = h[0];
  if ((rc = c->blocks.get(&ch.slots, std::max<size_t>(ch.total, 1), err))) return rc;
  k.slots = ch.slots; k.total = ch.total;
  if (ch.total) {
    const int kt = ktimer_begin("k_fit_state", st);
    hipLaunchKernelGGL(k_fit_state, dim3(gold_grid(ch.total)), dim3(GOLD_BLOCK), 0, st, k);
    ktimer_end(kt, st);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));  // the group's rows may go
  c->chunks.push_back(ch);
  fit_stats_add(FIT_CHUNKS, 1);
  fit_stats_add(FIT_PAIRS, h[1]);
  fit_stats_add(FIT_SLOTS, ch.total);
  fit_stats_add(FIT_BYTES_DOWN, sizeof h);
  return ANX_OK;
}

int fit_round(FitCall* c, const double* cur, const anx_params& p, anx_fit_counts* trials, anx_fit_counts* current, std::string& err) {
  static_assert(sizeof(anx_fit_counts) == 3 * sizeof(unsigned long long), "a cell triple is an anx_fit_counts");
  HIP_TRY(hipSetDevice(c->dl->device));
  hipStream_t st = c->st;
  double* h_cur = reinterpret_cast<double*>(c->h_pin);
  unsigned long long* h_cells = reinterpret_cast<unsigned long long*>(c->h_pin + FIT_MAXP * sizeof(double));
  for (uint32_t j = 0; j < FIT_MAXP; ++j) h_cur[j] = j < c->np ? cur[j] : 1.0;
  HIP_TRY(hipMemcpyAsync(c->d_cur, h_cur, FIT_MAXP * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(c->d_cells, 0, c->ncells * sizeof(unsigned long long), st));
  const size_t lds = c->ncells * sizeof(unsigned long long) + (FIT_MAXP + FIT_MAXG) * sizeof(double);
  const int kt = ktimer_begin("k_fit_trials", st);
  for (const FitChunk& ch : c->chunks) {
    if (!ch.total) continue;  // no pair of the chunk has its gold in its cropped list
    FitTrialArgs k{};
    k.n = ch.n; k.total = ch.total; k.slots = ch.slots; k.poff = ch.poff; k.pcnt = ch.pcnt; k.pgold = ch.pgold; k.cur = c->d_cur; k.grid = c->d_grid;
    k.np = c->np; k.ng = c->ng; k.cutoff_threshold = p.cutoff_threshold; k.freq_weight = p.freq_weight; k.cells = c->d_cells;
    hipLaunchKernelGGL(k_fit_trials, dim3(std::min<unsigned>(gold_grid(ch.n), FIT_MAX_BLOCKS)), dim3(GOLD_BLOCK), lds, st, k);
    fit_stats_add(FIT_TRIAL_LAUNCHES, 1);
  }
  ktimer_end(kt, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h_cells, c->d_cells, c->ncells * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  fit_stats_add(FIT_ROUNDS, 1);
  fit_stats_add(FIT_BYTES_DOWN, c->ncells * sizeof(unsigned long long));
  const anx_fit_counts now{h_cells[0], h_cells[1], h_cells[2]};
  *current = now;
  for (uint32_t j = 0; j < c->np; ++j) {
    const unsigned long long* tc = h_cells + 3u + 3u * j;
    for (uint32_t g = 0; g < c->ng; ++g) {
      anx_fit_counts& t = trials[(size_t)j * c->ng + g];
      if (c->grid[g] == cur[j]) { t = now; continue; }
      const unsigned long long* tt = h_cells + 3u + 3u * c->np + 3u * ((size_t)j * c->ng + g);
      t.at1 = now.at1 - tc[0] + tt[0];  // the pairs pattern j touches: out with their current result, in with the trial's
      t.ranked = now.ranked - tc[1] + tt[1];
      t.rr_fixed = now.rr_fixed - tc[2] + tt[2];
    }
  }
  return ANX_OK;
}

}  // namespace anx
