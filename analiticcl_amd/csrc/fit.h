// fit.h -- anx_fit_confusable_weights: what fit_capi.cpp (host: argument checks, chunking, the greedy rounds and their selection) asks
// of fit.hip (device: per chunk the compact state of the cropped lists that hold their gold, per round every trial of every pair).
#pragma once
#include <cstdint>
#include <string>

#include "csweep.h"
#include "engine.h"

namespace anx {

// One call: the grid on dl's device, a stream of its own, and the state of every chunk added so far.
struct FitCall;
int fit_call_begin(const DeviceLexicon* dl, uint32_t n_patterns, const double* grid, uint32_t n_grid, FitCall** out, std::string& err);
// One chunk, behind csweep_group_rank_late on the chunk's stream: per pair whether its gold is among its cropped rows and where
// (k_fit_gold), the offsets of those pairs' rows in a compact block (the exclusive scan), and per row {dist_score, freq_score, mask}
// with the mask of the row's base row (k_fit_state).  Waits for the chunk's stream: the group may end when it returns.
int fit_chunk_add(FitCall* c, const CsRankedView& v, std::string& err);
// One round over every chunk: trials[j][g] = the counts of "cur with cur[j] = grid[g]" (the current counts where grid[g] == cur[j]),
// *current = the counts under cur.  p: cutoff_threshold and freq_weight.  One download, one wait.
int fit_round(FitCall* c, const double* cur, const anx_params& p, anx_fit_counts* trials, anx_fit_counts* current, std::string& err);
void fit_call_end(FitCall* c);

// anx_debug_fit_stats: running totals since process start
enum { FIT_CALLS = 0, FIT_CHUNKS, FIT_ROUNDS, FIT_TRIAL_LAUNCHES, FIT_PAIRS, FIT_SLOTS, FIT_BYTES_DOWN, FIT_NSTATS };
void fit_stats_add(int which, uint64_t v);
void fit_stats(uint64_t out[FIT_NSTATS]);

}  // namespace anx
