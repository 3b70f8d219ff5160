// csweep.h -- anx_evaluate_sweep_confusables: what csweep_capi.cpp (host: argument checks, the candidate patterns parsed and flattened,
// chunking, grouping the sets, one base run per group) asks of csweep.hip (device: per call the patterns and the vocabulary's text, per
// group the unweighted score and ONE 64-bit match mask per base row, then per set the weights applied to the masks -- early before
// k_rank, late through k_conf_apply_late -- the classification and the reduction to a summary).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "engine.h"
#include "pair_spans.h"
#include "reweigh.h"
#include "sweep.h"

namespace anx {

// Once per call: the flattened candidate patterns, the weights of every set ([n_sets][n_patterns], row-major) and -- on first use -- the
// vocabulary as code points with presence bits on dl's device.  `t` and `weights` are read during begin only.
struct CsCall;
int csweep_call_begin(const HostModel& m, const DeviceLexicon* dl, const HostModel::ConfTables& t, const double* weights, size_t n_sets, CsCall** out, std::string& err);
void csweep_call_end(CsCall* c);

// One group of sets (equal max_anagram_distance, max_edit_distance, stop_at_exact_match) over one chunk: reweigh_group_begin's base rows,
// their score under the model's weights, and their masks: k_cs_screen (presence bits: rows no pattern can match get 0, the others a place
// in a dense list), the list ordered by script shape, the k_cs_mask_* kernels (edit script, found_in per pattern).  Rows the lane memory cannot hold are
// computed by the host from `inputs` (the chunk's input spans, host text) and patched in; under ANX_CONFUSABLES=host every row is.
// Waits for the device: the sections may be freed when it returns.
struct CsGroup;
int csweep_group_begin(CsCall* c, const SweepChunkView& v, const anx_params& group, const std::vector<LearnSection>& secs, const std::vector<size_t>& sec_rows,
                       const std::vector<const anx_row_measures*>& sec_meas, bool want_records, const PairSpan* inputs, CsGroup** out, std::string& err);
// One set of the group: `set` indexes the call's weights.  early: rows with an unweighted score >= p.score_threshold, score times the
// weight of the row's mask, k_rank under p.  late: the unweighted rows through k_rank without a cutoff, the weight of every ranked slot,
// then k_conf_apply_late (stable re-sort, p's cutoff).  The chunk's counts are ADDED to *sum; out may be nullptr (needs want_records).
// One download, one wait, no edit script.
int csweep_group_set(CsGroup* g, const anx_params& p, size_t set, bool early, bool baseline, anx_gold_summary* sum, anx_gold_eval* out, std::string& err);
// The front of a late set by itself, for the confusable fit (fit.hip): the unweighted rows with a score >= p.score_threshold through
// k_rank under p's max_matches / freq_weight without a cutoff -- the cropped lists every late weight assignment re-ranks.  Enqueued on the
// chunk's stream, no wait; k_conf_apply_late has NOT run.  The view's arrays are the group's and live until csweep_group_end.
struct DevRow;
struct CsRankedView {
  const DeviceLexicon* dl;
  void* stream;
  size_t n, R;                     // pairs of the chunk; base rows of the group (the capacity of r_rows)
  const void* info;                // [R] uint4 {pair, ., ., vocabulary id} per base row
  const unsigned long long* mask;  // [R] the base rows' match masks
  const uint32_t *rbeg, *rend;     // [n] the pair's range of base rows
  const uint32_t* soff;            // [n + 1] where the pair's ranked rows begin in r_rows
  const uint32_t* r_count;         // [n] ranked rows of the pair
  const uint32_t* gid;             // [n] gold id or 0xFFFFFFFF
  const DevRow* r_rows;
  uint32_t* scan_tmp;              // prefix_scan_tmp_bytes(n), free once the rank is enqueued
};
int csweep_group_rank_late(CsGroup* g, const anx_params& p, CsRankedView* out, std::string& err);
// anx_debug_sweep_conf_masks: the group's base rows as (pair, vocabulary id, mask); rows without a pair are left out
int csweep_group_masks(CsGroup* g, std::vector<uint32_t>& pair, std::vector<uint32_t>& vocab, std::vector<uint64_t>& mask, std::string& err);
void csweep_group_end(CsGroup* g);

// anx_debug_conf_sweep_stats: running totals since process start
enum { CS_CALLS = 0, CS_CHUNKS, CS_GROUPS, CS_SETS, CS_PAIR_PASSES, CS_BATCH_RUNS, CS_BASE_ROWS, CS_ROWS_LISTED, CS_ROWS_PATCHED, CS_ROWS_HOST_MODE,
       CS_BYTES_DOWN, CS_NSTATS };
void csweep_stats_add(int which, uint64_t v);
void csweep_stats(uint64_t out[CS_NSTATS]);

}  // namespace anx
