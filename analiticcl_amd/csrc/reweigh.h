// reweigh.h -- anx_evaluate_sweep_weights: what reweigh_capi.cpp (host: argument checks, chunking, grouping the sets, one base run per
// group) asks of reweigh.hip (device: per group the rows' entry order / frequency / measures once, then per weight set the score, the
// score threshold, the rank through k_rank, the classification and the reduction to a summary).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "engine.h"
#include "sweep.h"

namespace anx {

// One group of sets (equal max_anagram_distance, max_edit_distance, stop_at_exact_match) over one chunk (sweep_chunk_begin's).  begin:
// the base run's rows lie in compact export sections on the chunk's device (anx_eval_gather_rows with want_measures: every instance with
// ld <= d, unpruned), sec_meas[s] one anx_row_measures per record of section s.  k_rw_base keeps per row {pair, entry order, absolute
// frequency, vocabulary id} and the packed measures, and per pair the largest frequency; k_rw_pre the weight-independent reasons of the
// direct pairs under the group's k / d / stop.  Waits for the device: the sections may be freed when it returns.
struct RwGroup;
int reweigh_group_begin(const SweepChunkView& v, const anx_params& group, const std::vector<LearnSection>& secs, const std::vector<size_t>& sec_rows,
                        const std::vector<const anx_row_measures*>& sec_meas, bool want_records, RwGroup** out, std::string& err);
// One set of the group: the rows re-scored under w, tested against p.score_threshold, ranked by k_rank under p (max_matches,
// cutoff_threshold, freq_weight), classified and reduced.  The chunk's counts are ADDED to *sum; out (may be nullptr, needs
// want_records): the n records anx_evaluate_gold writes under p on a model created with w.  baseline: this is set 0 (it writes the
// rank-0 byte per pair every other set compares with).  One download, one wait.
int reweigh_group_set(RwGroup* g, const anx_params& p, const anx_weights& w, bool baseline, anx_gold_summary* sum, anx_gold_eval* out, std::string& err);
// The end of a set by itself (reweigh_group_set ends in it; anx_evaluate_sweep_confusables, csweep.hip, ranks the group's rows its own way
// first): k_rw_classify over the ranked rows the group holds, the direct pair's score under w for THRESHOLD, the reduction, one download,
// one wait.  The group's summary words were cleared on the stream before; *bytes: what came down.
int reweigh_group_finish(RwGroup* g, const anx_params& p, const anx_weights& w, bool baseline, anx_gold_summary* sum, anx_gold_eval* out, size_t* bytes, std::string& err);
size_t reweigh_group_rows(const RwGroup* g);
void reweigh_group_end(RwGroup* g);

// anx_debug_weight_sweep_stats: running totals since process start
enum { RW_CALLS = 0, RW_CHUNKS, RW_GROUPS, RW_SETS, RW_PAIR_PASSES, RW_BATCH_RUNS, RW_ROWS_RESCORED, RW_BYTES_DOWN, RW_NSTATS };
void reweigh_stats_add(int which, uint64_t v);
void reweigh_stats(uint64_t out[RW_NSTATS]);

}  // namespace anx
