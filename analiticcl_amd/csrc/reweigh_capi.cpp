// reweigh_capi.cpp -- anx_evaluate_sweep_weights / _packed: anx_evaluate_sweep's question for sets that also differ in the five score
// weights, answered without a model, a build or a batch run per set.  The argument checks, the chunking and the grouping live here.
// Per chunk of at most 2^20 pairs the set-independent part runs once (anx::sweep_chunk_begin, sweep.hip); the sets are grouped by
// (max_anagram_distance, max_edit_distance, stop_at_exact_match), groups in order of first appearance, so that set 0 is the first set
// of the first group; per group ONE base run through the batch path (anx_eval_gather_rows with max_matches 0, no cutoff, no frequency
// weight and a score threshold of minus infinity: every instance with ld <= d) with explain's measures beside the records; per set
// reweigh.hip re-scores, thresholds, ranks (k_rank), classifies and reduces.  The model's own weights take part in no result.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "engine.h"
#include "eval_gather.h"
#include "host_model.h"
#include "pair_spans.h"
#include "reweigh.h"
#include "sweep.h"

anx::HostModel& anx_learn_host(anx_model* m);
const anx::DeviceLexicon* anx_replica_of(const anx_model* m, size_t i);
std::mutex& anx_learn_mutex();
int anx_fail(int code, const std::string& msg);

namespace {

struct Tail {  // what every form of the call ends in
  const anx_params* sets;
  const anx_weights* weights;
  size_t n_sets;
  anx_gold_summary* summaries;
  anx_gold_eval* out;  // [n_sets][n] or nullptr
};

bool same_threshold(const anx_threshold& a, const anx_threshold& b) {
  return a.kind == b.kind && a.value == b.value && memcmp(&a.ratio, &b.ratio, sizeof a.ratio) == 0;
}
bool same_group(const anx_params& a, const anx_params& b) {
  return same_threshold(a.max_anagram_distance, b.max_anagram_distance) && same_threshold(a.max_edit_distance, b.max_edit_distance) &&
         (a.stop_at_exact_match != 0) == (b.stop_at_exact_match != 0);
}
// finite, none below 0, not all 0 (a sum of 0 makes every score 0 / 0)
bool weights_ok(const anx_weights& w) {
  const double v[5] = {w.ld, w.lcs, w.prefix, w.suffix, w.casew};
  double sum = 0.0;
  for (double x : v) {
    if (!std::isfinite(x) || x < 0.0) return false;
    sum += x;
  }
  return std::isfinite(sum) && sum > 0.0;
}
// The base run scores under the model's own weights and keeps what is >= minus infinity: every number, but no NaN.
bool model_weights_score_numbers(const anx_weights& w) {
  const double v[5] = {w.ld, w.lcs, w.prefix, w.suffix, w.casew};
  double mag = 0.0;
  for (double x : v) {
    if (!std::isfinite(x)) return false;
    mag += std::fabs(x);
  }
  const double sum = w.ld + w.lcs + w.prefix + w.suffix + w.casew;
  return std::isfinite(mag) && sum != 0.0;
}

// one chunk: pairs [lo, lo + cnt) of the call's n
int chunk_run(anx_model* m, const char* const* in, const anx::PairSpan* sa, const anx::PairSpan* sg, size_t lo, size_t cnt, size_t n, const Tail& t,
              const std::vector<std::vector<size_t>>& groups) {
  std::string err;
  anx::LearnVocab** vocab = anx::learn_vocab_slot(m);
  anx::SweepChunk* c = nullptr;
  if (int rc = anx::sweep_chunk_begin(anx_learn_host(m), anx_replica_of(m, 0), vocab, sa, sg, cnt, false, &c, err)) return anx_fail(rc, err);
  struct End { anx::SweepChunk* c; ~End() { anx::sweep_chunk_end(c); } } end{c};
  anx::reweigh_stats_add(anx::RW_CHUNKS, 1);
  anx::reweigh_stats_add(anx::RW_PAIR_PASSES, 1);
  anx::SweepChunkView view;
  anx::sweep_chunk_view(c, &view);
  for (const std::vector<size_t>& members : groups) {
    anx_params base = t.sets[members[0]];
    base.max_matches = 0;
    base.cutoff_threshold = 0.0;
    base.freq_weight = 0.0f;
    base.score_threshold = -std::numeric_limits<double>::infinity();
    anx::RwGroup* g = nullptr;
    {
      anx_eval_gather rows;  // (freed when the group has taken what it needs of the sections)
      rows.want_measures = true;
      const int grc = anx_eval_gather_rows(m, in, sa, cnt, &base, rows);
      anx::reweigh_stats_add(anx::RW_BATCH_RUNS, rows.batch_runs);
      if (grc) return grc;
      if (int rc = anx::reweigh_group_begin(view, base, rows.secs, rows.sec_rows, rows.sec_meas, t.out != nullptr, &g, err)) return anx_fail(rc, err);
    }
    struct GEnd { anx::RwGroup* g; ~GEnd() { anx::reweigh_group_end(g); } } gend{g};
    anx::reweigh_stats_add(anx::RW_GROUPS, 1);
    for (size_t s : members) {
      if (int rc = anx::reweigh_group_set(g, t.sets[s], t.weights[s], s == 0, &t.summaries[s], t.out ? t.out + s * n + lo : nullptr, err)) return anx_fail(rc, err);
      anx::reweigh_stats_add(anx::RW_SETS, 1);
    }
  }
  return ANX_OK;
}

int run_call(anx_model* m, const char* const* in, const std::vector<anx::PairSpan>& sa, const std::vector<anx::PairSpan>& sg, const Tail& t, size_t chunk) {
  const size_t n = sa.size();
  std::vector<std::vector<size_t>> groups;  // by first appearance: set 0 is groups[0][0]
  for (size_t s = 0; s < t.n_sets; ++s) {
    size_t g = 0;
    while (g < groups.size() && !same_group(t.sets[groups[g][0]], t.sets[s])) ++g;
    if (g == groups.size()) groups.emplace_back();
    groups[g].push_back(s);
  }
  std::lock_guard<std::mutex> lk(anx_learn_mutex());
  anx::reweigh_stats_add(anx::RW_CALLS, 1);
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t cnt = std::min(chunk, n - lo);
    if (int rc = chunk_run(m, in ? in + lo : nullptr, sa.data() + lo, sg.data() + lo, lo, cnt, n, t, groups)) return rc;
  }
  return ANX_OK;
}
// everything but the strings themselves; *run = false: the call is answered already (code in the return value)
int check_call(anx_model* m, const void* a, const void* g, size_t n, const Tail& t, bool* run) {
  *run = false;
  if (!m || !t.sets || !t.weights || !t.summaries) return anx_fail(ANX_EINVAL, "NULL argument");
  if (t.n_sets == 0 || t.n_sets > ANX_SWEEP_MAX_SETS) return anx_fail(ANX_EINVAL, "weight sweep: the number of sets is outside 1 .. 256");
  for (size_t s = 0; s < t.n_sets; ++s)
    if (!weights_ok(t.weights[s]))
      return anx_fail(ANX_EINVAL, "weight sweep: set " + std::to_string(s) + " has a weight that is not finite or below 0, or its five weights sum to 0");
  memset(t.summaries, 0, t.n_sets * sizeof(anx_gold_summary));
  if (n == 0) return ANX_OK;
  if (!a || !g) return anx_fail(ANX_EINVAL, "NULL argument");
  const anx::HostModel& h = anx_learn_host(m);
  if (!h.built) return anx_fail(ANX_ENOTBUILT, "Model has not been built yet! Call build() before evaluate_sweep_weights()");
  if (h.lex.any_variants)
    return anx_fail(ANX_EINVAL, "weight sweep: the model has a variant list; the variant score multiplies the score after the weights (plain models only)");
  if (!h.confusables.empty())
    return anx_fail(ANX_EINVAL, "weight sweep: the model has a confusable list; the confusable weight multiplies the score after the weights (plain models only)");
  if (!model_weights_score_numbers(h.weights))
    return anx_fail(ANX_EINVAL, "weight sweep: the model's own weights are not finite or sum to 0: its base run would score NaN");
  if (anx_model_num_replicas(m) < 1 || !anx_replica_of(m, 0))
    return anx_fail(ANX_ENODEVICE, "model is not resident on a device (no HIP device / anx_model_to_device not called)");
  *run = true;
  return ANX_OK;
}
int pointer_call(anx_model* m, const char* const* a, const char* const* g, size_t n, const Tail& t, size_t chunk) {
  bool run;
  if (int rc = check_call(m, a, g, n, t, &run); rc || !run) return rc;
  if (chunk < 1 || chunk > anx::PAIRS_CHUNK) return anx_fail(ANX_EINVAL, "weight sweep: chunk size outside 1 .. 2^20");
  std::vector<anx::PairSpan> sa, sg;
  if (!anx::spans_of_pointers(a, n, sa) || !anx::spans_of_pointers(g, n, sg)) return anx_fail(ANX_EINVAL, "NULL string");
  return run_call(m, a, sa, sg, t, chunk);
}
}  // namespace

extern "C" {
int anx_evaluate_sweep_weights(anx_model* m, const char* const* inputs, const char* const* gold, size_t n, const anx_params* sets, const anx_weights* weights,
                               size_t n_sets, anx_gold_summary* summaries, anx_gold_eval* out) {
  return pointer_call(m, inputs, gold, n, Tail{sets, weights, n_sets, summaries, out}, anx::PAIRS_CHUNK);
}
int anx_debug_evaluate_sweep_weights_chunk(anx_model* m, const char* const* inputs, const char* const* gold, size_t n, const anx_params* sets,
                                           const anx_weights* weights, size_t n_sets, anx_gold_summary* summaries, anx_gold_eval* out, size_t chunk) {
  return pointer_call(m, inputs, gold, n, Tail{sets, weights, n_sets, summaries, out}, chunk);
}
int anx_evaluate_sweep_weights_packed(anx_model* m, const char* blob_in, size_t len_in, const char* blob_gold, size_t len_gold, size_t n, const anx_params* sets,
                                      const anx_weights* weights, size_t n_sets, anx_gold_summary* summaries, anx_gold_eval* out) {
  const Tail t{sets, weights, n_sets, summaries, out};
  bool run;
  if (int rc = check_call(m, blob_in, blob_gold, n, t, &run); rc || !run) return rc;
  if (len_in >= ((size_t)1 << 32) || len_gold >= ((size_t)1 << 32)) return anx_fail(ANX_ELIMIT, "packed pairs exceed 4 GB per blob: split the call");
  std::vector<anx::PairSpan> sa, sg;
  if (!anx::spans_of(blob_in, len_in, n, sa) || !anx::spans_of(blob_gold, len_gold, n, sg)) return anx_fail(ANX_EINVAL, "packed inputs hold fewer strings than announced");
  return run_call(m, nullptr, sa, sg, t, anx::PAIRS_CHUNK);  // (the spans lie back to back, each behind its NUL byte)
}
int anx_debug_weight_sweep_stats(uint64_t* out, int n) {
  if (!out || n < 0) return anx_fail(ANX_EINVAL, "NULL argument");
  uint64_t all[anx::RW_NSTATS];
  anx::reweigh_stats(all);
  for (int i = 0; i < n && i < anx::RW_NSTATS; ++i) out[i] = all[i];
  return ANX_OK;
}
}  // extern "C"
