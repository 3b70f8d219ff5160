// csweep_capi.cpp -- anx_evaluate_sweep_confusables / _packed: anx_evaluate_gold's question for a model that held the candidate patterns
// as its confusable list, once per assignment of weights to them, answered without a model, a batch run or an edit script per set.  The
// argument checks, the pattern parser, the chunking and the grouping live here.  Per chunk of at most 2^20 pairs the set-independent part
// runs once (anx::sweep_chunk_begin, sweep.hip); the sets are grouped by (max_anagram_distance, max_edit_distance, stop_at_exact_match),
// groups in order of first appearance, so that set 0 is the first set of the first group; per group ONE base run through the batch path
// (as reweigh_capi.cpp) and one mask pass (csweep.hip); per set csweep.hip applies the set's weights, ranks, classifies and reduces.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "csweep.h"
#include "engine.h"
#include "eval_gather.h"
#include "host_model.h"
#include "pair_spans.h"

anx::HostModel& anx_learn_host(anx_model* m);
const anx::DeviceLexicon* anx_replica_of(const anx_model* m, size_t i);
std::mutex& anx_learn_mutex();
int anx_fail(int code, const std::string& msg);

namespace {

struct Tail {  // what every form of the call ends in
  const char* const* patterns;
  size_t n_patterns;
  const anx_params* sets;
  const double* weights;   // [n_sets][n_patterns]
  const uint8_t* early;    // [n_sets] or nullptr
  size_t n_sets;
  anx_gold_summary* summaries;
  anx_gold_eval* out;      // [n_sets][n] or nullptr
};

bool same_threshold(const anx_threshold& a, const anx_threshold& b) {
  return a.kind == b.kind && a.value == b.value && memcmp(&a.ratio, &b.ratio, sizeof a.ratio) == 0;
}
bool same_group(const anx_params& a, const anx_params& b) {
  return same_threshold(a.max_anagram_distance, b.max_anagram_distance) && same_threshold(a.max_edit_distance, b.max_edit_distance) &&
         (a.stop_at_exact_match != 0) == (b.stop_at_exact_match != 0);
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
}  // namespace
// the candidate patterns through the list parser, flattened as a model's list is; the weights in the tables are 1.0 (the sets carry them)
// (also the confusable fit's, fit_capi.cpp)
int anx_csweep_parse_patterns(const char* const* patterns, size_t n_patterns, anx::HostModel::ConfTables& t) {
  if (!patterns) return anx_fail(ANX_EINVAL, "NULL argument");
  if (n_patterns == 0 || n_patterns > ANX_SWEEP_CONF_MAX_PATTERNS) return anx_fail(ANX_EINVAL, "confusable sweep: the number of patterns is outside 1 .. 64");
  std::vector<anx::Confusable> list(n_patterns);
  for (size_t j = 0; j < n_patterns; ++j) {
    std::string err;
    if (!patterns[j]) return anx_fail(ANX_EINVAL, "confusable sweep: pattern " + std::to_string(j) + " is NULL");
    if (anx::parse_confusable(patterns[j], 1.0, list[j], err)) return anx_fail(ANX_EINVAL, "confusable sweep: pattern " + std::to_string(j) + ": " + err);
  }
  anx::conf_tables_build(list, t);
  return ANX_OK;
}
namespace {

// one chunk: pairs [lo, lo + cnt) of the call's n
int chunk_run(anx_model* m, anx::CsCall* call, const char* const* in, const anx::PairSpan* sa, const anx::PairSpan* sg, size_t lo, size_t cnt, size_t n, const Tail& t,
              const std::vector<std::vector<size_t>>& groups) {
  std::string err;
  anx::LearnVocab** vocab = anx::learn_vocab_slot(m);
  anx::SweepChunk* c = nullptr;
  if (int rc = anx::sweep_chunk_begin(anx_learn_host(m), anx_replica_of(m, 0), vocab, sa, sg, cnt, false, &c, err)) return anx_fail(rc, err);
  struct End { anx::SweepChunk* c; ~End() { anx::sweep_chunk_end(c); } } end{c};
  anx::csweep_stats_add(anx::CS_CHUNKS, 1);
  anx::csweep_stats_add(anx::CS_PAIR_PASSES, 1);
  anx::SweepChunkView view;
  anx::sweep_chunk_view(c, &view);
  for (const std::vector<size_t>& members : groups) {
    anx_params base = t.sets[members[0]];
    base.max_matches = 0;
    base.cutoff_threshold = 0.0;
    base.freq_weight = 0.0f;
    base.score_threshold = -std::numeric_limits<double>::infinity();
    anx::CsGroup* g = nullptr;
    {
      anx_eval_gather rows;  // (freed when the group has taken what it needs of the sections)
      rows.want_measures = true;
      const int grc = anx_eval_gather_rows(m, in, sa, cnt, &base, rows);
      anx::csweep_stats_add(anx::CS_BATCH_RUNS, rows.batch_runs);
      if (grc) return grc;
      if (int rc = anx::csweep_group_begin(call, view, base, rows.secs, rows.sec_rows, rows.sec_meas, t.out != nullptr, sa, &g, err)) return anx_fail(rc, err);
    }
    struct GEnd { anx::CsGroup* g; ~GEnd() { anx::csweep_group_end(g); } } gend{g};
    anx::csweep_stats_add(anx::CS_GROUPS, 1);
    for (size_t s : members) {
      if (int rc = anx::csweep_group_set(g, t.sets[s], s, t.early && t.early[s], s == 0, &t.summaries[s], t.out ? t.out + s * n + lo : nullptr, err)) return anx_fail(rc, err);
      anx::csweep_stats_add(anx::CS_SETS, 1);
    }
  }
  return ANX_OK;
}

int run_call(anx_model* m, const char* const* in, const std::vector<anx::PairSpan>& sa, const std::vector<anx::PairSpan>& sg, const Tail& t,
             const anx::HostModel::ConfTables& tables, size_t chunk) {
  const size_t n = sa.size();
  std::vector<std::vector<size_t>> groups;  // by first appearance: set 0 is groups[0][0]
  for (size_t s = 0; s < t.n_sets; ++s) {
    size_t g = 0;
    while (g < groups.size() && !same_group(t.sets[groups[g][0]], t.sets[s])) ++g;
    if (g == groups.size()) groups.emplace_back();
    groups[g].push_back(s);
  }
  std::lock_guard<std::mutex> lk(anx_learn_mutex());
  anx::csweep_stats_add(anx::CS_CALLS, 1);
  std::string err;
  anx::CsCall* call = nullptr;
  if (int rc = anx::csweep_call_begin(anx_learn_host(m), anx_replica_of(m, 0), tables, t.weights, t.n_sets, &call, err)) return anx_fail(rc, err);
  struct CEnd { anx::CsCall* c; ~CEnd() { anx::csweep_call_end(c); } } cend{call};
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t cnt = std::min(chunk, n - lo);
    if (int rc = chunk_run(m, call, in ? in + lo : nullptr, sa.data() + lo, sg.data() + lo, lo, cnt, n, t, groups)) return rc;
  }
  return ANX_OK;
}
}  // namespace
// what is refused because of the model, before the device is asked for (also the confusable fit's, fit_capi.cpp)
int anx_csweep_check_model(anx_model* m, const char* who) {
  const anx::HostModel& h = anx_learn_host(m);
  if (!h.built) return anx_fail(ANX_ENOTBUILT, std::string("Model has not been built yet! Call build() before ") + who + "()");
  if (h.lex.any_variants)
    return anx_fail(ANX_EINVAL, "confusable sweep: the model has a variant list; a row reached through a variant is weighted by the variant's text (not built)");
  if (!h.confusables.empty())
    return anx_fail(ANX_EINVAL, "confusable sweep: the model has a confusable list of its own; the candidates would multiply on top of it (not built)");
  if (!model_weights_score_numbers(h.weights))
    return anx_fail(ANX_EINVAL, "confusable sweep: the model's own weights are not finite or sum to 0: its base run would score NaN");
  if (anx_model_num_replicas(m) < 1 || !anx_replica_of(m, 0))
    return anx_fail(ANX_ENODEVICE, "model is not resident on a device (no HIP device / anx_model_to_device not called)");
  return ANX_OK;
}
namespace {
// everything but the strings themselves; *run = false: the call is answered already (code in the return value)
int check_call(anx_model* m, const void* a, const void* g, size_t n, const Tail& t, anx::HostModel::ConfTables& tables, bool* run) {
  *run = false;
  if (!m || !t.sets || !t.weights || !t.summaries || !t.patterns) return anx_fail(ANX_EINVAL, "NULL argument");
  if (t.n_sets == 0 || t.n_sets > ANX_SWEEP_MAX_SETS) return anx_fail(ANX_EINVAL, "confusable sweep: the number of sets is outside 1 .. 256");
  if (int rc = anx_csweep_parse_patterns(t.patterns, t.n_patterns, tables)) return rc;
  for (size_t s = 0; s < t.n_sets; ++s)
    for (size_t j = 0; j < t.n_patterns; ++j) {
      const double w = t.weights[s * t.n_patterns + j];
      if (!std::isfinite(w) || !(w > 0.0))
        return anx_fail(ANX_EINVAL, "confusable sweep: set " + std::to_string(s) + " gives pattern " + std::to_string(j) + " a weight that is not finite or not above 0");
    }
  memset(t.summaries, 0, t.n_sets * sizeof(anx_gold_summary));
  if (n == 0) return ANX_OK;
  if (!a || !g) return anx_fail(ANX_EINVAL, "NULL argument");
  if (int rc = anx_csweep_check_model(m, "evaluate_sweep_confusables")) return rc;
  *run = true;
  return ANX_OK;
}
int pointer_call(anx_model* m, const char* const* a, const char* const* g, size_t n, const Tail& t, size_t chunk) {
  bool run;
  anx::HostModel::ConfTables tables;
  if (int rc = check_call(m, a, g, n, t, tables, &run); rc || !run) return rc;
  if (chunk < 1 || chunk > anx::PAIRS_CHUNK) return anx_fail(ANX_EINVAL, "confusable sweep: chunk size outside 1 .. 2^20");
  std::vector<anx::PairSpan> sa, sg;
  if (!anx::spans_of_pointers(a, n, sa) || !anx::spans_of_pointers(g, n, sg)) return anx_fail(ANX_EINVAL, "NULL string");
  return run_call(m, a, sa, sg, t, tables, chunk);
}
template <typename T>
T* to_malloc(const std::vector<T>& v) {
  T* p = static_cast<T*>(malloc(std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (p && !v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}
}  // namespace

extern "C" {
int anx_evaluate_sweep_confusables(anx_model* m, const char* const* inputs, const char* const* gold, size_t n, const char* const* patterns, size_t n_patterns,
                                   const anx_params* sets, const double* weights, const uint8_t* early, size_t n_sets, anx_gold_summary* summaries, anx_gold_eval* out) {
  return pointer_call(m, inputs, gold, n, Tail{patterns, n_patterns, sets, weights, early, n_sets, summaries, out}, anx::PAIRS_CHUNK);
}
int anx_debug_evaluate_sweep_confusables_chunk(anx_model* m, const char* const* inputs, const char* const* gold, size_t n, const char* const* patterns,
                                               size_t n_patterns, const anx_params* sets, const double* weights, const uint8_t* early, size_t n_sets,
                                               anx_gold_summary* summaries, anx_gold_eval* out, size_t chunk) {
  return pointer_call(m, inputs, gold, n, Tail{patterns, n_patterns, sets, weights, early, n_sets, summaries, out}, chunk);
}
int anx_evaluate_sweep_confusables_packed(anx_model* m, const char* blob_in, size_t len_in, const char* blob_gold, size_t len_gold, size_t n,
                                          const char* const* patterns, size_t n_patterns, const anx_params* sets, const double* weights, const uint8_t* early,
                                          size_t n_sets, anx_gold_summary* summaries, anx_gold_eval* out) {
  const Tail t{patterns, n_patterns, sets, weights, early, n_sets, summaries, out};
  bool run;
  anx::HostModel::ConfTables tables;
  if (int rc = check_call(m, blob_in, blob_gold, n, t, tables, &run); rc || !run) return rc;
  if (len_in >= ((size_t)1 << 32) || len_gold >= ((size_t)1 << 32)) return anx_fail(ANX_ELIMIT, "packed pairs exceed 4 GB per blob: split the call");
  std::vector<anx::PairSpan> sa, sg;
  if (!anx::spans_of(blob_in, len_in, n, sa) || !anx::spans_of(blob_gold, len_gold, n, sg)) return anx_fail(ANX_EINVAL, "packed inputs hold fewer strings than announced");
  return run_call(m, nullptr, sa, sg, t, tables, anx::PAIRS_CHUNK);  // (the spans lie back to back, each behind its NUL byte)
}
int anx_debug_sweep_conf_masks(anx_model* m, const char* const* inputs, size_t n, const char* const* patterns, size_t n_patterns, const anx_params* group,
                               uint32_t** pair, uint32_t** vocab, uint64_t** mask, size_t* rows) {
  if (!m || !inputs || !group || !pair || !vocab || !mask || !rows) return anx_fail(ANX_EINVAL, "NULL argument");
  if (n == 0 || n > anx::PAIRS_CHUNK) return anx_fail(ANX_EINVAL, "anx_debug_sweep_conf_masks: 1 .. 2^20 inputs");
  anx::HostModel::ConfTables tables;
  if (int rc = anx_csweep_parse_patterns(patterns, n_patterns, tables)) return rc;
  if (int rc = anx_csweep_check_model(m, "anx_debug_sweep_conf_masks")) return rc;
  std::vector<anx::PairSpan> sa;
  if (!anx::spans_of_pointers(inputs, n, sa)) return anx_fail(ANX_EINVAL, "NULL string");
  std::lock_guard<std::mutex> lk(anx_learn_mutex());
  std::string err;
  const std::vector<double> ones(n_patterns, 1.0);
  anx::CsCall* call = nullptr;
  if (int rc = anx::csweep_call_begin(anx_learn_host(m), anx_replica_of(m, 0), tables, ones.data(), 1, &call, err)) return anx_fail(rc, err);
  struct CEnd { anx::CsCall* c; ~CEnd() { anx::csweep_call_end(c); } } cend{call};
  anx::SweepChunk* c = nullptr;  // (the gold side of the chunk: the inputs themselves; nothing here reads it)
  if (int rc = anx::sweep_chunk_begin(anx_learn_host(m), anx_replica_of(m, 0), anx::learn_vocab_slot(m), sa.data(), sa.data(), n, false, &c, err)) return anx_fail(rc, err);
  struct End { anx::SweepChunk* c; ~End() { anx::sweep_chunk_end(c); } } end{c};
  anx::SweepChunkView view;
  anx::sweep_chunk_view(c, &view);
  anx_params base = *group;
  base.max_matches = 0;
  base.cutoff_threshold = 0.0;
  base.freq_weight = 0.0f;
  base.score_threshold = -std::numeric_limits<double>::infinity();
  anx::CsGroup* g = nullptr;
  {
    anx_eval_gather gathered;
    gathered.want_measures = true;
    if (const int grc = anx_eval_gather_rows(m, inputs, sa.data(), n, &base, gathered)) return grc;
    if (int rc = anx::csweep_group_begin(call, view, base, gathered.secs, gathered.sec_rows, gathered.sec_meas, false, sa.data(), &g, err)) return anx_fail(rc, err);
  }
  struct GEnd { anx::CsGroup* g; ~GEnd() { anx::csweep_group_end(g); } } gend{g};
  std::vector<uint32_t> hp, hv;
  std::vector<uint64_t> hm;
  if (int rc = anx::csweep_group_masks(g, hp, hv, hm, err)) return anx_fail(rc, err);
  *pair = to_malloc(hp); *vocab = to_malloc(hv); *mask = to_malloc(hm);
  if (!*pair || !*vocab || !*mask) { free(*pair); free(*vocab); free(*mask); return anx_fail(ANX_EINVAL, "out of host memory"); }
  *rows = hp.size();
  return ANX_OK;
}
int anx_debug_conf_mask_text(const char* const* patterns, size_t n_patterns, const char* a, const char* b, uint64_t* mask) {
  if (!a || !b || !mask) return anx_fail(ANX_EINVAL, "NULL argument");
  anx::HostModel::ConfTables tables;
  if (int rc = anx_csweep_parse_patterns(patterns, n_patterns, tables)) return rc;
  *mask = anx::confusable_mask_text(tables, a, strlen(a), b, strlen(b));
  return ANX_OK;
}
int anx_debug_conf_sweep_stats(uint64_t* out, int n) {
  if (!out || n < 0) return anx_fail(ANX_EINVAL, "NULL argument");
  uint64_t all[anx::CS_NSTATS];
  anx::csweep_stats(all);
  for (int i = 0; i < n && i < anx::CS_NSTATS; ++i) out[i] = all[i];
  return ANX_OK;
}
}  // extern "C"
