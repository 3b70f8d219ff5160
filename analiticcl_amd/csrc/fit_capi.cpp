// fit_capi.cpp -- anx_fit_confusable_weights / _packed: the weights of candidate confusable patterns fitted over gold pairs by a
// deterministic greedy coordinate ascent (late mode only).  The argument checks, the chunking, the rounds and their selection live here.
// Per chunk of at most 2^20 pairs the confusable sweep's set-independent part runs once -- anx::sweep_chunk_begin, ONE base run through
// the batch path, the masks (anx::csweep_group_begin) and the unweighted late ranking (anx::csweep_group_rank_late) -- and fit.hip keeps
// the cropped lists that hold their gold; then the chunk's group, rows and sections go.  Per round fit.hip evaluates every trial of every
// pair in one launch per chunk, and fit_select picks the round's trial on the host.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "csweep.h"
#include "engine.h"
#include "eval_gather.h"
#include "fit.h"
#include "host_model.h"
#include "pair_spans.h"

anx::HostModel& anx_learn_host(anx_model* m);
const anx::DeviceLexicon* anx_replica_of(const anx_model* m, size_t i);
std::mutex& anx_learn_mutex();
int anx_fail(int code, const std::string& msg);
int anx_csweep_parse_patterns(const char* const* patterns, size_t n_patterns, anx::HostModel::ConfTables& t);
int anx_csweep_check_model(anx_model* m, const char* who);

namespace {

struct Tail {  // what every form of the call ends in
  const char* const* patterns;
  size_t n_patterns;
  const anx_params* params;
  const anx_fit_params* fit;
  double* weights_out;
  anx_fit_round* rounds;
  anx_fit_counts* trials;
  anx_fit_result* result;
};

// the key of a trial: ACC1 (at1, rr_fixed), MRR (rr_fixed, at1)
struct Key { uint64_t a, b; };
Key key_of(const anx_fit_counts& c, uint32_t objective) { return objective == ANX_FIT_MRR ? Key{c.rr_fixed, c.at1} : Key{c.at1, c.rr_fixed}; }
bool key_greater(const Key& x, const Key& y) { return x.a != y.a ? x.a > y.a : x.b > y.b; }
// The round's trial: the largest key among the trials with grid[g] != cur[j], the first in (j, g) order on ties; accepted iff its key
// is greater than the current one and its first component gains at least min_gain.
bool fit_select(const anx_fit_counts* trials, const double* cur, size_t np, const double* grid, size_t ng, const anx_fit_counts& now, uint32_t objective,
                uint64_t min_gain, size_t* pattern, size_t* grid_index) {
  bool have = false;
  Key best{0, 0};
  size_t bj = 0, bg = 0;
  for (size_t j = 0; j < np; ++j)
    for (size_t g = 0; g < ng; ++g) {
      if (grid[g] == cur[j]) continue;  // not a trial
      const Key k = key_of(trials[j * ng + g], objective);
      if (!have || key_greater(k, best)) { have = true; best = k; bj = j; bg = g; }
    }
  if (!have) return false;
  const Key c = key_of(now, objective);
  if (!key_greater(best, c)) return false;
  if (best.a < c.a || best.a - c.a < min_gain) return false;
  *pattern = bj; *grid_index = bg;
  return true;
}

bool weight_ok(double w) { return std::isfinite(w) && w > 0.0; }

// one chunk into the fit's state: pairs [lo, lo + cnt)
int chunk_state(anx_model* m, anx::CsCall* call, anx::FitCall* fit, const char* const* in, const anx::PairSpan* sa, const anx::PairSpan* sg, size_t cnt, const anx_params& p) {
  std::string err;
  anx::LearnVocab** vocab = anx::learn_vocab_slot(m);
  anx::SweepChunk* c = nullptr;
  if (int rc = anx::sweep_chunk_begin(anx_learn_host(m), anx_replica_of(m, 0), vocab, sa, sg, cnt, false, &c, err)) return anx_fail(rc, err);
  struct End { anx::SweepChunk* c; ~End() { anx::sweep_chunk_end(c); } } end{c};
  anx::SweepChunkView view;
  anx::sweep_chunk_view(c, &view);
  anx_params base = p;  // as csweep_capi.cpp: every instance with ld <= d
  base.max_matches = 0;
  base.cutoff_threshold = 0.0;
  base.freq_weight = 0.0f;
  base.score_threshold = -std::numeric_limits<double>::infinity();
  anx::CsGroup* g = nullptr;
  {
    anx_eval_gather rows;  // (freed when the group has taken what it needs of the sections)
    rows.want_measures = true;
    if (const int grc = anx_eval_gather_rows(m, in, sa, cnt, &base, rows)) return grc;
    if (int rc = anx::csweep_group_begin(call, view, base, rows.secs, rows.sec_rows, rows.sec_meas, false, sa, &g, err)) return anx_fail(rc, err);
  }
  struct GEnd { anx::CsGroup* g; ~GEnd() { anx::csweep_group_end(g); } } gend{g};
  anx::CsRankedView ranked{};
  if (int rc = anx::csweep_group_rank_late(g, p, &ranked, err)) return anx_fail(rc, err);
  if (int rc = anx::fit_chunk_add(fit, ranked, err)) return anx_fail(rc, err);
  return ANX_OK;
}

int run_call(anx_model* m, const char* const* in, const std::vector<anx::PairSpan>& sa, const std::vector<anx::PairSpan>& sg, const Tail& t,
             const anx::HostModel::ConfTables& tables, size_t chunk) {
  const size_t n = sa.size(), np = t.n_patterns, ng = t.fit->n_grid;
  const anx_fit_params& f = *t.fit;
  std::lock_guard<std::mutex> lk(anx_learn_mutex());
  anx::fit_stats_add(anx::FIT_CALLS, 1);
  std::string err;
  anx::FitCall* fit = nullptr;
  if (int rc = anx::fit_call_begin(anx_replica_of(m, 0), (uint32_t)np, f.grid, (uint32_t)ng, &fit, err)) return anx_fail(rc, err);
  struct FEnd { anx::FitCall* c; ~FEnd() { anx::fit_call_end(c); } } fend{fit};
  {
    const std::vector<double> ones(np, 1.0);  // (the ranking the state is cut from is unweighted)
    anx::CsCall* call = nullptr;
    if (int rc = anx::csweep_call_begin(anx_learn_host(m), anx_replica_of(m, 0), tables, ones.data(), 1, &call, err)) return anx_fail(rc, err);
    struct CEnd { anx::CsCall* c; ~CEnd() { anx::csweep_call_end(c); } } cend{call};
    for (size_t lo = 0; lo < n; lo += chunk) {
      const size_t cnt = std::min(chunk, n - lo);
      if (int rc = chunk_state(m, call, fit, in ? in + lo : nullptr, sa.data() + lo, sg.data() + lo, cnt, *t.params)) return rc;
    }
  }
  // the rounds: no text, no rows and no rank from here on
  std::vector<anx_fit_counts> table(np * ng);
  anx_fit_result& res = *t.result;
  double* cur = t.weights_out;
  for (;;) {
    anx_fit_counts now{};
    if (int rc = anx::fit_round(fit, cur, *t.params, table.data(), &now, err)) return anx_fail(rc, err);
    if (t.trials) memcpy(t.trials + (size_t)res.n_trial_rounds * np * ng, table.data(), np * ng * sizeof(anx_fit_counts));
    if (res.n_trial_rounds == 0) res.start = res.final = now;
    ++res.n_trial_rounds;
    size_t j = 0, g = 0;
    if (!fit_select(table.data(), cur, np, f.grid, ng, now, f.objective, f.min_gain, &j, &g)) { res.stop = 0; break; }
    cur[j] = f.grid[g];
    res.final = table[j * ng + g];
    t.rounds[res.n_rounds++] = anx_fit_round{(uint32_t)j, (uint32_t)g, f.grid[g], res.final};
    if (res.n_rounds == f.max_rounds) { res.stop = 1; break; }
  }
  return ANX_OK;
}

// everything but the strings themselves; *run = false: the call is answered already (code in the return value)
int check_call(anx_model* m, const void* a, const void* g, size_t n, const Tail& t, anx::HostModel::ConfTables& tables, bool* run) {
  *run = false;
  if (!m || !t.patterns || !t.params || !t.fit || !t.weights_out || !t.rounds || !t.result || !t.fit->grid) return anx_fail(ANX_EINVAL, "NULL argument");
  const anx_fit_params& f = *t.fit;
  if (int rc = anx_csweep_parse_patterns(t.patterns, t.n_patterns, tables)) return rc;
  if (f.n_grid == 0 || f.n_grid > ANX_FIT_MAX_GRID) return anx_fail(ANX_EINVAL, "confusable fit: the number of grid weights is outside 1 .. 16");
  if (f.max_rounds == 0 || f.max_rounds > ANX_FIT_MAX_ROUNDS) return anx_fail(ANX_EINVAL, "confusable fit: max_rounds is outside 1 .. 256");
  if (f.objective != ANX_FIT_ACC1 && f.objective != ANX_FIT_MRR) return anx_fail(ANX_EINVAL, "confusable fit: unknown objective " + std::to_string(f.objective));
  for (uint32_t g2 = 0; g2 < f.n_grid; ++g2)
    if (!weight_ok(f.grid[g2])) return anx_fail(ANX_EINVAL, "confusable fit: grid weight " + std::to_string(g2) + " is not finite or not above 0");
  for (size_t j = 0; f.start && j < t.n_patterns; ++j)
    if (!weight_ok(f.start[j])) return anx_fail(ANX_EINVAL, "confusable fit: start weight " + std::to_string(j) + " is not finite or not above 0");
  memset(t.result, 0, sizeof(anx_fit_result));
  for (size_t j = 0; j < t.n_patterns; ++j) t.weights_out[j] = f.start ? f.start[j] : 1.0;
  if (n == 0) return ANX_OK;
  if (!a || !g) return anx_fail(ANX_EINVAL, "NULL argument");
  if (n > ANX_FIT_MAX_PAIRS) return anx_fail(ANX_ELIMIT, "confusable fit: more than 2^24 pairs in one call (16 chunks of resident state): split the pairs");
  const anx::HostModel& h = anx_learn_host(m);
  if (anx::switches().confusables_host && !h.confusables.empty())
    return anx_fail(ANX_EINVAL, "confusable fit: confusables are weighted on the host (ANX_CONFUSABLES=host): the ranked rows exist on the host only");
  if (h.confusables_before_pruning)
    return anx_fail(ANX_EINVAL, "confusable fit: the model weights confusables before pruning (set_confusables_before_pruning); the fit is late mode only");
  if (int rc = anx_csweep_check_model(m, "fit_confusable_weights")) return rc;
  *run = true;
  return ANX_OK;
}
int pointer_call(anx_model* m, const char* const* a, const char* const* g, size_t n, const Tail& t, size_t chunk) {
  bool run;
  anx::HostModel::ConfTables tables;
  if (int rc = check_call(m, a, g, n, t, tables, &run); rc || !run) return rc;
  if (chunk < 1 || chunk > anx::PAIRS_CHUNK) return anx_fail(ANX_EINVAL, "confusable fit: chunk size outside 1 .. 2^20");
  std::vector<anx::PairSpan> sa, sg;
  if (!anx::spans_of_pointers(a, n, sa) || !anx::spans_of_pointers(g, n, sg)) return anx_fail(ANX_EINVAL, "NULL string");
  return run_call(m, a, sa, sg, t, tables, chunk);
}

}  // namespace

extern "C" {
int anx_fit_confusable_weights(anx_model* m, const char* const* inputs, const char* const* gold, size_t n, const char* const* patterns, size_t n_patterns,
                               const anx_params* params, const anx_fit_params* fit, double* weights_out, anx_fit_round* rounds, anx_fit_counts* trials,
                               anx_fit_result* result) {
  return pointer_call(m, inputs, gold, n, Tail{patterns, n_patterns, params, fit, weights_out, rounds, trials, result}, anx::PAIRS_CHUNK);
}
int anx_debug_fit_confusable_weights_chunk(anx_model* m, const char* const* inputs, const char* const* gold, size_t n, const char* const* patterns,
                                           size_t n_patterns, const anx_params* params, const anx_fit_params* fit, double* weights_out, anx_fit_round* rounds,
                                           anx_fit_counts* trials, anx_fit_result* result, size_t chunk) {
  return pointer_call(m, inputs, gold, n, Tail{patterns, n_patterns, params, fit, weights_out, rounds, trials, result}, chunk);
}
int anx_fit_confusable_weights_packed(anx_model* m, const char* blob_in, size_t len_in, const char* blob_gold, size_t len_gold, size_t n,
                                      const char* const* patterns, size_t n_patterns, const anx_params* params, const anx_fit_params* fit, double* weights_out,
                                      anx_fit_round* rounds, anx_fit_counts* trials, anx_fit_result* result) {
  const Tail t{patterns, n_patterns, params, fit, weights_out, rounds, trials, result};
  bool run;
  anx::HostModel::ConfTables tables;
  if (int rc = check_call(m, blob_in, blob_gold, n, t, tables, &run); rc || !run) return rc;
  if (len_in >= ((size_t)1 << 32) || len_gold >= ((size_t)1 << 32)) return anx_fail(ANX_ELIMIT, "packed pairs exceed 4 GB per blob: split the call");
  std::vector<anx::PairSpan> sa, sg;
  if (!anx::spans_of(blob_in, len_in, n, sa) || !anx::spans_of(blob_gold, len_gold, n, sg)) return anx_fail(ANX_EINVAL, "packed inputs hold fewer strings than announced");
  return run_call(m, nullptr, sa, sg, t, tables, anx::PAIRS_CHUNK);  // (the spans lie back to back, each behind its NUL byte)
}
int anx_debug_fit_select(const anx_fit_counts* trials, const double* cur, size_t n_patterns, const double* grid, size_t n_grid, const anx_fit_counts* cur_counts,
                         uint32_t objective, uint64_t min_gain, int32_t* pattern, int32_t* grid_index) {
  if (!trials || !cur || !grid || !cur_counts || !pattern || !grid_index) return anx_fail(ANX_EINVAL, "NULL argument");
  if (n_patterns == 0 || n_patterns > ANX_SWEEP_CONF_MAX_PATTERNS || n_grid == 0 || n_grid > ANX_FIT_MAX_GRID)
    return anx_fail(ANX_EINVAL, "confusable fit: 1 .. 64 patterns and 1 .. 16 grid weights");
  if (objective != ANX_FIT_ACC1 && objective != ANX_FIT_MRR) return anx_fail(ANX_EINVAL, "confusable fit: unknown objective " + std::to_string(objective));
  size_t j = 0, g = 0;
  const bool ok = fit_select(trials, cur, n_patterns, grid, n_grid, *cur_counts, objective, min_gain, &j, &g);
  *pattern = ok ? (int32_t)j : -1;
  *grid_index = ok ? (int32_t)g : -1;
  return ANX_OK;
}
int anx_debug_fit_stats(uint64_t* out, int n) {
  if (!out || n < 0) return anx_fail(ANX_EINVAL, "NULL argument");
  uint64_t all[anx::FIT_NSTATS];
  anx::fit_stats(all);
  for (int i = 0; i < n && i < anx::FIT_NSTATS; ++i) out[i] = all[i];
  return ANX_OK;
}
}  // extern "C"
