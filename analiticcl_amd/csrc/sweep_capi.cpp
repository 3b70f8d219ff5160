// sweep_capi.cpp -- anx_evaluate_sweep / anx_evaluate_sweep_packed: anx_evaluate_gold's question for several parameter sets over the
// same (input, gold) pairs, answered per set as an anx_gold_summary reduced on the device (and, when asked for, the records).
// The argument checks and the chunking live here.  Per chunk of at most 2^20 pairs the part that does not depend on the set -- the
// spans, the upload of the 2 n strings, the encoder, the pair kernels, the gold lookup, the vocabulary flags -- runs once
// (anx::sweep_chunk_begin, sweep.hip) and stays on replica 0's device; then every set sends the chunk's inputs through the batch
// pipeline as anx_evaluate_gold does (anx_eval_gather_rows, eval_capi.cpp), sweep.hip classifies and reduces under that set, and the
// set's gather buffers go back to the pool before the next set starts.  The model is reached through the accessors capi.cpp defines
// for learn mode and the exports; the vocabulary table is learn mode's, under its lock.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "engine.h"
#include "eval_gather.h"
#include "host_model.h"
#include "pair_spans.h"
#include "sweep.h"

anx::HostModel& anx_learn_host(anx_model* m);
const anx::DeviceLexicon* anx_replica_of(const anx_model* m, size_t i);
std::mutex& anx_learn_mutex();
int anx_fail(int code, const std::string& msg);

namespace {

struct Tail {  // what every form of the call ends in
  const anx_params* sets;
  size_t n_sets;
  anx_gold_summary* summaries;
  anx_gold_eval* out;     // [n_sets][n] or nullptr
  anx_pair_score* pairs;  // [n] or nullptr
};

// one chunk: pairs [lo, lo + cnt) of the call's n
int sweep_chunk(anx_model* m, const char* const* in, const anx::PairSpan* sa, const anx::PairSpan* sg, size_t lo, size_t cnt, size_t n, const Tail& t) {
  std::string err;
  anx::LearnVocab** vocab = anx::learn_vocab_slot(m);
  anx::SweepChunk* c = nullptr;
  if (int rc = anx::sweep_chunk_begin(anx_learn_host(m), anx_replica_of(m, 0), vocab, sa, sg, cnt, t.out != nullptr, &c, err)) return anx_fail(rc, err);
  struct End { anx::SweepChunk* c; ~End() { anx::sweep_chunk_end(c); } } end{c};
  anx::sweep_stats_add(anx::SWEEP_CHUNKS, 1);
  for (size_t s = 0; s < t.n_sets; ++s) {
    anx_eval_gather rows;  // (freed at the end of this round of the loop: one set's rows at a time)
    const int grc = anx_eval_gather_rows(m, in, sa, cnt, &t.sets[s], rows);
    anx::sweep_stats_add(anx::SWEEP_BATCH_RUNS, rows.batch_runs);
    if (grc) return grc;
    if (int rc = anx::sweep_chunk_set(c, t.sets[s], s == 0, rows.secs, rows.sec_rows, &t.summaries[s], t.out ? t.out + s * n + lo : nullptr, err))
      return anx_fail(rc, err);
    anx::sweep_stats_add(anx::SWEEP_SETS, 1);
  }
  if (t.pairs)
    if (int rc = anx::sweep_chunk_pairs(c, t.pairs + lo, err)) return anx_fail(rc, err);
  return ANX_OK;
}

int run_call(anx_model* m, const char* const* in, const std::vector<anx::PairSpan>& sa, const std::vector<anx::PairSpan>& sg, const Tail& t, size_t chunk) {
  const size_t n = sa.size();
  std::lock_guard<std::mutex> lk(anx_learn_mutex());
  anx::sweep_stats_add(anx::SWEEP_CALLS, 1);
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t cnt = std::min(chunk, n - lo);
    if (int rc = sweep_chunk(m, in ? in + lo : nullptr, sa.data() + lo, sg.data() + lo, lo, cnt, n, t)) return rc;
  }
  return ANX_OK;
}
// everything but the strings themselves; *run = false: the call is answered already (code in the return value)
int check_call(anx_model* m, const void* a, const void* g, size_t n, const Tail& t, bool* run) {
  *run = false;
  if (!m || !t.sets || !t.summaries) return anx_fail(ANX_EINVAL, "NULL argument");
  if (t.n_sets == 0 || t.n_sets > ANX_SWEEP_MAX_SETS) return anx_fail(ANX_EINVAL, "sweep: the number of parameter sets is outside 1 .. 256");
  memset(t.summaries, 0, t.n_sets * sizeof(anx_gold_summary));
  if (n == 0) return ANX_OK;
  if (!a || !g) return anx_fail(ANX_EINVAL, "NULL argument");
  if (!anx_learn_host(m).built) return anx_fail(ANX_ENOTBUILT, "Model has not been built yet! Call build() before evaluate_sweep()");
  if (anx_model_num_replicas(m) < 1 || !anx_replica_of(m, 0))
    return anx_fail(ANX_ENODEVICE, "model is not resident on a device (no HIP device / anx_model_to_device not called)");
  if (anx::switches().confusables_host && !anx_learn_host(m).confusables.empty())
    return anx_fail(ANX_EINVAL, "sweep: confusables are weighted on the host (ANX_CONFUSABLES=host): the ranked rows exist on the host only");
  *run = true;
  return ANX_OK;
}
int pointer_call(anx_model* m, const char* const* a, const char* const* g, size_t n, const Tail& t, size_t chunk) {
  bool run;
  if (int rc = check_call(m, a, g, n, t, &run); rc || !run) return rc;
  if (chunk < 1 || chunk > anx::PAIRS_CHUNK) return anx_fail(ANX_EINVAL, "sweep: chunk size outside 1 .. 2^20");
  std::vector<anx::PairSpan> sa, sg;
  if (!anx::spans_of_pointers(a, n, sa) || !anx::spans_of_pointers(g, n, sg)) return anx_fail(ANX_EINVAL, "NULL string");
  return run_call(m, a, sa, sg, t, chunk);
}
}  // namespace

extern "C" {
int anx_evaluate_sweep(anx_model* m, const char* const* inputs, const char* const* gold, size_t n, const anx_params* sets, size_t n_sets,
                       anx_gold_summary* summaries, anx_gold_eval* out, anx_pair_score* pairs) {
  return pointer_call(m, inputs, gold, n, Tail{sets, n_sets, summaries, out, pairs}, anx::PAIRS_CHUNK);
}
int anx_debug_evaluate_sweep_chunk(anx_model* m, const char* const* inputs, const char* const* gold, size_t n, const anx_params* sets, size_t n_sets,
                                   anx_gold_summary* summaries, anx_gold_eval* out, anx_pair_score* pairs, size_t chunk) {
  return pointer_call(m, inputs, gold, n, Tail{sets, n_sets, summaries, out, pairs}, chunk);
}
int anx_evaluate_sweep_packed(anx_model* m, const char* blob_in, size_t len_in, const char* blob_gold, size_t len_gold, size_t n, const anx_params* sets,
                              size_t n_sets, anx_gold_summary* summaries, anx_gold_eval* out, anx_pair_score* pairs) {
  const Tail t{sets, n_sets, summaries, out, pairs};
  bool run;
  if (int rc = check_call(m, blob_in, blob_gold, n, t, &run); rc || !run) return rc;
  if (len_in >= ((size_t)1 << 32) || len_gold >= ((size_t)1 << 32)) return anx_fail(ANX_ELIMIT, "packed pairs exceed 4 GB per blob: split the call");
  std::vector<anx::PairSpan> sa, sg;
  if (!anx::spans_of(blob_in, len_in, n, sa) || !anx::spans_of(blob_gold, len_gold, n, sg)) return anx_fail(ANX_EINVAL, "packed inputs hold fewer strings than announced");
  return run_call(m, nullptr, sa, sg, t, anx::PAIRS_CHUNK);  // (the spans lie back to back, each behind its NUL byte)
}
int anx_debug_sweep_stats(uint64_t* out, int n) {
  if (!out || n < 0) return anx_fail(ANX_EINVAL, "NULL argument");
  uint64_t all[anx::SWEEP_NSTATS];
  anx::sweep_stats(all);
  for (int i = 0; i < n && i < anx::SWEEP_NSTATS; ++i) out[i] = all[i];
  return ANX_OK;
}
}  // extern "C"
