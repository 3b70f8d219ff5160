// eval_capi.cpp -- anx_evaluate_gold / anx_evaluate_gold_packed: per (input, gold) pair, where the gold answer ended up in the ranked rows
// of find_variants(input, P) and, if nowhere, which stage of the reference's pipeline lost it (the ANX_GOLD_* reasons).
// The argument checks and the chunking live here.  A call of any size is cut into chunks of at most 2^20 pairs (anx::PAIRS_CHUNK, as
// anx_score_pairs); per chunk the inputs go through the batch pipeline (batches of at most ANX_MAX_BATCH inputs per replica, as learn
// mode runs them: never the small call), every shard's compact export is gathered onto replica 0's device
// (anx_batch_gather_compact_via) and eval.hip joins the rows with the pair measures there.  The model is reached through the accessors
// capi.cpp defines for learn mode and the exports; the vocabulary table is learn mode's, under its lock.
#include <algorithm>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "engine.h"
#include "eval_gather.h"
#include "host_model.h"
#include "pair_spans.h"

anx::HostModel& anx_learn_host(anx_model* m);
const anx::DeviceLexicon* anx_replica_of(const anx_model* m, size_t i);
std::mutex& anx_learn_mutex();
bool anx_batch_host_rescored(const anx_batch* b);
size_t anx_export_num_shards(const anx_batch* b);
void anx_export_shard(const anx_batch* b, size_t g, void* caller_stream, const anx::DeviceLexicon** dl, anx::Batch** sb, void** stream);
int anx_fail(int code, const std::string& msg);
int anx_learn_code();
namespace anx {
int batch_gather_measures(const HostModel& m, const DeviceLexicon* dl, const Batch* b, int dst_device, void* dst, size_t capacity, void* stream, std::string& err);  // engine.hip
}

// the ranked rows of the chunk's inputs as sections on replica 0's device (inputs relative to the chunk): eval_gather.h
int anx_eval_gather_rows(anx_model* m, const char* const* in, const anx::PairSpan* sa, size_t n, const anx_params* p, anx_eval_gather& out) {
  const int R = anx_model_num_replicas(m);
  const int dev0 = out.dev0 = anx_model_replica_device(m, 0);
  const size_t per_round = std::max<size_t>(1, (size_t)anx::switches().max_batch * (size_t)R);
  std::vector<void*>& bufs = out.bufs;
  std::vector<anx::LearnSection>& secs = out.secs;
  std::vector<size_t>& sec_rows = out.sec_rows;
  std::deque<std::vector<uint32_t>>& idx_store = out.idx_store;
  for (size_t lo = 0; lo < n; lo += per_round) {
    const size_t cnt = std::min(per_round, n - lo);
    anx_batch* b = in ? anx_batch_encode(m, in + lo, cnt, p)
                      : anx_batch_encode_packed(m, sa[lo].p, (size_t)(sa[lo + cnt - 1].p + sa[lo + cnt - 1].len + 1 - sa[lo].p), cnt, p);
    if (!b) { const int c = anx_learn_code(); return c ? c : ANX_EINVAL; }
    int rc = anx_batch_run(m, b, nullptr);
    ++out.batch_runs;
    if (rc == ANX_OK && anx_batch_host_rescored(b)) {
      anx_batch_free(b);
      return anx_fail(ANX_EINVAL, "evaluate: confusables are weighted on the host for this model: its ranked rows exist on the host only");
    }
    size_t need = 0;
    void* buf = nullptr;
    if (rc == ANX_OK) {
      char probe = 0;  // capacity 0: the call only reports the bytes it needs (ANX_ELIMIT)
      (void)anx_batch_gather_compact_via(b, dev0, &probe, 0, nullptr, &need);
      if (!(buf = anx::eval_device_alloc(dev0, need))) rc = anx_fail(ANX_ENODEVICE, "out of device memory for the evaluate gather");
      else bufs.push_back(buf);
    }
    const int S = anx_batch_num_shards(b);
    std::vector<size_t> so((size_t)S + 1, 0);
    size_t used = 0;
    if (rc == ANX_OK) rc = anx_batch_gather_compact_via(b, dev0, buf, need, so.data(), &used);
    for (int g = 0; g < S && rc == ANX_OK; ++g) {
      size_t first = 0, ns = 0;
      const uint32_t* idx = nullptr;
      rc = anx_batch_shard_info(b, g, nullptr, &first, &ns);
      if (rc == ANX_OK) rc = anx_batch_shard_inputs(b, g, &idx);
      if (rc) break;
      if (idx) {  // a length-partitioned shard: its inputs by index, made chunk-wide
        idx_store.emplace_back(idx, idx + ns);
        for (uint32_t& x : idx_store.back()) x += (uint32_t)lo;
        idx = idx_store.back().data();
      }
      const anx::DeviceLexicon* sdl = nullptr;
      anx::Batch* sb = nullptr;
      void* sst = nullptr;
      anx_export_shard(b, (size_t)g, nullptr, &sdl, &sb, &sst);
      const size_t rows = sb ? anx::batch_n_results(sb) : 0;
      const size_t off_bytes = ((ns + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
      if (so[(size_t)g] + off_bytes + rows * (sizeof(anx_topk_record) + sizeof(uint32_t)) > so[(size_t)g + 1]) {  // (every record lies inside the shard's part of the buffer)
        rc = anx_fail(ANX_EINVAL, "evaluate: a gathered section is smaller than its rows");
        break;
      }
      if (out.want_measures) {  // the measures behind the section's records, computed on the shard's replica and placed beside them
        void* mb = anx::eval_device_alloc(dev0, std::max<size_t>(rows, 1) * sizeof(anx_row_measures));
        if (!mb) { rc = anx_fail(ANX_ENODEVICE, "out of device memory for the evaluate gather"); break; }
        bufs.push_back(mb);
        std::string err;
        if (rows && sb)
          if (const int mrc = anx::batch_gather_measures(anx_learn_host(m), sdl, sb, dev0, mb, rows * sizeof(anx_row_measures), sst, err)) { rc = anx_fail(mrc, err); break; }
        out.sec_meas.push_back(static_cast<const anx_row_measures*>(mb));
      }
      secs.push_back(anx::LearnSection{static_cast<char*>(buf) + so[(size_t)g], ns, lo + first, idx});
      sec_rows.push_back(rows);
    }
    anx_batch_free(b);
    if (rc) return rc;
  }
  return ANX_OK;
}

namespace {
int evaluate_chunk(anx_model* m, const char* const* in, const anx::PairSpan* sa, const anx::PairSpan* sg, size_t n, const anx_params* p, anx_gold_eval* out,
                   anx_pair_score* pairs) {
  anx_eval_gather rows;
  if (int rc = anx_eval_gather_rows(m, in, sa, n, p, rows)) return rc;
  std::string err;
  anx::LearnVocab** vocab = anx::learn_vocab_slot(m);
  const int rc = anx::evaluate_chunk(anx_learn_host(m), anx_replica_of(m, 0), vocab, sa, sg, n, *p, rows.secs, rows.sec_rows, out, pairs, err);
  return rc ? anx_fail(rc, err) : ANX_OK;
}

int run_call(anx_model* m, const char* const* in, const std::vector<anx::PairSpan>& sa, const std::vector<anx::PairSpan>& sg, const anx_params* p,
             anx_gold_eval* out, anx_pair_score* pairs, size_t chunk) {
  const size_t n = sa.size();
  std::lock_guard<std::mutex> lk(anx_learn_mutex());
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t cnt = std::min(chunk, n - lo);
    if (int rc = evaluate_chunk(m, in ? in + lo : nullptr, sa.data() + lo, sg.data() + lo, cnt, p, out + lo, pairs ? pairs + lo : nullptr)) return rc;
  }
  return ANX_OK;
}
// everything but the strings themselves; *run = false: the call is answered already (code in the return value)
int check_call(anx_model* m, const void* a, const void* g, size_t n, const anx_params* p, const anx_gold_eval* out, bool* run) {
  *run = false;
  if (!m || !p) return anx_fail(ANX_EINVAL, "NULL argument");
  if (n == 0) return ANX_OK;
  if (!a || !g || !out) return anx_fail(ANX_EINVAL, "NULL argument");
  if (!anx_learn_host(m).built) return anx_fail(ANX_ENOTBUILT, "Model has not been built yet! Call build() before evaluate()");
  if (anx_model_num_replicas(m) < 1 || !anx_replica_of(m, 0))
    return anx_fail(ANX_ENODEVICE, "model is not resident on a device (no HIP device / anx_model_to_device not called)");
  if (anx::switches().confusables_host && !anx_learn_host(m).confusables.empty())
    return anx_fail(ANX_EINVAL, "evaluate: confusables are weighted on the host (ANX_CONFUSABLES=host): the ranked rows exist on the host only");
  *run = true;
  return ANX_OK;
}
int pointer_call(anx_model* m, const char* const* a, const char* const* g, size_t n, const anx_params* p, anx_gold_eval* out, anx_pair_score* pairs, size_t chunk) {
  bool run;
  if (int rc = check_call(m, a, g, n, p, out, &run); rc || !run) return rc;
  if (chunk < 1 || chunk > anx::PAIRS_CHUNK) return anx_fail(ANX_EINVAL, "evaluate: chunk size outside 1 .. 2^20");
  std::vector<anx::PairSpan> sa, sg;
  if (!anx::spans_of_pointers(a, n, sa) || !anx::spans_of_pointers(g, n, sg)) return anx_fail(ANX_EINVAL, "NULL string");
  return run_call(m, a, sa, sg, p, out, pairs, chunk);
}
}  // namespace

extern "C" {
int anx_evaluate_gold(anx_model* m, const char* const* inputs, const char* const* gold, size_t n, const anx_params* p, anx_gold_eval* out,
                      anx_pair_score* pairs) {
  return pointer_call(m, inputs, gold, n, p, out, pairs, anx::PAIRS_CHUNK);
}
int anx_debug_evaluate_gold_chunk(anx_model* m, const char* const* inputs, const char* const* gold, size_t n, const anx_params* p, anx_gold_eval* out,
                                  anx_pair_score* pairs, size_t chunk) {
  return pointer_call(m, inputs, gold, n, p, out, pairs, chunk);
}
int anx_evaluate_gold_packed(anx_model* m, const char* blob_in, size_t len_in, const char* blob_gold, size_t len_gold, size_t n, const anx_params* p,
                             anx_gold_eval* out, anx_pair_score* pairs) {
  bool run;
  if (int rc = check_call(m, blob_in, blob_gold, n, p, out, &run); rc || !run) return rc;
  if (len_in >= ((size_t)1 << 32) || len_gold >= ((size_t)1 << 32)) return anx_fail(ANX_ELIMIT, "packed pairs exceed 4 GB per blob: split the call");
  std::vector<anx::PairSpan> sa, sg;
  if (!anx::spans_of(blob_in, len_in, n, sa) || !anx::spans_of(blob_gold, len_gold, n, sg)) return anx_fail(ANX_EINVAL, "packed inputs hold fewer strings than announced");
  return run_call(m, nullptr, sa, sg, p, out, pairs, anx::PAIRS_CHUNK);  // (the spans lie back to back, each behind its NUL byte)
}
}  // extern "C"
