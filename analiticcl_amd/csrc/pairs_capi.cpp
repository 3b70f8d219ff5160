// pairs_capi.cpp -- anx_score_pairs / anx_score_pairs_packed (and their _weighted twins): the model's measures for caller-chosen string pairs.
// The reference has them as public functions on two normalised strings (src/distance.rs:101-231: damerau_levenshtein,
// longest_common_substring_length, common_prefix_length, common_suffix_length) and computes the score inside score_and_rank
// (src/lib.rs:1433-1452); here both sides go through the device normaliser and pairs.hip computes every measure and the score.
// The argument checks and the chunking live here; the model is reached through the accessors capi.cpp defines.  A call of any size is
// cut into chunks of at most 2^20 pairs (anx::PAIRS_CHUNK), so the working memory is bounded; a multi-device model runs the call on its
// first replica.  Nothing here is shared between calls: concurrent callers each take their own stream and pool blocks.
// The _weighted twins add compute_confusable_weight(a, b) (src/lib.rs:1733-1756) per pair, which the reference multiplies into every
// ranked row's dist_score (src/lib.rs:1656-1663); anx_model_confusable_weight_text is the same number from the host alone.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "engine.h"
#include "host_model.h"
#include "pair_spans.h"

const anx::HostModel& anx_host_of(const anx_model* m);
const anx::DeviceLexicon* anx_replica_of(const anx_model* m, size_t i);
int anx_fail(int code, const std::string& msg);

namespace {
// everything but the strings themselves; *run = false: the call is answered already (code in the return value)
int check_call(const anx_model* m, const void* a, const void* b, size_t n, const anx_pair_score* out, bool* run, bool weighted = false,
               const double* weight = nullptr) {
  *run = false;
  if (!m) return anx_fail(ANX_EINVAL, "NULL argument");
  if (n == 0) return ANX_OK;
  if (!a || !b || !out || (weighted && !weight)) return anx_fail(ANX_EINVAL, "NULL argument");
  if (!anx_host_of(m).built) return anx_fail(ANX_ENOTBUILT, "Model has not been built yet! Call build() before score_pairs()");
  if (!anx_replica_of(m, 0)) return anx_fail(ANX_ENODEVICE, "model is not resident on a device (no HIP device / anx_model_to_device not called)");
  *run = true;
  return ANX_OK;
}
int run_chunks(const anx_model* m, const std::vector<anx::PairSpan>& a, const std::vector<anx::PairSpan>& b, anx_pair_score* out, double* weight = nullptr) {
  const size_t n = a.size();
  for (size_t lo = 0; lo < n; lo += anx::PAIRS_CHUNK) {
    const size_t cnt = std::min(anx::PAIRS_CHUNK, n - lo);
    std::string err;
    const int rc = anx::score_pairs_chunk(anx_host_of(m), anx_replica_of(m, 0), a.data() + lo, b.data() + lo, cnt, out + lo, err, weight ? weight + lo : nullptr);
    if (rc) return anx_fail(rc, err);
  }
  return ANX_OK;
}
int pointer_call(const anx_model* m, const char* const* a, const char* const* b, size_t n, anx_pair_score* out, double* weight) {
  std::vector<anx::PairSpan> sa, sb;
  if (!anx::spans_of_pointers(a, n, sa) || !anx::spans_of_pointers(b, n, sb)) return anx_fail(ANX_EINVAL, "NULL string");
  return run_chunks(m, sa, sb, out, weight);
}
int packed_call(const anx_model* m, const char* blob_a, size_t len_a, const char* blob_b, size_t len_b, size_t n, anx_pair_score* out, double* weight) {
  if (len_a >= ((size_t)1 << 32) || len_b >= ((size_t)1 << 32)) return anx_fail(ANX_ELIMIT, "packed pairs exceed 4 GB per blob: split the call");
  std::vector<anx::PairSpan> sa, sb;
  if (!anx::spans_of(blob_a, len_a, n, sa) || !anx::spans_of(blob_b, len_b, n, sb)) return anx_fail(ANX_EINVAL, "packed inputs hold fewer strings than announced");
  return run_chunks(m, sa, sb, out, weight);
}
}  // namespace

extern "C" {
int anx_score_pairs(const anx_model* m, const char* const* a, const char* const* b, size_t n, anx_pair_score* out) {
  bool run;
  if (int rc = check_call(m, a, b, n, out, &run); rc || !run) return rc;
  return pointer_call(m, a, b, n, out, nullptr);
}
int anx_score_pairs_packed(const anx_model* m, const char* blob_a, size_t len_a, const char* blob_b, size_t len_b, size_t n, anx_pair_score* out) {
  bool run;
  if (int rc = check_call(m, blob_a, blob_b, n, out, &run); rc || !run) return rc;
  return packed_call(m, blob_a, len_a, blob_b, len_b, n, out, nullptr);
}
int anx_score_pairs_weighted(const anx_model* m, const char* const* a, const char* const* b, size_t n, anx_pair_score* out, double* weight) {
  bool run;
  if (int rc = check_call(m, a, b, n, out, &run, true, weight); rc || !run) return rc;
  return pointer_call(m, a, b, n, out, weight);
}
int anx_score_pairs_weighted_packed(const anx_model* m, const char* blob_a, size_t len_a, const char* blob_b, size_t len_b, size_t n, anx_pair_score* out,
                                    double* weight) {
  bool run;
  if (int rc = check_call(m, blob_a, blob_b, n, out, &run, true, weight); rc || !run) return rc;
  return packed_call(m, blob_a, len_a, blob_b, len_b, n, out, weight);
}
int anx_model_confusable_weight_text(const anx_model* m, const char* a, const char* b, double* out) {
  if (!m || !a || !b || !out) return anx_fail(ANX_EINVAL, "NULL argument");
  *out = anx_host_of(m).confusable_weight_text(a, strlen(a), b, strlen(b));
  return ANX_OK;
}
int anx_debug_pairs_conf_stats(uint64_t* out) {
  if (!out) return anx_fail(ANX_EINVAL, "NULL argument");
  anx::pairs_conf_stats(out);
  return ANX_OK;
}
}  // extern "C"
