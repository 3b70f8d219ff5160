// compact_via_capi.cpp -- compact records with `via`: anx_batch_fetch_compact_via, anx_compact_to_results_via, anx_pipeline_next_via.
// The 16-byte anx_topk_record keeps its layout; `via` (the vocabulary id of the variant a row was reached through, src/lib.rs:1677-1727)
// travels as a parallel uint32 array, UINT32_MAX = none, so models with variant lists get the compact fetch and the pipeline.
// The block layout, the shard layouts and the pipeline are capi.cpp's (anx_compact_fetch, anx_pipeline_take); this file brings the
// engine's fetch that writes the `via` words (anx::batch_fetch_compact_via_into) and installs it for the pipeline's fetch stage.  A
// translation unit of its own, as learn_capi.cpp: capi.cpp is also linked against a stub engine that has no such fetch.
#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "engine.h"
#include "host_model.h"

using anx_compact_via_into = int (*)(const anx::Batch*, anx_topk_record*, uint32_t*, uint32_t*, uint32_t, bool, std::string&);
int anx_compact_fetch(const anx_batch* b, anx_topk_record** rows, uint32_t** offs, uint32_t** via, anx_compact_via_into via_into);
int anx_pipeline_take(anx_pipeline* pl, anx_topk_record** rows, uint32_t** offs, uint32_t** via, size_t* n);
void anx_compact_via_install(anx_compact_via_into f);
int anx_fail(int code, const std::string& msg);

namespace {
struct Install { Install() { anx_compact_via_install(&anx::batch_fetch_compact_via_into); } } g_install;
}  // namespace

extern "C" {
int anx_batch_fetch_compact_via(const anx_batch* b, anx_topk_record** rows, uint32_t** offs, uint32_t** via) {
  if (!b || !rows || !offs || !via) return anx_fail(ANX_EINVAL, "NULL argument");
  return anx_compact_fetch(b, rows, offs, via, &anx::batch_fetch_compact_via_into);
}
void anx_compact_to_results_via(const anx_topk_record* rows, const uint32_t* via, size_t n_rows, anx_result* out) {
  if (!rows || !via || !out) return;
  auto work = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i)
      out[i] = anx_result{rows[i].vocab_id, rows[i].dist_score, (double)rows[i].freq_score, via[i] == 0xFFFFFFFFu ? ANX_NO_VIA : (uint64_t)via[i]};
  };
  const unsigned nthreads = n_rows < (1u << 16) ? 1u : std::max(1u, std::min(16u, anx::usable_hw_threads()));
  if (nthreads == 1) { work(0, n_rows); return; }
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nthreads; ++t) th.emplace_back(work, n_rows * t / nthreads, n_rows * (t + 1) / nthreads);
  for (auto& x : th) x.join();
}
int anx_pipeline_next_via(anx_pipeline* pl, anx_topk_record** rows, uint32_t** offs, uint32_t** via, size_t* n) {
  if (!pl || !rows || !offs || !via) return anx_fail(ANX_EINVAL, "NULL argument");
  return anx_pipeline_take(pl, rows, offs, via, n);
}
}  // extern "C"
