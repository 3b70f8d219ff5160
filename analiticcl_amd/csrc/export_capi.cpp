// export_capi.cpp -- the device-side exports with `via`: anx_batch_export_compact_via, anx_batch_gather_compact_via, anx_batch_export_topk_via.
// The via-less exports (capi.cpp) write 16-byte anx_topk_record rows, which have no room for the vocabulary id of the variant a row was
// reached through; these calls add it as a parallel array of one word per row (UINT32_MAX = none), for every model, and leave offsets and
// records byte-equal to what the via-less calls write.  The argument checks are those of capi.cpp's calls; the batch and the model are
// reached through the accessors capi.cpp defines.
#include <functional>
#include <string>
#include <vector>

#include "engine.h"
#include "host_model.h"

size_t anx_export_num_shards(const anx_batch* b);
void anx_export_shard(const anx_batch* b, size_t g, void* caller_stream, const anx::DeviceLexicon** dl, anx::Batch** sb, void** stream);
int anx_export_on_shards(const anx_batch* b, const std::function<int(size_t, std::string&)>& fn);
bool anx_batch_host_rescored(const anx_batch* b);
int anx_fail(int code, const std::string& msg);

namespace {
struct ShardRef {
  const anx::DeviceLexicon* dl = nullptr;
  anx::Batch* b = nullptr;
  void* stream = nullptr;
};
ShardRef shard_of(const anx_batch* b, size_t g, void* caller_stream) {
  ShardRef s;
  anx_export_shard(b, g, caller_stream, &s.dl, &s.b, &s.stream);
  return s;
}
// the checks of anx_batch_export_topk / _compact: a finished device-ranked batch on ONE replica
int check_export(const anx_batch* b) {
  if (!b) return anx_fail(ANX_EINVAL, "NULL batch");
  if (anx_batch_host_rescored(b)) return anx_fail(ANX_EINVAL, "confusables are loaded: results are rescored on the host, use anx_batch_fetch");
  if (anx_export_num_shards(b) != 1) return anx_fail(ANX_EINVAL, "the batch is spread over several replicas: export one shard at a time (anx_batch_shard_*)");
  return ANX_OK;
}
}  // namespace

extern "C" {
int anx_debug_exclusive_scan(int device, const uint32_t* in, size_t n, uint32_t* out, uint32_t* copy) {
  if (!out || (!in && n)) return anx_fail(ANX_EINVAL, "NULL argument");
  std::string err;
  const int rc = anx::debug_exclusive_scan(device, in, n, out, copy, err);
  return rc ? anx_fail(rc, err) : ANX_OK;
}
int anx_debug_rank_rows(int device, size_t nq, const uint32_t* counts, const uint32_t* maxfreq, const uint32_t* qexpand, const double* score,
                        const uint32_t* order, const uint32_t* position, const uint32_t* vocab, const uint32_t* freq, const uint32_t* via,
                        double cutoff_threshold, uint64_t max_matches, float freq_weight, int have_freq, int any_variants, uint32_t seg_cap,
                        uint32_t row_cap, uint32_t overflow, uint32_t* out_count, void* out_rows) {
  if (nq && (!counts || !maxfreq || !qexpand || !out_count)) return anx_fail(ANX_EINVAL, "NULL argument");
  size_t total = 0;
  for (size_t q = 0; q < nq; ++q) total += counts[q];
  if (total && (!score || !order || !position || !vocab || !freq || !out_rows)) return anx_fail(ANX_EINVAL, "NULL argument");
  const anx::DebugRankIn in{nq, counts, maxfreq, qexpand, score, order, position, vocab, freq, via, cutoff_threshold, max_matches, freq_weight,
                            have_freq ? 1 : 0, any_variants ? 1 : 0, seg_cap, row_cap, overflow};
  std::string err;
  const int rc = anx::debug_rank_rows(device, in, out_count, out_rows, err);
  return rc ? anx_fail(rc, err) : ANX_OK;
}
int anx_batch_export_topk_via(const anx_batch* b, void* dst, void* via, uint32_t stride, void* stream) {
  if (int rc = check_export(b)) return rc;
  const ShardRef s = shard_of(b, 0, stream);
  if (!s.b) return anx_fail(ANX_EINVAL, "batch has not been run");
  std::string err;
  const int rc = anx::batch_export_topk_via(s.dl, s.b, dst, via, stride, stream, err);
  return rc ? anx_fail(rc, err) : ANX_OK;
}
int anx_batch_export_compact_via(const anx_batch* b, void* dst, size_t capacity, void* stream, size_t* used) {
  if (!used) return anx_fail(ANX_EINVAL, "NULL argument");
  if (int rc = check_export(b)) return rc;
  const ShardRef s = shard_of(b, 0, stream);
  if (!s.b) return anx_fail(ANX_EINVAL, "batch has not been run");
  std::string err;
  const int rc = anx::batch_export_compact_via(s.dl, s.b, dst, capacity, stream, used, err);
  return rc ? anx_fail(rc, err) : ANX_OK;
}
int anx_batch_gather_compact_via(const anx_batch* b, int dst_device, void* device_dst, size_t capacity, size_t* shard_offsets, size_t* used) {
  if (!b || !device_dst || !used) return anx_fail(ANX_EINVAL, "NULL argument");
  if (anx_batch_host_rescored(b)) return anx_fail(ANX_EINVAL, "host-rescored confusable batches have no device-side export: anx_batch_fetch");
  const size_t S = anx_export_num_shards(b);
  std::vector<ShardRef> sh(S);
  std::vector<size_t> off(S + 1, 0);
  for (size_t g = 0; g < S; ++g) {
    sh[g] = shard_of(b, g, nullptr);
    if (!sh[g].b) return anx_fail(ANX_EINVAL, "batch has not been run");
    off[g + 1] = off[g] + ((anx::batch_compact_via_bytes(sh[g].b) + 255) & ~(size_t)255);
  }
  *used = off[S];
  if (shard_offsets) for (size_t g = 0; g <= S; ++g) shard_offsets[g] = off[g];
  if (capacity < off[S]) return anx_fail(ANX_ELIMIT, "gather buffer too small: " + std::to_string(off[S]) + " bytes needed");
  // every shard from its replica's own thread and stream, as anx_batch_gather_compact
  char* dst = static_cast<char*>(device_dst);
  return anx_export_on_shards(b, [&](size_t g, std::string& err) {
    return anx::batch_gather_compact_via(sh[g].dl, sh[g].b, dst_device, dst + off[g], off[g + 1] - off[g], sh[g].stream, err);
  });
}
}  // extern "C"
