// explain_capi.cpp -- anx_batch_fetch_measures: one anx_row_measures per ranked row of a batch that has run, in the order of
// anx_batch_fetch_compact_via.  The argument checks and the walk over the shards live here; every shard's records are computed on its
// own device (engine.hip batch_fetch_measures_into, kernels_explain.hpp) and land where the compact fetch puts the shard's rows:
// consecutive shards write straight into their slice of the call's block, the scattered shards of the length-partitioned split go
// through a block of their own and are copied to their inputs' places.  The batch is reached through the accessors capi.cpp defines
// for the exports.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "engine.h"
#include "host_model.h"

const anx::HostModel& anx_host_of(const anx_model* m);
const anx_model* anx_batch_model_of(const anx_batch* b);
bool anx_batch_host_rescored(const anx_batch* b);
size_t anx_export_num_shards(const anx_batch* b);
void anx_export_shard(const anx_batch* b, size_t g, void* caller_stream, const anx::DeviceLexicon** dl, anx::Batch** sb, void** stream);
int anx_fail(int code, const std::string& msg);

namespace {
struct ShardView {
  const anx::DeviceLexicon* dl = nullptr;
  anx::Batch* b = nullptr;
  size_t lo = 0, n = 0, rows = 0;
  const uint32_t* idx = nullptr;  // the shard's inputs (ascending), nullptr = the consecutive range [lo, lo + n)
};
}  // namespace

extern "C" {
int anx_batch_fetch_measures(const anx_batch* b, anx_row_measures** out_rows, uint32_t** out_offsets) {
  if (!b || !out_rows || !out_offsets) return anx_fail(ANX_EINVAL, "NULL argument");
  if (anx_batch_host_rescored(b))
    return anx_fail(ANX_EINVAL, "confusables are loaded: results are rescored on the host, the device rows are not the final rows");
  const anx::HostModel& m = anx_host_of(anx_batch_model_of(b));
  const size_t S = anx_export_num_shards(b);
  std::vector<ShardView> sh(S);
  size_t n = 0, total = 0;
  bool scattered = false;
  for (size_t g = 0; g < S; ++g) {
    ShardView& v = sh[g];
    void* st = nullptr;
    anx_export_shard(b, g, nullptr, &v.dl, &v.b, &st);
    if (int rc = anx_batch_shard_info(b, (int)g, nullptr, &v.lo, &v.n)) return rc;
    if (int rc = anx_batch_shard_inputs(b, (int)g, &v.idx)) return rc;
    if (!v.dl || !v.b) return anx_fail(ANX_ENODEVICE, "model is not resident on a device");
    v.rows = anx::batch_n_results(v.b);
    n += v.n;
    total += v.rows;
    scattered = scattered || v.idx;
  }
  if (total >= ((size_t)1 << 32)) return anx_fail(ANX_ELIMIT, "more than 2^32 result rows");
  // one pinned block [rows | offsets]: the rows rounded to 64 bytes, n + 2 offset words
  const size_t row_bytes = (std::max<size_t>(1, total) * sizeof(anx_row_measures) + 63) & ~(size_t)63;
  char* blk = static_cast<char*>(anx::host_result_alloc(row_bytes + (n + 2) * sizeof(uint32_t)));
  if (!blk) return anx_fail(ANX_EINVAL, "out of memory");
  anx_row_measures* rows = reinterpret_cast<anx_row_measures*>(blk);
  uint32_t* offs = reinterpret_cast<uint32_t*>(blk + row_bytes);
  std::string err;
  int rc = ANX_OK;
  if (!scattered) {
    // shard g's last offset is shard g + 1's first (the same value): the shards run one after the other, so the overlap is harmless
    size_t base = 0;
    for (size_t g = 0; g < S && rc == ANX_OK; ++g) {
      rc = anx::batch_fetch_measures_into(m, sh[g].dl, sh[g].b, rows + base, offs + sh[g].lo, (uint32_t)base, err);
      base += sh[g].rows;
    }
    if (rc == ANX_OK) offs[n] = (uint32_t)total;
  } else {
    std::vector<anx_row_measures*> part(S, nullptr);
    std::vector<std::vector<uint32_t>> loff(S);
    for (size_t g = 0; g < S && rc == ANX_OK; ++g) {
      part[g] = static_cast<anx_row_measures*>(anx::host_result_alloc(std::max<size_t>(1, sh[g].rows) * sizeof(anx_row_measures)));
      if (!part[g]) { err = "out of memory"; rc = ANX_EINVAL; break; }
      loff[g].assign(sh[g].n + 1, 0u);
      rc = anx::batch_fetch_measures_into(m, sh[g].dl, sh[g].b, part[g], loff[g].data(), 0u, err);
    }
    if (rc == ANX_OK) {
      auto input = [&](size_t g, size_t i) { return sh[g].idx ? (size_t)sh[g].idx[i] : sh[g].lo + i; };
      std::fill(offs, offs + n + 1, 0u);
      for (size_t g = 0; g < S; ++g)
        for (size_t i = 0; i < sh[g].n; ++i) offs[input(g, i) + 1] = loff[g][i + 1] - loff[g][i];
      for (size_t i = 0; i < n; ++i) offs[i + 1] += offs[i];
      for (size_t g = 0; g < S; ++g)
        for (size_t i = 0; i < sh[g].n; ++i) {
          const size_t c = loff[g][i + 1] - loff[g][i];
          if (c) memcpy(rows + offs[input(g, i)], part[g] + loff[g][i], c * sizeof(anx_row_measures));
        }
    }
    for (anx_row_measures* p : part) anx::host_result_free(p);
  }
  if (rc) { anx::host_result_free(blk); return anx_fail(rc, err); }
  *out_rows = rows;
  *out_offsets = offs;
  return ANX_OK;
}
void anx_measures_free(anx_row_measures* rows, uint32_t* offsets) {
  (void)offsets;  // one block: the offsets live behind the rows
  anx::host_result_free(rows);
}
}  // extern "C"
