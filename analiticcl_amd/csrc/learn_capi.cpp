// learn_capi.cpp -- anx_learn_variants: strict learn mode (src/lib.rs:1029-1139) with the fold on the device.
// Every input goes through the batch pipeline (batches of at most ANX_MAX_BATCH inputs per replica); every shard's compact export is
// gathered onto replica 0's device (anx_batch_gather_compact: the shards of other replicas are copied there), learn.hip folds all of
// it, and HostModel::learn_apply appends the result.  The statistics, the host fold and the rebuild are capi.cpp's (shared with the
// non-strict mode and anx_learn_apply_rows).
#include <chrono>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "engine.h"
#include "host_model.h"
#include "pair_spans.h"

anx::HostModel& anx_learn_host(anx_model* m);
std::mutex& anx_learn_mutex();
uint64_t anx_learn_host_fold(anx_model* m, const char* const* text, size_t n, const anx_result* rows, const size_t* off, double* ms);
void anx_learn_count_device_fold(uint64_t rows, uint64_t refs);
int anx_learn_finish(anx_model* m, int auto_build, double* ms);
bool anx_batch_host_rescored(const anx_batch* b);
size_t anx_batch_rows(const anx_batch* b);
int anx_learn_fail(int code, const std::string& msg);
int anx_learn_check_rows(const anx_model* m, size_t n, const anx_result* rows, const size_t* off);
int anx_learn_code();

namespace {
using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// the inputs packed for the device fold (each followed by a NUL byte)
int pack_offsets(const char* const* utf8, size_t n, std::vector<uint32_t>& soff) {
  soff.assign(n + 1, 0);
  size_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!utf8[i]) return anx_learn_fail(ANX_EINVAL, "NULL input");
    total += strlen(utf8[i]) + 1;
    if (total >= 0xFFFFFFFFull) return anx_learn_fail(ANX_ELIMIT, "learn: more than 4 GB of input text in one call");
    soff[i + 1] = (uint32_t)total;
  }
  return ANX_OK;
}
std::vector<char> pack_blob(const char* const* utf8, size_t n, const std::vector<uint32_t>& soff) {
  std::vector<char> blob((size_t)soff[n] + 1, 0);
  for (size_t i = 0; i < n; ++i) memcpy(blob.data() + soff[i], utf8[i], soff[i + 1] - soff[i]);
  return blob;
}

// *host_rows: the rows exist only on the host (confusables weighted there): nothing was folded
int strict_device(anx_model* m, const char* const* utf8, size_t n, const anx_params* p, const std::vector<char>& blob,
                  const std::vector<uint32_t>& soff, anx::LearnFold& fold, bool* host_rows, size_t* n_rows, double* ms) {
  *host_rows = false;
  const int R = anx_model_num_replicas(m);
  const int dev0 = anx_model_replica_device(m, 0);
  const size_t per_round = (size_t)anx::switches().max_batch * (size_t)R;
  std::vector<void*> bufs;
  std::vector<anx::LearnSection> secs;
  std::deque<std::vector<uint32_t>> idx_store;
  size_t rows = 0;
  auto release = [&]() { for (void* b : bufs) anx::learn_device_free(dev0, b); };
  const auto t0 = Clock::now();
  for (size_t lo = 0; lo < n; lo += per_round) {
    const size_t cnt = std::min(per_round, n - lo);
    anx_batch* b = anx_batch_encode(m, utf8 + lo, cnt, p);
    if (!b) { release(); const int c = anx_learn_code(); return c ? c : ANX_EINVAL; }
    int rc = anx_batch_run(m, b, nullptr);
    if (rc == ANX_OK && anx_batch_host_rescored(b)) { *host_rows = true; anx_batch_free(b); release(); return ANX_OK; }
    size_t need = 0;
    void* buf = nullptr;
    if (rc == ANX_OK) {
      char probe = 0;  // capacity 0: the call only reports the bytes it needs (ANX_ELIMIT)
      (void)anx_batch_gather_compact(b, dev0, &probe, 0, nullptr, &need);
      if (!(buf = anx::learn_device_alloc(dev0, need))) rc = anx_learn_fail(ANX_ENODEVICE, "out of device memory for the learn gather");
      else bufs.push_back(buf);
    }
    const int S = anx_batch_num_shards(b);
    std::vector<size_t> so((size_t)S + 1, 0);
    size_t used = 0;
    if (rc == ANX_OK) rc = anx_batch_gather_compact(b, dev0, buf, need, so.data(), &used);
    for (int g = 0; g < S && rc == ANX_OK; ++g) {
      size_t first = 0, ns = 0;
      const uint32_t* idx = nullptr;
      rc = anx_batch_shard_info(b, g, nullptr, &first, &ns);
      if (rc == ANX_OK) rc = anx_batch_shard_inputs(b, g, &idx);
      if (rc) break;
      if (idx) {  // a length-partitioned shard: its inputs by index, made call-wide
        idx_store.emplace_back(idx, idx + ns);
        for (uint32_t& x : idx_store.back()) x += (uint32_t)lo;
        idx = idx_store.back().data();
      }
      secs.push_back(anx::LearnSection{static_cast<char*>(buf) + so[(size_t)g], ns, lo + first, idx});
    }
    if (rc == ANX_OK) rows += anx_batch_rows(b);
    anx_batch_free(b);
    if (rc) { release(); return rc; }
  }
  ms[0] = ms_since(t0);
  const auto t1 = Clock::now();
  std::string err;
  anx::LearnVocab** vocab = anx::learn_vocab_slot(m);
  const int rc = anx::learn_fold_device(anx_learn_host(m), dev0, vocab, blob.data(), soff.data(), n, secs, rows, fold, err);
  release();
  ms[1] = ms_since(t1);
  *n_rows = rows;
  return rc ? anx_learn_fail(rc, err) : ANX_OK;
}
}  // namespace

extern "C" {
int anx_learn_variants(anx_model* m, const char* const* utf8, size_t n, const anx_params* p, int auto_build, uint64_t* count) {
  if (!m || (!utf8 && n) || !p || !count) return anx_learn_fail(ANX_EINVAL, "NULL argument");
  if (anx_model_num_replicas(m) < 1)
    return anx_learn_fail(ANX_ENODEVICE, "model is not resident on a device (no HIP device / anx_model_to_device not called)");
  std::lock_guard<std::mutex> lk(anx_learn_mutex());
  anx::HostModel& host = anx_learn_host(m);
  double ms[6] = {0, 0, 0, 0, 0, 0};
  std::vector<uint32_t> soff;
  if (int rc = pack_offsets(utf8, n, soff)) return rc;
  uint64_t c = 0;
  bool host_rows = anx::switches().learn_fold_host;
  if (!host_rows) {
    const std::vector<char> blob = pack_blob(utf8, n, soff);
    anx::LearnFold fold;
    size_t rows = 0;
    if (int rc = strict_device(m, utf8, n, p, blob, soff, fold, &host_rows, &rows, ms)) return rc;
    if (!host_rows) {
      const auto t0 = Clock::now();
      const uint64_t before = host.learn_refs_added;
      std::string err;
      c = host.learn_apply(utf8, n, fold, err);
      if (c == UINT64_MAX) return anx_learn_fail(ANX_EINVAL, err);
      ms[3] = ms_since(t0);
      anx_learn_count_device_fold(rows, host.learn_refs_added - before);
    }
  }
  if (host_rows) {  // ANX_LEARN_FOLD=host, or confusables weighted on the host: the rows are on the host, the host fold applies them
    const auto t0 = Clock::now();
    anx_result* rows = nullptr;
    size_t* offs = nullptr;
    if (int rc = anx_find_variants_batch(m, utf8, n, p, &rows, &offs)) return rc;
    ms[0] = ms_since(t0);
    c = anx_learn_host_fold(m, utf8, n, rows, offs, &ms[2]);
    anx_results_free(rows, offs);
  }
  *count = c;
  return anx_learn_finish(m, auto_build, ms);
}

// Test hook: anx_learn_apply_rows' contract with the DEVICE fold.  The caller's rows are packed into n_sections compact export
// sections on replica 0's device, the layout strict_device gathers a batch's shards into: contiguous input ranges (section s holds the
// inputs [s n / S, (s + 1) n / S), empty when S > n), or with by_index index-listed sections that deal the inputs out round-robin
// (section s holds s, s + S, ...: neighbours land in different sections).  The fold and the apply are anx_learn_variants'.
int anx_debug_learn_fold_rows(anx_model* m, const char* const* utf8, size_t n, const anx_result* rows, const size_t* offsets, int n_sections,
                              int by_index, uint64_t* count) {
  if (!m || (!utf8 && n) || !offsets || (!rows && offsets[n]) || !count) return anx_learn_fail(ANX_EINVAL, "NULL argument");
  for (size_t i = 0; i < n; ++i)
    if (!utf8[i]) return anx_learn_fail(ANX_EINVAL, "NULL input");
  if (n_sections < 1) return anx_learn_fail(ANX_EINVAL, "at least one section");
  if (int rc = anx_learn_check_rows(m, n, rows, offsets)) return rc;
  if (anx_model_num_replicas(m) < 1)
    return anx_learn_fail(ANX_ENODEVICE, "model is not resident on a device (no HIP device / anx_model_to_device not called)");
  if (offsets[n] >= 0x7FFFFFFFull) return anx_learn_fail(ANX_ELIMIT, "learn fold: more than 2^31 rows");
  std::lock_guard<std::mutex> lk(anx_learn_mutex());
  anx::HostModel& host = anx_learn_host(m);
  std::vector<uint32_t> soff;
  if (int rc = pack_offsets(utf8, n, soff)) return rc;
  const std::vector<char> blob = pack_blob(utf8, n, soff);
  const int dev0 = anx_model_replica_device(m, 0);
  const size_t S = (size_t)n_sections;
  std::vector<void*> bufs;
  std::vector<anx::LearnSection> secs;
  std::deque<std::vector<uint32_t>> idx_store;
  auto release = [&]() { for (void* b : bufs) anx::learn_device_free(dev0, b); };
  std::vector<char> img;
  for (size_t s = 0; s < S; ++s) {
    std::vector<uint32_t> members;
    size_t lo = 0;
    if (by_index) {
      for (size_t i = s; i < n; i += S) members.push_back((uint32_t)i);
    } else {
      lo = s * n / S;
      for (size_t i = lo; i < (s + 1) * n / S; ++i) members.push_back((uint32_t)i);
    }
    const size_t ns = members.size();
    const size_t off_bytes = ((ns + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
    size_t nr = 0;
    for (uint32_t i : members) nr += offsets[i + 1] - offsets[i];
    img.assign(off_bytes + nr * sizeof(anx_topk_record), 0);
    uint32_t* so = reinterpret_cast<uint32_t*>(img.data());
    anx_topk_record* rec = reinterpret_cast<anx_topk_record*>(img.data() + off_bytes);
    size_t k = 0;
    for (size_t j = 0; j < ns; ++j) {
      so[j] = (uint32_t)k;
      for (size_t r = offsets[members[j]]; r < offsets[members[j] + 1]; ++r, ++k) {
        rec[k].vocab_id = (uint32_t)rows[r].vocab_id;
        rec[k].freq_score = (float)rows[r].freq_score;
        rec[k].dist_score = rows[r].dist_score;
      }
    }
    so[ns] = (uint32_t)k;
    void* buf = anx::learn_device_alloc(dev0, img.size());
    if (!buf) { release(); return anx_learn_fail(ANX_ENODEVICE, "out of device memory for the learn sections"); }
    bufs.push_back(buf);
    if (!anx::learn_device_upload(dev0, buf, img.data(), img.size())) { release(); return anx_learn_fail(ANX_ENODEVICE, "upload of a learn section failed"); }
    const uint32_t* idx = nullptr;
    if (by_index) {
      idx_store.push_back(std::move(members));
      idx = idx_store.back().data();
    }
    secs.push_back(anx::LearnSection{buf, ns, lo, idx});
  }
  std::string err;
  anx::LearnFold fold;
  anx::LearnVocab** vocab = anx::learn_vocab_slot(m);
  const int rc = anx::learn_fold_device(host, dev0, vocab, blob.data(), soff.data(), n, secs, offsets[n], fold, err);
  release();
  if (rc) return anx_learn_fail(rc, err);
  const uint64_t before = host.learn_refs_added;
  const uint64_t c = host.learn_apply(utf8, n, fold, err);
  if (c == UINT64_MAX) return anx_learn_fail(ANX_EINVAL, err);
  anx_learn_count_device_fold(offsets[n], host.learn_refs_added - before);
  *count = c;
  return ANX_OK;
}
}  // extern "C"
