// results.hip -- the way of a finished run's ranked rows off the device: the fetches into host memory (rows, compact records, the
// measures behind the rows), the exports into the caller's device memory (fixed stride, compact) and the gather of a shard's compact
// section onto another device.  Its kernels: the row emitters (kernels_fetch.hpp) and the explain kernels (kernels_explain.hpp); the
// prefix sum over the counts is engine.hip's (prefix_scan_enqueue).  Nothing here runs the pipeline: that, and k_rank, stay in engine.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "engine_internal.h"

namespace anx {

#include "kernels_common.hpp"
#include "kernels_fetch.hpp"
#include "kernels_explain.hpp"

// The temporaries of one call on stream st: pool blocks that return to the pool when the call ends -- after a wait for st unless the
// call has drained it itself (finish), since nothing of the call may still be in flight when another batch / thread takes the blocks.
namespace {
struct CallBlocks {
  PoolBlocks blocks;
  hipStream_t st;
  bool drained = false;
  explicit CallBlocks(hipStream_t s) : st(s) {}
  template <typename T>
  int get(T** p, size_t count, std::string& err) { return blocks.get(p, count, err); }
  int finish(std::string& err) {  // the call's last wait
    HIP_TRY(hipStreamSynchronize(st));
    drained = true;
    return ANX_OK;
  }
  void keep() { blocks.v.clear(); }  // the blocks outlive the call (their owner frees them)
  ~CallBlocks() {
    if (!drained) (void)hipStreamSynchronize(st);
    blocks.release();
  }
};
// what the offsets of the rows in the CALLER's input order take: cnt[n_input], off[n_input + 1], tmp: the scan's block sums
struct RowOffsets {
  uint32_t *cnt = nullptr, *off = nullptr, *tmp = nullptr;
  int get(CallBlocks& cb, size_t n, std::string& err) {
    int rc;
    if ((rc = cb.get(&cnt, n, err)) || (rc = cb.get(&off, n + 1, err)) || (rc = cb.get(&tmp, prefix_scan_tmp_bytes(n) / sizeof(uint32_t), err))) return rc;
    return ANX_OK;
  }
};
}  // namespace

// The way of the ranked rows into the CALLER's input order, enqueued on st -- what every fetch and the compact export share: the
// counts scattered to the original indices (d_cnt[n_input]) and an exclusive scan over them (d_off[n_input + 1]; d_tmp: the scan's
// block sums, prefix_scan_tmp_bytes) -- enqueue_offsets -- then the row copy through `emit` (kernels_fetch.hpp) to where the offsets say.
static int enqueue_offsets(const Batch* b, uint32_t* d_cnt, uint32_t* d_off, uint32_t* d_tmp, hipStream_t st, std::string& err) {
  const uint32_t n32 = (uint32_t)b->n_input, nq32 = (uint32_t)b->nq;
  HIP_TRY(hipMemsetAsync(d_cnt, 0, n32 * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_fetch_counts, dim3((nq32 + 255) / 256), dim3(256), 0, st, nq32, b->r_count, b->q_orig, d_cnt);
  prefix_scan_enqueue(d_cnt, n32, d_off, d_tmp, st, nullptr);
  return ANX_OK;
}
template <typename Emit>
static int enqueue_rows(const Batch* b, uint32_t* d_cnt, uint32_t* d_off, uint32_t* d_tmp, hipStream_t st, const Emit& emit, std::string& err) {
  if (const int rc = enqueue_offsets(b, d_cnt, d_off, d_tmp, st, err)) return rc;
  const uint32_t nq32 = (uint32_t)b->nq;
  hipLaunchKernelGGL(k_emit_rows<Emit>, dim3((nq32 + 255) / 256), dim3(256), 0, st, nq32, b->soff, b->r_count, b->r_rows, b->q_orig, d_off, emit);
  return ANX_OK;
}

// Downloads the ranked rows of the batch into caller-provided storage: out[0 .. n_results), off[0 .. n_input] = base + the CSR
// offsets (a shard of a multi-device batch writes its slice of the whole call's arrays) and, where via is given, via[0 .. n_results).
// The device lays the rows out in input order (enqueue_rows with make_emit(d_out, d_via)), so the host only copies: the offsets
// (u32) and the finished arrays.  Runs on the stream of the batch's last run.
template <typename Row, typename Off, typename MakeEmit>
static int fetch_rows(const Batch* b, Row* out, Off* off, uint32_t* via, Off base, const MakeEmit& make_emit, std::string& err) {
  if (!b->ran) { err = "batch has not been run"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(b->device));
  const size_t n = b->n_input;
  if (!b->nq || !b->n_results) {
    for (size_t i = 0; i <= n; ++i) off[i] = base;
    return ANX_OK;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(b->last_stream);
  CallBlocks tmp(st);
  RowOffsets ro;
  Row* d_out = nullptr;
  uint32_t* d_via = nullptr;
  int rc;
  if ((rc = ro.get(tmp, n, err)) || (rc = tmp.get(&d_out, b->n_results, err)) || (via && (rc = tmp.get(&d_via, b->n_results, err)))) return rc;
  if ((rc = enqueue_rows(b, ro.cnt, ro.off, ro.tmp, st, make_emit(d_out, d_via), err))) return rc;
  std::vector<uint32_t> staged;  // u32 offsets land in the caller's array, wider ones are widened from a copy
  uint32_t* h_off;
  if constexpr (sizeof(Off) == sizeof(uint32_t)) h_off = off;
  else { staged.resize(n + 1); h_off = staged.data(); }
  HIP_TRY(hipMemcpyAsync(h_off, ro.off, (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(out, d_out, b->n_results * sizeof(Row), hipMemcpyDeviceToHost, st));
  if (via) HIP_TRY(hipMemcpyAsync(via, d_via, b->n_results * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if ((rc = tmp.finish(err))) return rc;
  if (base || !staged.empty())
    for (size_t i = 0; i <= n; ++i) off[i] = base + h_off[i];
  return ANX_OK;
}

int batch_fetch_into(const Batch* b, anx_result* out, size_t* off, size_t base, std::string& err) {
  return fetch_rows(b, out, off, nullptr, base, [](anx_result* d_out, uint32_t*) { return EmitResult{d_out}; }, err);
}

// The same rows as 16-byte anx_topk_record {vocab u32, freq f32, dist f64} with u32 offsets: half the bytes over PCIe (config 2:
// 70 MB instead of 141 MB per million queries).  via (may be null): one word per row, 0xFFFFFFFF = none.  plain: the model has no
// variant lists -- every word is 0xFFFFFFFF, written on the host: the device and PCIe see what the call without via does.
int batch_fetch_compact_into(const Batch* b, anx_topk_record* out, uint32_t* off, uint32_t* via, uint32_t base, bool plain, std::string& err) {
  if (via && !plain)
    return fetch_rows(b, out, off, via, base, [](anx_topk_record* d_out, uint32_t* d_via) { return EmitRecordVia{d_out, d_via}; }, err);
  const int rc = fetch_rows(b, out, off, nullptr, base, [](anx_topk_record* d_out, uint32_t*) { return EmitRecord{d_out}; }, err);
  if (rc == ANX_OK && via && b->n_results) memset(via, 0xFF, (size_t)b->n_results * sizeof(uint32_t));
  return rc;
}

int batch_fetch(const HostModel&, const DeviceLexicon*, const Batch* b, anx_result** rows, size_t** offs, std::string& err) {
  if (!b->ran) { err = "batch has not been run"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(b->device));
  size_t* off = static_cast<size_t*>(malloc((b->n_input + 1) * sizeof(size_t)));
  anx_result* out = static_cast<anx_result*>(host_result_alloc(std::max<size_t>(1, b->n_results) * sizeof(anx_result)));
  if (!off || !out) { free(off); host_result_free(out); err = "out of memory"; return ANX_EINVAL; }
  const int rc = batch_fetch_into(b, out, off, 0, err);
  if (rc) { free(off); host_result_free(out); return rc; }
  *rows = out;
  *offs = off;
  return ANX_OK;
}

// anx_batch_fetch_measures for one shard: out[0 .. n_results) = the measures behind row r of batch_fetch_compact_into (same rows, same
// order), off[0 .. n_input] = base + the CSR offsets.  The vocabulary id -> entry table of the replica is built on first use; the
// offsets are the scan every fetch makes (enqueue_offsets); k_row_measures settles the short rows and lists the long ones for
// k_row_measures_long (kernels_explain.hpp).  Runs on the stream of the batch's last run.
static int vocab_entry_ensure(const HostModel& m, const DeviceLexicon* dl, hipStream_t st, std::string& err) {
  std::lock_guard<std::mutex> g(dl->explain_mu);
  if (dl->vocab_ent) return ANX_OK;
  const size_t V = std::max<size_t>(m.decoder.size(), 1);
  if (V >= 0xFFFFFFFFull) { err = "more than 2^32 vocabulary items"; return ANX_ELIMIT; }
  CallBlocks tmp(st);
  uint32_t* t = nullptr;
  if (const int rc = tmp.get(&t, V, err)) return rc;
  HIP_TRY(hipMemsetAsync(t, 0xFF, V * sizeof(uint32_t), st));
  if (dl->nentries) hipLaunchKernelGGL(k_vocab_entry_scatter, dim3((dl->nentries + 255) / 256), dim3(256), 0, st, dl->nentries, dl->ent_vocab, (uint32_t)V, t);
  HIP_TRY(hipGetLastError());
  if (const int rc = tmp.finish(err)) return rc;  // (another thread's stream may read the table as soon as the pointer is published)
  tmp.keep();  // the replica's from here on (lexicon_free)
  dl->vocab_ent_n = (uint32_t)V;
  dl->vocab_ent = t;
  return ANX_OK;
}
int replica_vocab_entries(const HostModel& m, const DeviceLexicon* dl, hipStream_t st, std::string& err) { return vocab_entry_ensure(m, dl, st, err); }
// The device sequence of anx_batch_fetch_measures, enqueued on st: the offsets of the compact export into ro.off[n_input + 1] and one
// record per ranked row into d_out[n_results], in export order.  d_list[n_surv + 4]: scratch ([0]: the list's length, rows from [4] on).
static int measures_enqueue(const HostModel& m, const DeviceLexicon* dl, const Batch* b, hipStream_t st, const RowOffsets& ro, uint4* d_out, uint32_t* d_list,
                            std::string& err) {
  const uint32_t total = (uint32_t)b->n_surv, nq32 = (uint32_t)b->nq;
  HIP_TRY(hipMemsetAsync(d_list, 0, 4 * sizeof(uint32_t), st));
  if (const int rc = enqueue_offsets(b, ro.cnt, ro.off, ro.tmp, st, err)) return rc;
  ExplainArgs k{};
  k.nq = nq32; k.total = total; k.V = dl->vocab_ent_n; k.nentries = dl->nentries; k.qw = b->qw; k.cstride = dl->cstride; k.n_out = (uint32_t)b->n_results;
  k.NP = dl->nplanes; k.bits_ok = (dl->nsym <= 32 && !switches().scan_sad) ? 1 : 0;
  k.soff = b->soff; k.r_count = b->r_count; k.q_orig = b->q_orig; k.off_orig = ro.off; k.q_meta = b->q_meta; k.r_rows = b->r_rows;
  k.q_rec = b->q_rec; k.q_rows = b->q_rows; k.q_bits = reinterpret_cast<const uint4*>(b->q_bits); k.q_cv = b->q_cv;
  k.vocab_ent = dl->vocab_ent; k.e_rec = dl->e_rec; k.scan_rec = dl->scan_rec; k.rows = dl->rows; k.cls_planes = dl->cls_planes; k.quot = dl->quot;
  k.w_ld = m.weights.ld; k.w_lcs = m.weights.lcs; k.w_prefix = m.weights.prefix; k.w_suffix = m.weights.suffix; k.w_case = m.weights.casew;
  k.w_sum = m.weights.ld + m.weights.lcs + m.weights.prefix + m.weights.suffix + m.weights.casew;  // src/types.rs:69-73, as launch_plan.hpp
  k.out = d_out; k.list = d_list + 4; k.list_n = d_list;
  {
    const int kt = ktimer_begin("k_row_measures", st);
    hipLaunchKernelGGL(k_row_measures, dim3((total + XM_THREADS - 1) / XM_THREADS), dim3(XM_THREADS), 0, st, k);
    ktimer_end(kt, st);
  }
  {
    const int kt = ktimer_begin("k_row_measures_long", st);
    hipLaunchKernelGGL(k_row_measures_long, dim3(std::min<uint32_t>(XM_LONG_BLOCKS, total)), dim3(64), 0, st, k);
    ktimer_end(kt, st);
  }
  HIP_TRY(hipGetLastError());
  return ANX_OK;
}
int batch_fetch_measures_into(const HostModel& m, const DeviceLexicon* dl, const Batch* b, anx_row_measures* out, uint32_t* off, uint32_t base, std::string& err) {
  static_assert(sizeof(anx_row_measures) == sizeof(uint4), "the record leaves as one 16-byte store");
  if (!dl) { err = "model is not resident on a device"; return ANX_ENODEVICE; }
  if (!b->ran) { err = "batch has not been run"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(b->device));
  const size_t n = b->n_input;
  if (!b->nq || !b->n_results) {
    for (size_t i = 0; i <= n; ++i) off[i] = base;
    return ANX_OK;
  }
  if (b->n_results >= 0xFFFFFFFFull || b->n_surv >= 0xFFFFFFFFull) { err = "more than 2^32 result rows"; return ANX_ELIMIT; }
  hipStream_t st = reinterpret_cast<hipStream_t>(b->last_stream);
  int rc;
  if ((rc = vocab_entry_ensure(m, dl, st, err))) return rc;
  CallBlocks tmp(st);
  RowOffsets ro;
  uint4* d_out = nullptr;
  uint32_t* d_list = nullptr;
  if ((rc = ro.get(tmp, n, err)) || (rc = tmp.get(&d_out, b->n_results, err)) || (rc = tmp.get(&d_list, (size_t)b->n_surv + 4, err))) return rc;
  if ((rc = measures_enqueue(m, dl, b, st, ro, d_out, d_list, err))) return rc;
  HIP_TRY(hipMemcpyAsync(off, ro.off, (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(out, d_out, b->n_results * sizeof(uint4), hipMemcpyDeviceToHost, st));
  if ((rc = tmp.finish(err))) return rc;
  if (base)
    for (size_t i = 0; i <= n; ++i) off[i] += base;
  return ANX_OK;
}

// The same records for the weight sweep (reweigh.hip): not downloaded but placed at dst on device dst_device, beside the shard's section
// of batch_gather_compact_via -- record r belongs to record r of that section.  Computed on the batch's own device into a pool block
// (in place when the batch lives on dst_device), copied over as gather_compact copies a section; returns when the bytes are there.
int batch_gather_measures(const HostModel& m, const DeviceLexicon* dl, const Batch* b, int dst_device, void* dst, size_t capacity, void* stream, std::string& err) {
  if (!dl) { err = "model is not resident on a device"; return ANX_ENODEVICE; }
  if (!b->ran) { err = "batch has not been run"; return ANX_EINVAL; }
  if (!b->nq || !b->n_results) return ANX_OK;
  if (b->n_results >= 0xFFFFFFFFull || b->n_surv >= 0xFFFFFFFFull) { err = "more than 2^32 result rows"; return ANX_ELIMIT; }
  const size_t need = (size_t)b->n_results * sizeof(uint4), n = b->n_input;
  if (!dst || capacity < need) { err = "measure buffer too small: " + std::to_string(need) + " bytes needed for this shard"; return ANX_ELIMIT; }
  HIP_TRY(hipSetDevice(b->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int rc;
  if ((rc = vocab_entry_ensure(m, dl, st, err))) return rc;
  const bool local = b->device == dst_device;
  CallBlocks tmp(st);
  RowOffsets ro;
  uint32_t* d_list = nullptr;
  uint4* d_out = static_cast<uint4*>(dst);
  if ((rc = ro.get(tmp, n, err)) || (rc = tmp.get(&d_list, (size_t)b->n_surv + 4, err)) || (!local && (rc = tmp.get(&d_out, b->n_results, err)))) return rc;
  if ((rc = measures_enqueue(m, dl, b, st, ro, d_out, d_list, err))) return rc;
  if (!local) HIP_TRY(hipMemcpyPeerAsync(dst, dst_device, d_out, b->device, need, st));
  return tmp.finish(err);
}

// Fixed-stride export into the caller's device memory: `stride` records per input (k_export_topk).  with_via: also the `via` word of
// every slot in a parallel array via[n_input * stride]: 0xFFFFFFFF for rows without one and for unused slots -- also those of inputs
// the encoder dropped (no query: their RECORD slots stay untouched)
static int export_topk(const Batch* b, void* dst, void* via, bool with_via, uint32_t stride, void* stream, std::string& err) {
  if (!b->ran) { err = "batch has not been run"; return ANX_EINVAL; }
  if (!dst || (with_via && !via) || stride == 0) { err = "bad export arguments"; return ANX_EINVAL; }
  if (stride < b->max_rows) {  // rows beyond the stride would be dropped silently (freq_weight != 0, variant lists or max_matches = 0
                               // can return more than max_matches + 1 rows): refuse
    err = "export stride " + std::to_string(stride) + " is smaller than the longest result list (" + std::to_string(b->max_rows) +
          " rows): use a larger stride or " + (with_via ? "anx_batch_export_compact_via" : "anx_batch_export_compact");
    return ANX_ELIMIT;
  }
  HIP_TRY(hipSetDevice(b->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  b->async_stream = stream; b->async_pending = true;
  if (with_via && b->nq < b->n_input) HIP_TRY(hipMemsetAsync(via, 0xFF, b->n_input * (size_t)stride * sizeof(uint32_t), st));
  const uint64_t total = (uint64_t)b->nq * stride;
  const dim3 grid((uint32_t)((total + 255) / 256));
  anx_topk_record* out = static_cast<anx_topk_record*>(dst);
  if (total && with_via) hipLaunchKernelGGL(k_export_topk<true>, grid, dim3(256), 0, st, (uint32_t)b->nq, stride, b->soff, b->r_count, b->r_rows, b->q_orig, out, static_cast<uint32_t*>(via));
  else if (total) hipLaunchKernelGGL(k_export_topk<false>, grid, dim3(256), 0, st, (uint32_t)b->nq, stride, b->soff, b->r_count, b->r_rows, b->q_orig, out, static_cast<uint32_t*>(nullptr));
  HIP_TRY(hipGetLastError());
  return ANX_OK;
}
int batch_export_topk(const DeviceLexicon*, const Batch* b, void* dst, uint32_t stride, void* stream, std::string& err) { return export_topk(b, dst, nullptr, false, stride, stream, err); }
int batch_export_topk_via(const DeviceLexicon*, const Batch* b, void* dst, void* via, uint32_t stride, void* stream, std::string& err) { return export_topk(b, dst, via, true, stride, stream, err); }

// Compact form of the same records: uint32 offsets[n+1] (input order; padded to a 16-byte multiple), then the
// n_results records back to back.  The size is known on the host (n_results is read back by the run), so the
// multi-GPU gather moves the used bytes only (config 2: 4.4 results per query, 74 MB per million instead of 176 MB).
// with_via: followed by the `via` words of its rows (EmitRecordVia): [u32 offsets[n + 1] padded to 16 bytes][records][u32 via[n_results]]
// -- offsets and records are the bytes of the form without; a model without variant lists gets 0xFFFFFFFF in every word
size_t batch_compact_bytes(const Batch* b) {
  return (((b->n_input + 1) * sizeof(uint32_t) + 15) & ~(size_t)15) + (b->ran ? (size_t)b->n_results : 0) * sizeof(anx_topk_record);
}
size_t batch_compact_via_bytes(const Batch* b) { return batch_compact_bytes(b) + (b->ran ? (size_t)b->n_results : 0) * sizeof(uint32_t); }
static int export_compact(const Batch* b, void* dst, size_t capacity, void* stream, size_t* used, bool with_via, std::string& err) {
  if (!b->ran) { err = "batch has not been run"; return ANX_EINVAL; }
  if (!dst || !used) { err = "bad export arguments"; return ANX_EINVAL; }
  const size_t n = b->n_input;
  const size_t off_bytes = ((n + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
  *used = with_via ? batch_compact_via_bytes(b) : batch_compact_bytes(b);
  if (capacity < *used) { err = "export buffer too small: " + std::to_string(*used) + " bytes needed"; return ANX_ELIMIT; }
  HIP_TRY(hipSetDevice(b->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  b->async_stream = stream; b->async_pending = true;
  uint32_t* d_off = static_cast<uint32_t*>(dst);
  anx_topk_record* d_rows = reinterpret_cast<anx_topk_record*>(static_cast<char*>(dst) + off_bytes);
  uint32_t* d_via = reinterpret_cast<uint32_t*>(d_rows + b->n_results);
  if (n == 0 || b->nq == 0) { HIP_TRY(hipMemsetAsync(d_off, 0, off_bytes, st)); return ANX_OK; }
  if (!b->x_cnt) {  // (the batch's: an asynchronous export outlives this call; batch_free waits for it and frees them)
    HIP_TRY(pool_malloc(reinterpret_cast<void**>(&b->x_cnt), n * sizeof(uint32_t)));
    HIP_TRY(pool_malloc(reinterpret_cast<void**>(&b->x_tmp), prefix_scan_tmp_bytes(n)));
  }
  const int rc = with_via ? enqueue_rows(b, b->x_cnt, d_off, b->x_tmp, st, EmitRecordVia{d_rows, d_via}, err) : enqueue_rows(b, b->x_cnt, d_off, b->x_tmp, st, EmitRecord{d_rows}, err);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return ANX_OK;
}
int batch_export_compact(const DeviceLexicon*, const Batch* b, void* dst, size_t capacity, void* stream, size_t* used, std::string& err) { return export_compact(b, dst, capacity, stream, used, false, err); }
int batch_export_compact_via(const DeviceLexicon*, const Batch* b, void* dst, size_t capacity, void* stream, size_t* used, std::string& err) { return export_compact(b, dst, capacity, stream, used, true, err); }

// with_via: the section is batch_export_compact_via's
static int gather_compact(const Batch* b, int dst_device, void* dst, size_t capacity, void* stream, bool with_via, std::string& err) {
  if (!b->ran) { err = "batch has not been run"; return ANX_EINVAL; }
  const size_t need = with_via ? batch_compact_via_bytes(b) : batch_compact_bytes(b);
  if (capacity < need) { err = "gather buffer too small: " + std::to_string(need) + " bytes needed for this shard"; return ANX_ELIMIT; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  size_t used = 0;
  if (b->device == dst_device) {  // already where the rows are wanted
    const int rc = export_compact(b, dst, capacity, stream, &used, with_via, err);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    return ANX_OK;
  }
  HIP_TRY(hipSetDevice(b->device));
  {  // direct access between the two devices where the topology has it (xGMI); without it the peer copy is staged by the runtime
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, b->device, dst_device) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(dst_device, 0);  // (or enabled already)
    (void)hipGetLastError();
  }
  CallBlocks tmp(st);  // (waits for st on every exit, as the call has to anyway: it returns when the bytes are there)
  char* sec = nullptr;
  int rc = tmp.get(&sec, need, err);
  if (rc) return rc;
  if ((rc = export_compact(b, sec, need, stream, &used, with_via, err))) return rc;
  const hipError_t e = hipMemcpyPeerAsync(dst, dst_device, sec, b->device, used, st);
  if (e != hipSuccess) { err = std::string("hipMemcpyPeerAsync: ") + hipGetErrorString(e); return ANX_ENODEVICE; }
  return ANX_OK;
}
int batch_gather_compact(const DeviceLexicon*, const Batch* b, int dst_device, void* dst, size_t capacity, void* stream, std::string& err) { return gather_compact(b, dst_device, dst, capacity, stream, false, err); }
int batch_gather_compact_via(const DeviceLexicon*, const Batch* b, int dst_device, void* dst, size_t capacity, void* stream, std::string& err) { return gather_compact(b, dst_device, dst, capacity, stream, true, err); }

bool batch_conf_fallback(const Batch* b) { return b->conf_fallback; }
int batch_download_text(const Batch* b, std::string& text, std::vector<uint32_t>& off, std::string& err) {
  if (b->n_input == 0) {  // a shard that received no inputs never allocated its text: it contributes nothing
    text.clear();
    off.assign(1, 0u);
    return ANX_OK;
  }
  if (!b->d_text || !b->d_textoff) { err = "the batch does not hold its inputs"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(b->device));
  off.assign(b->n_input + 1, 0u);
  HIP_TRY(hipMemcpy(off.data(), b->d_textoff, (b->n_input + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  text.assign(b->n_input ? (size_t)off[b->n_input] : 0, '\0');
  if (!text.empty()) HIP_TRY(hipMemcpy(&text[0], b->d_text, text.size(), hipMemcpyDeviceToHost));
  return ANX_OK;
}
void batch_stats(const Batch* b, anx_batch_stats* s) { *s = b->stats; }

}  // namespace anx
