// kernels_fetch.hpp -- the kernels that lay the ranked rows of a finished run out in the CALLER's input order (results.hip)
// Included inside namespace anx after kernels_common.hpp; gfx950 only.
#pragma once

// download / export path: result rows in the CALLER's input order -- the counts scattered to the input indices (k_fetch_counts), an
// exclusive scan over them, then the rows through an emitter (k_emit_rows)
__global__ __launch_bounds__(256) void k_fetch_counts(uint32_t nq, const uint32_t* __restrict__ r_count,
                                                      const uint32_t* __restrict__ q_orig, uint32_t* __restrict__ cnt_orig) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s < nq) cnt_orig[q_orig[s]] = r_count[s];
}
// DevRow -> the 16-byte compact record (freq_score as float32)
__device__ inline anx_topk_record topk_record_of(const DevRow& d) {
  anx_topk_record r;
  r.vocab_id = d.vocab_id;
  r.freq_score = (float)d.freq_score;
  r.dist_score = d.dist_score;
  return r;
}
// What k_emit_rows writes for a row: the anx_result of the download, the compact record of the compact fetch and the gather, or
// the compact record plus `via` (the vocabulary id of the variant a row was reached through, 0xFFFFFFFF = none) as a parallel
// array, one word per row -- the 16-byte record keeps its layout for models with variant lists.
struct EmitResult {
  anx_result* out;
  __device__ void operator()(uint32_t at, const DevRow& d) const {
    anx_result r;
    r.vocab_id = d.vocab_id;
    r.dist_score = d.dist_score;
    r.freq_score = d.freq_score;
    r.via = d.via == 0xFFFFFFFFu ? ANX_NO_VIA : (uint64_t)d.via;
    out[at] = r;
  }
};
struct EmitRecord {
  anx_topk_record* out;
  __device__ void operator()(uint32_t at, const DevRow& d) const { out[at] = topk_record_of(d); }
};
struct EmitRecordVia {
  anx_topk_record* out;
  uint32_t* via;
  __device__ void operator()(uint32_t at, const DevRow& d) const {
    out[at] = topk_record_of(d);
    via[at] = d.via;
  }
};
// rows of query s (sorted order) -> emit at off_orig[q_orig[s]] .. (input order, no padding)
template <typename Emit>
__global__ __launch_bounds__(256) void k_emit_rows(uint32_t nq, const uint32_t* __restrict__ soff, const uint32_t* __restrict__ r_count,
                                                   const DevRow* __restrict__ r_rows, const uint32_t* __restrict__ q_orig,
                                                   const uint32_t* __restrict__ off_orig, Emit emit) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nq) return;
  const uint32_t n = r_count[s], src = soff[s], dst = off_orig[q_orig[s]];
  for (uint32_t i = 0; i < n; ++i) emit(dst + i, r_rows[src + i]);
}
// fixed-stride export: `stride` records per query in input order, the unused ones marked with vocab_id 0xFFFFFFFF
// VIA: also one `via` word per slot into the parallel array out_via (0xFFFFFFFF for rows without one and for unused slots)
template <bool VIA>
__global__ __launch_bounds__(256) void k_export_topk(uint32_t nq, uint32_t stride, const uint32_t* __restrict__ soff,
                                                     const uint32_t* __restrict__ r_count,
                                                     const DevRow* __restrict__ r_rows,
                                                     const uint32_t* __restrict__ q_orig,
                                                     anx_topk_record* __restrict__ out, uint32_t* __restrict__ out_via) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (uint64_t)nq * stride) return;
  const uint32_t q = (uint32_t)(t / stride), i = (uint32_t)(t % stride);
  anx_topk_record r;
  r.vocab_id = 0xFFFFFFFFu;
  r.freq_score = 0.0f;
  r.dist_score = 0.0;
  uint32_t via = 0xFFFFFFFFu;
  if (i < r_count[q]) {
    const DevRow d = r_rows[soff[q] + i];
    r = topk_record_of(d);
    if constexpr (VIA) via = d.via;
  }
  out[(size_t)q_orig[q] * stride + i] = r;
  if constexpr (VIA) out_via[(size_t)q_orig[q] * stride + i] = via;
}
