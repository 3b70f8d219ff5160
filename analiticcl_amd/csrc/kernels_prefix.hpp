// kernels_prefix.hpp -- exclusive prefix sum (k_scan_local / k_scan_add; k_scan_sums for very long inputs) and the run's summary (k_run_summary)
// Part of the single translation unit engine.hip (included inside namespace anx); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------------
// Exclusive prefix sum (u32), two small kernels (three above SCAN_FUSED_BLOCKS * SCAN_TILE elements).  out has n+1 entries.
// ------------------------------------------------------------------------------------------------
constexpr int SCAN_ITEMS = 8, SCAN_THREADS = 256, SCAN_TILE = SCAN_ITEMS * SCAN_THREADS;

__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wsum[SCAN_THREADS / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wsum[wid] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
  for (int i = 0; i < SCAN_THREADS / 64; ++i) {
    if (i < wid) base += wsum[i];
    tot += wsum[i];
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_local(const uint32_t* __restrict__ in, uint32_t n,
                                                             uint32_t* __restrict__ out,
                                                             uint32_t* __restrict__ blocksum) {
  const uint32_t i0 = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS], s = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) {
    v[i] = i0 + i < n ? in[i0 + i] : 0;
    s += v[i];
  }
  uint32_t tot;
  uint32_t ex = block_exclusive_scan(s, &tot);
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) {
    if (i0 + i < n) out[i0 + i] = ex;
    ex += v[i];
  }
  if (threadIdx.x == 0) blocksum[blockIdx.x] = tot;
}
// (only above SCAN_FUSED_BLOCKS blocks: below that k_scan_add sums the block totals itself)
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_sums(uint32_t* __restrict__ blocksum, uint32_t nb) {
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < nb; b0 += SCAN_THREADS) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t v = i < nb ? blocksum[i] : 0;
    uint32_t tot;
    const uint32_t ex = block_exclusive_scan(v, &tot);
    if (i < nb) blocksum[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) blocksum[nb] = carry;
}
// sum of v over the block, in every thread
__device__ inline uint32_t block_sum(uint32_t v) {
  __shared__ uint32_t wsum[SCAN_THREADS / 64];
#pragma unroll
  for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t tot = 0;
#pragma unroll
  for (int i = 0; i < SCAN_THREADS / 64; ++i) tot += wsum[i];
  return tot;
}
// copy: nullptr, or a second array that receives out[0 .. n) as well (the compaction's cursors: no separate copy)
// fused: blocksum holds the blocks' TOTALS (no k_scan_sums ran): the block adds up the totals in front of it, block 0 all of them for
// out[n] -- nb * nb / 2 words read in all, so only up to SCAN_FUSED_BLOCKS blocks; else blocksum holds the offsets and [nb] the total
constexpr uint32_t SCAN_FUSED_BLOCKS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_add(uint32_t* __restrict__ out, uint32_t n,
                                                           const uint32_t* __restrict__ blocksum, uint32_t nb, uint32_t* __restrict__ copy, int fused) {
  const uint32_t i0 = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  uint32_t add, total;
  if (fused) {
    const uint32_t lim = blockIdx.x ? blockIdx.x : nb;
    uint32_t s = 0;
    for (uint32_t i = threadIdx.x; i < lim; i += SCAN_THREADS) s += blocksum[i];
    s = block_sum(s);
    add = blockIdx.x ? s : 0u;
    total = s;
  } else {
    add = blocksum[blockIdx.x];
    total = blockIdx.x ? 0u : blocksum[nb];
  }
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i)
    if (i0 + i < n) {
      const uint32_t v = out[i0 + i] + add;
      out[i0 + i] = v;
      if (copy) copy[i0 + i] = v;
    }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = total;
}

// What a run reports of its ranked lists (Run::compact_rank): ctl[w_total] += the sum, ctl[w_max] = the maximum of r_count[0 .. nq),
// one atomic of each per block; block 0 also copies the words the read-back wants beside them -- soff[nq] to ctl[w_surv] and, with
// confusables weighted on the device, cf_ctr[0 .. 2) to ctl[w_conf ..].  ctl is the run's control block, cleared at its start.
constexpr int SUMMARY_ITEMS = 16;
__global__ __launch_bounds__(SCAN_THREADS) void k_run_summary(const uint32_t* __restrict__ r_count, uint32_t nq, uint32_t* __restrict__ ctl,
                                                              uint32_t w_total, uint32_t w_max, const uint32_t* __restrict__ soff_end, uint32_t w_surv,
                                                              const uint32_t* __restrict__ cf_ctr, uint32_t w_conf) {
  __shared__ uint32_t wmax[SCAN_THREADS / 64];
  uint32_t s = 0, mx = 0;
  const uint32_t base = blockIdx.x * (SCAN_THREADS * SUMMARY_ITEMS) + threadIdx.x;
#pragma unroll 4
  for (int i = 0; i < SUMMARY_ITEMS; ++i) {
    const uint32_t q = base + i * SCAN_THREADS;
    const uint32_t v = q < nq ? r_count[q] : 0u;
    s += v;
    mx = max(mx, v);
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  s = block_sum(s);  // (its barrier also publishes wmax)
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < SCAN_THREADS / 64; ++i) mx = max(mx, wmax[i]);
    if (s) atomicAdd(ctl + w_total, s);
    if (mx) atomicMax(ctl + w_max, mx);
    if (blockIdx.x == 0) {
      ctl[w_surv] = *soff_end;
      if (cf_ctr) { ctl[w_conf] = cf_ctr[0]; ctl[w_conf + 1] = cf_ctr[1]; }
    }
  }
}

