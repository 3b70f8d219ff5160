// reweigh_shared.hpp -- what reweigh.hip (anx_evaluate_sweep_weights) and csweep.hip (anx_evaluate_sweep_confusables) both compile: the
// score's arithmetic, the run-of-equal-keys helper of their flat row kernels, and the group's buffers.
// Included inside namespace anx after kernels_common.hpp and kernels_gold.hpp.
#pragma once

// the score's operands for one set
struct RwWeights {
  double w_ld, w_lcs, w_prefix, w_suffix, w_case, w_sum;
  const double* quot;  // [33][33] x / L as the host divides (DeviceLexicon::quot), or nullptr
};
// src/lib.rs:1433-1452 with input_length = la, as score_finish (kernels_score.hpp) and xm_score (kernels_explain.hpp) write it
__device__ inline double rw_score(const RwWeights& k, uint32_t la, uint32_t ld, uint32_t lcs, uint32_t pre, uint32_t suf, uint32_t samecase) {
  const double L = (double)la;
  const bool tab = k.quot && la <= 32u;
  auto over_L = [&](uint32_t x) { return (tab && x <= 32u) ? k.quot[x * 33u + la] : (double)x / L; };
  const double distance_score = ld > la ? 0.0 : 1.0 - over_L(ld);
  const double lcs_score = over_L(lcs);
  const double prefix_score = over_L(pre);
  const double suffix_score = over_L(suf);
  const double num = k.w_ld * distance_score + k.w_lcs * lcs_score + k.w_prefix * prefix_score + k.w_suffix * suffix_score + (samecase ? k.w_case : 0.0);
  return k.w_sum == 1.0 ? num : num / k.w_sum;  // x / 1.0 == x
}

// The run of equal keys among neighbouring lanes this lane lies in (survivor_counts, kernels_score.hpp): its first and last lane and
// the mask of its lanes.  Every lane of the wave calls this.
struct RwRun { uint32_t start, end; unsigned long long lanes; };
__device__ __forceinline__ RwRun rw_run(uint32_t key) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t kprev = (uint32_t)__shfl_up((int)key, 1);
  const bool head = lane == 0u || kprev != key;
  const unsigned long long hm = __ballot(head);
  const uint32_t start = 63u - (uint32_t)__clzll((long long)(hm & ((2ull << lane) - 1ull)));  // (lane 0 is a head)
  const unsigned long long above = lane == 63u ? 0ull : hm & ~((2ull << lane) - 1ull);
  const uint32_t end = above ? (uint32_t)__ffsll((long long)above) - 2u : 63u;
  return RwRun{start, end, ((2ull << end) - 1ull) & ~((1ull << start) - 1ull)};
}

// ---- host: one group's buffers (reweigh_group_begin fills them, reweigh_group_end returns them) ---------------------------------------
struct RwGroup {
  SweepChunkView v{};
  size_t n = 0, R = 0;
  PoolBlocks blocks;               // pool blocks of the group, back to the pool at its end
  void* h_down = nullptr;          // pinned: the summary | the records
  uint4* info = nullptr;
  uint2* meas = nullptr;
  double *score = nullptr, *t_key = nullptr;
  uint32_t *cnt = nullptr, *soff = nullptr, *cur = nullptr, *maxf = nullptr, *tmp = nullptr, *r_count = nullptr, *ovf = nullptr, *pre = nullptr;
  SurvRow* c_rows = nullptr;
  DevRow* r_rows = nullptr;
  unsigned long long* d_sum = nullptr;
  uint4* d_out = nullptr;
  template <typename T>
  int get(T** p, size_t count, std::string& err) { return blocks.get(p, count, err); }
};
