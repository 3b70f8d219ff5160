// conf_rank.hpp -- the order of ranked rows after the confusable weights: what k_conf_apply_late (conf.hip) sorts and cuts off by, and
// what the confusable fit (fit.hip) counts by.  Included inside namespace anx after kernels_common.hpp (DevRow).
#pragma once

__device__ inline double conf_vr_score(const DevRow& r, float fw) {  // src/types.rs:335-341
  if (fw == 0.0f) return r.dist_score;
  return (r.dist_score + ((double)fw * r.freq_score)) / (1.0 + (double)fw);
}
__device__ inline bool conf_before(const DevRow& x, const DevRow& y, float fw) {  // rank_cmp, src/types.rs:344-365: x strictly before y
  if (fw > 0.0f) return conf_vr_score(x, fw) > conf_vr_score(y, fw);
  if (x.dist_score != y.dist_score) return x.dist_score > y.dist_score;
  return x.freq_score > y.freq_score;
}
