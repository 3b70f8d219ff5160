// eval_gather.h -- the ranked rows of a chunk's inputs as compact export sections on replica 0's device (eval_capi.cpp): what
// anx_evaluate_gold hands to eval.hip, and anx_evaluate_sweep (sweep_capi.cpp) to sweep.hip once per parameter set.
#pragma once
#include <deque>
#include <vector>

#include "engine.h"

// the sections of one chunk under one parameter set; the gather buffers go back to the device's pool with the object
struct anx_eval_gather {
  int dev0 = 0;
  std::vector<void*> bufs;
  std::vector<anx::LearnSection> secs;   // inputs relative to the chunk
  std::vector<size_t> sec_rows;
  std::deque<std::vector<uint32_t>> idx_store;
  size_t batch_runs = 0;
  // want_measures (anx_evaluate_sweep_weights): sec_meas[s] = one anx_row_measures per record of section s, beside it on the same device
  bool want_measures = false;
  std::vector<const anx_row_measures*> sec_meas;
  anx_eval_gather() = default;
  anx_eval_gather(const anx_eval_gather&) = delete;
  anx_eval_gather& operator=(const anx_eval_gather&) = delete;
  ~anx_eval_gather() { for (void* b : bufs) anx::eval_device_free(dev0, b); }
};
// The chunk's n inputs through the staged batch path with `p` (rounds of max_batch x replicas inputs, never the small call), every
// shard's compact export gathered onto replica 0's device (anx_batch_gather_compact_via).
// in == nullptr: the inputs are consecutive NUL-terminated spans of one blob (the packed calls): a round's part of it goes to the batch
// encoder as it is.  Returns an ANX_* code (the message is set).
int anx_eval_gather_rows(anx_model* m, const char* const* in, const anx::PairSpan* sa, size_t n, const anx_params* p, anx_eval_gather& out);
