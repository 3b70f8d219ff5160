// pair_spans.h -- what the C API files of the calls over caller-chosen string pairs share (pairs_capi.cpp, mine_capi.cpp, eval_capi.cpp,
// sweep_capi.cpp, reweigh_capi.cpp; learn_capi.cpp for the vocabulary table): the two input forms as spans, and the model's slot for
// learn mode's vocabulary table.  The argument checks and the chunking differ per call and stay in those files.
#pragma once
#include <cstring>
#include <vector>

#include "engine.h"

void** anx_learn_vocab_slot(anx_model* m, void (*release)(void*));  // capi.cpp

namespace anx {

// the first n NUL-terminated spans of blob[0, len); false: the blob holds fewer
inline bool spans_of(const char* blob, size_t len, size_t n, std::vector<PairSpan>& out) {
  out.resize(n);
  size_t pos = 0;
  for (size_t i = 0; i < n; ++i) {
    const char* z = pos < len ? static_cast<const char*>(memchr(blob + pos, 0, len - pos)) : nullptr;
    if (!z) return false;
    out[i] = PairSpan{blob + pos, (size_t)(z - (blob + pos))};
    pos = (size_t)(z - blob) + 1;
  }
  return true;
}
// the n C strings of the pointer form; false: a NULL string
inline bool spans_of_pointers(const char* const* s, size_t n, std::vector<PairSpan>& out) {
  out.resize(n);
  for (size_t i = 0; i < n; ++i) {
    if (!s[i]) return false;
    out[i] = PairSpan{s[i], strlen(s[i])};
  }
  return true;
}
// where the model keeps learn mode's vocabulary table on the device (the caller holds the learn lock); the model frees it with learn_vocab_free
inline LearnVocab** learn_vocab_slot(anx_model* m) {
  return reinterpret_cast<LearnVocab**>(anx_learn_vocab_slot(m, [](void* p) { learn_vocab_free(static_cast<LearnVocab*>(p)); }));
}

}  // namespace anx
