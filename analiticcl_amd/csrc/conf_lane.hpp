// conf_lane.hpp -- the per-lane working memory of the edit-script kernels (conf.hip: k_conf_script, k_pairs_conf_script; mine.hip:
// k_mine_script) and the byte decoder they share.  Include after hip_runtime.h and engine_internal.h.
#pragma once
#include "confusables_core.hpp"

namespace anx {

// per-lane working memory (k_conf_script): words of the lane memory of confusables_core.hpp, the 64 lanes of a wave interleaved
// (word w of lane l = block[w * 64 + l]): lanes that work on the same word of their own rows share cache lines
constexpr uint32_t CF_MAXCP = 64;      // code points per string the device handles
constexpr uint32_t CF_ARENA = 768;     // code points
constexpr uint32_t CF_DIFFS = 48;
constexpr uint32_t CF_V = 4 * (CF_MAXCP + 2) + 8;
constexpr uint32_t CF_FRAMES = 16;
constexpr uint32_t CF_IN_OFF = 0, CF_CAND_OFF = CF_MAXCP, CF_ARENA_OFF = 2 * CF_MAXCP, CF_D_OFF = CF_ARENA_OFF + CF_ARENA,
                   CF_V_OFF = CF_D_OFF + CF_DIFFS * cdiff::DIFF_WORDS, CF_F_OFF = CF_V_OFF + CF_V,
                   CF_WORDS = CF_F_OFF + CF_FRAMES * cdiff::FRAME_WORDS;
constexpr uint32_t CF_BLOCKS = 4096, CF_THREADS = 64;  // lanes in flight = working sets of a batch (262 k x 5.8 KB = 1.5 GB of HBM; 8192 blocks measured no faster)
#ifndef ANX_CF_G
#define ANX_CF_G 4
#endif
constexpr uint32_t CF_G = ANX_CF_G;  // words of a lane that stay together
typedef cdiff::Core<64, CF_G> DC;

// UTF-8 -> scalar values into the lane memory at word `dst`, exactly as the host's utf8_decode_at (host_model.cpp): the length comes
// from the lead byte alone (a sequence the string is too short for, a stray continuation byte and 0xF8.. are one byte that decodes
// to itself) -- the host function is this kernel's fallback, so the two must read any bytes alike.  false: more than CF_MAXCP code points
__device__ inline bool pairs_conf_decode(const cdiff::Ctx& c, const uint8_t* __restrict__ text, uint32_t t0, uint32_t t1, uint32_t dst, uint32_t* n_out) {
  uint32_t n = 0;
  for (uint32_t p = t0; p < t1;) {
    const uint32_t b0 = text[p];
    uint32_t len = b0 < 0x80u ? 1u : (b0 >> 5) == 0x6u ? 2u : (b0 >> 4) == 0xEu ? 3u : (b0 >> 3) == 0x1Eu ? 4u : 1u;
    if (len > t1 - p) len = 1u;
    uint32_t cp = b0;
    if (len == 2u) cp = ((b0 & 0x1Fu) << 6) | (text[p + 1] & 0x3Fu);
    else if (len == 3u) cp = ((b0 & 0x0Fu) << 12) | ((text[p + 1] & 0x3Fu) << 6) | (text[p + 2] & 0x3Fu);
    else if (len == 4u) cp = ((b0 & 0x07u) << 18) | ((text[p + 1] & 0x3Fu) << 12) | ((text[p + 2] & 0x3Fu) << 6) | (text[p + 3] & 0x3Fu);
    if (n >= CF_MAXCP) return false;
    DC::W(c, dst + n++) = cp;
    p += len;
  }
  *n_out = n;
  return true;
}

}  // namespace anx
