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

// The ASCII presence bits of one side from its bytes, and whether the bytes are anything but well-formed UTF-8 (a stray continuation
// byte, a lead byte without its continuation bytes, an overlong form, 0xF8..).  The decoder of k_pairs_conf_script and of the host
// takes the length from the lead byte alone: on such bytes it may swallow an ASCII byte into a character, or produce an ASCII
// character from non-ASCII bytes, so bits and byte-wise prefix / suffix say nothing about the decoded string.
__device__ inline bool pairs_side_bits(const uint8_t* __restrict__ blob, uint32_t t0, uint32_t t1, cdiff::CharSet& cs) {
  cs.w[0] = cs.w[1] = 0;
  cs.other = 0;
  bool bad = false;
  uint32_t pend = 0, lo = 0x80u;
  for (uint32_t x = t0; x < t1; ++x) {
    const uint32_t ch = blob[x];
    if (ch < 64u) cs.w[0] |= 1ull << ch; else if (ch < 128u) cs.w[1] |= 1ull << (ch - 64u); else cs.other = 1;
    if (pend) {
      if ((ch & 0xC0u) != 0x80u || ch < lo) bad = true;
      --pend;
      lo = 0x80u;
    } else if (ch >= 0x80u) {
      if (ch >= 0xC2u && ch < 0xE0u) pend = 1;
      else if (ch >= 0xE0u && ch < 0xF0u) { pend = 2; lo = ch == 0xE0u ? 0xA0u : 0x80u; }
      else if (ch >= 0xF0u && ch < 0xF8u) { pend = 3; lo = ch == 0xF0u ? 0x90u : 0x80u; }
      else bad = true;
    }
  }
  return bad || pend != 0;
}

// An instruction with a multi-character or non-ASCII option, on presence bits: one of its options must have every ASCII character in
// the set (s0, s1) and, if it has a character beyond ASCII, the string(s) must have one too (`other`).  Necessary like the bits of a
// `simple` instruction: the option is a substring of the text it is matched against.
__device__ inline bool pairs_opt_may(const cdiff::Patterns& P, const cdiff::FlatOp& o, uint64_t s0, uint64_t s1, bool other) {
  for (uint32_t k = 0; k < o.nopt; ++k) {
    const cdiff::FlatOpt opt = P.opts[o.opt_begin + k];
    bool all = true;
    for (uint32_t i = 0; i < opt.len && all; ++i) {
      const uint32_t cp = P.pool[opt.off + i];
      all = cp < 64u ? (s0 >> cp) & 1ull : cp < 128u ? (s1 >> (cp - 64u)) & 1ull : other;
    }
    if (all) return true;
  }
  return false;
}

}  // namespace anx
