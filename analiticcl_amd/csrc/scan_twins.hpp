// scan_twins.hpp -- queries with equal count vectors ("twins") in the scan, as ONE body of code for both encoders (encode.hip on
// the device, engine.hip's encode_host), the scan kernels (kernels_scan.hpp) and a stand-alone host test
// (tests/test_scan_twins_cpu.py).
//
// The class test of a bit-plane tile depends on a query only through its NBITPLANES thermometer planes.  Both encoders therefore
// order the queries of a (scan kernel, length, signature, kind) run by twin_hash of the planes, which puts equal planes next to
// each other, and scan_tile tests a run of equal planes once and copies the leader's hit bit onto its followers (twin_fill).
// The hash only orders: the kernel compares the planes themselves, so a collision interleaves two count vectors and loses some
// sharing, never a result.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ANX_TWIN_HD __host__ __device__ inline
#else
#define ANX_TWIN_HD inline
#endif

namespace anx {

constexpr int kTwinHashBits = 10;  // what the device encoder's 64-bit sort key has left below (kind flag + length, 8 x 5 signature bits, kind)

// Hash of the four plane words of a bit-plane query (kinds 1..4); count-vector queries (kind 0) sort with hash 0.
ANX_TWIN_HD uint32_t twin_hash(uint32_t p1, uint32_t p2, uint32_t p3, uint32_t p4) {
  uint32_t h = p1 * 0x9E3779B1u;
  h = (h ^ p2 ^ (h >> 15)) * 0x85EBCA77u;
  h = (h ^ p3 ^ (h >> 13)) * 0xC2B2AE3Du;
  h = (h ^ p4 ^ (h >> 16)) * 0x27D4EB2Fu;
  return (h ^ (h >> 15)) >> (32 - kTwinHashBits);
}

// Hit masks of a pass in shift-in order: the query tested first sits in the HIGHEST bit of the pass, a follower one bit below its
// predecessor.  p has the bit of every follower ("same planes as the query one bit above"), g[] the hit bits of the leaders and
// zeros at the followers' bits.  Copies every leader's bit onto its run of followers by doubling: after the step with shift s a
// bit has reached the followers up to 2s - 1 places below it, and p keeps the followers that are at least 2s places into their
// run; runs of up to 31 followers take five steps, a pass without twins none.
template <int N>
ANX_TWIN_HD void twin_fill(uint32_t (&g)[N], uint32_t p) {
  for (uint32_t s = 1; p; s <<= 1) {
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] |= p & (g[j] >> s);
    p &= p >> s;
  }
}

}  // namespace anx
