"""scan_twins.hpp on the host (no GPU needed): the header both encoders and the scan kernels share is compiled into a stand-alone
C++ program that checks

  * twin_fill -- the doubling steps that copy a leader's hit bit onto its run of followers after a pass of the scan -- against a
    bit-by-bit loop: every (hit, twin) mask pair of 10 bits, and random 32-bit pairs whose runs have every length 1..31;
  * twin_hash -- the last sort key of both encoders -- is a function of the four planes alone (equal planes, equal hash), stays
    inside kTwinHashBits bits and spreads distinct planes over the buckets (an order that kept them apart would lose nothing but
    the sharing; one that mapped everything to one bucket would lose the ordering)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "analiticcl_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <set>
#include "scan_twins.hpp"

// Shift-in order: the query tested first sits in the highest bit, a follower one bit below its predecessor.  Walks the pass from
// the first query down and hands every follower the bit of the query above it.
static uint32_t fill_ref(uint32_t g, uint32_t p, int bits) {
  for (int i = bits - 2; i >= 0; --i)
    if ((p >> i) & 1u) g = (g & ~(1u << i)) | (((g >> (i + 1)) & 1u) << i);
  return g;
}
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

int main() {
  long checked = 0;
  // every pair of 10-bit masks: p never has the top bit of the pass (the first query follows nobody), g is zero at the followers
  for (uint32_t p = 0; p < 512u; ++p)
    for (uint32_t h = 0; h < 1024u; ++h) {
      const uint32_t g0 = h & ~p;
      uint32_t g[1] = {g0};
      anx::twin_fill(g, p);
      if (g[0] != fill_ref(g0, p, 10)) { printf("fill: p=%x g=%x -> %x, expected %x\n", p, g0, g[0], fill_ref(g0, p, 10)); return 1; }
      ++checked;
    }
  // 32-bit passes: one run of every length 1..31 at every position, other runs around it at random; four masks at once as the kernel
  // calls it
  for (int len = 1; len <= 31; ++len)
    for (int top = len; top <= 31; ++top)        // the leader's bit; followers top-1 .. top-len
      for (int rep = 0; rep < 16; ++rep) {
        uint32_t p = rnd() & rnd() & 0x7FFFFFFFu;
        const uint32_t run = (len == 32 ? 0xFFFFFFFFu : ((1u << len) - 1u)) << (top - len);
        p = (p | run) & ~(1u << top);
        if (top - len - 1 >= 0) p &= ~(1u << (top - len - 1));  // the run ends where it should
        uint32_t g[4], g0[4];
        for (int j = 0; j < 4; ++j) g[j] = g0[j] = rnd() & ~p;
        anx::twin_fill(g, p);
        for (int j = 0; j < 4; ++j)
          if (g[j] != fill_ref(g0[j], p, 32)) { printf("fill32: p=%x g=%x -> %x, expected %x\n", p, g0[j], g[j], fill_ref(g0[j], p, 32)); return 1; }
        ++checked;
      }
  // a pass without twins is left alone
  { uint32_t g[2] = {0xDEADBEEFu, 0u}; anx::twin_fill(g, 0u); if (g[0] != 0xDEADBEEFu || g[1] != 0u) return 2; }
  // the hash: a pure function of the planes, inside its bits, and not constant
  std::set<uint32_t> seen;
  for (int i = 0; i < 20000; ++i) {
    const uint32_t p1 = rnd(), p2 = p1 & rnd(), p3 = p2 & rnd(), p4 = p3 & rnd();  // thermometer planes are nested
    const uint32_t h = anx::twin_hash(p1, p2, p3, p4);
    if (h != anx::twin_hash(p1, p2, p3, p4)) return 3;
    if (h >> anx::kTwinHashBits) { printf("hash out of range: %x\n", h); return 4; }
    seen.insert(h);
  }
  if (seen.size() < (1u << anx::kTwinHashBits) * 9 / 10) { printf("hash uses %zu buckets\n", seen.size()); return 5; }
  // planes that differ in one bit of one plane (a letter more or less: the common neighbours inside a signature) rarely collide
  int coll = 0;
  for (int i = 0; i < 4000; ++i) {
    const uint32_t p1 = rnd() & 0x3FFFFFFu, bit = 1u << (rnd() % 26u);
    if (anx::twin_hash(p1, 0, 0, 0) == anx::twin_hash(p1 ^ bit, 0, 0, 0)) ++coll;
    if (anx::twin_hash(p1 | bit, 0, 0, 0) == anx::twin_hash(p1 | bit, bit, 0, 0)) ++coll;
  }
  if (coll > 80) { printf("%d collisions of 8000 neighbours\n", coll); return 6; }  // 8000 / 1024 expected
  printf("ok %ld\n", checked);
  return 0;
}
"""


def test_twin_fill_and_hash_against_bit_loops(tmp_path):
    src = tmp_path / "twins_main.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "twins_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-I", CSRC, "-o", exe, str(src)])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok ")
