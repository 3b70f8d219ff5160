// pairs.hip -- anx_score_pairs: the model's measures for caller-chosen string pairs (gfx950 / CDNA4).
//
// Replaces, for a whole list of pairs at once, the reference's public distance functions on two normalised strings:
// damerau_levenshtein(a, b, 255) (src/distance.rs:101-179), longest_common_substring_length (:181-205), common_prefix_length
// (:207-218), common_suffix_length (:220-231), the case test of src/lib.rs:1367-1377 and the distance score of src/lib.rs:1433-1452.
// No lexicon entry is involved.  Both sides of a chunk are ONE blob of 2 n strings (a of pair i = string i, b = string n + i) that
// goes through the query encoder's k_enc_strings (encode.hip pairs_encode_launch): codes at code_off, symbols and the case flag in meta.
//
// The Damerau-Levenshtein here is the UNRESTRICTED one with no distance bound -- the full Lowrance-Wagner recurrence
//   D[i][j] = min(D[i][j-1] + 1, D[i-1][j] + 1, D[i-1][j-1] + (a_i != b_j), D[last-1][db-1] + (i - last - 1) + 1 + (j - db - 1))
// with last = the last row before i whose symbol is b_j and db = the last column before j of row i that matched: the transposition
// term reaches an arbitrary earlier row, so the pair's whole matrix is addressable (LDS).  The engine's other DL kernels
// (kernels_score.hpp) compute only outcomes <= d.  The reference's guard row and column hold la + lb and can never win the minimum;
// "no earlier occurrence" (last == 0 or db == 0) is tested instead, so a cell is a byte (D <= max(la, lb) <= 255) and nothing
// larger is ever stored.  Row 0 and column 0 (D[0][j] = j, D[i][0] = i) are computed, not stored.
//   k_pairs_short : both sides <= 16 BYTES (so <= 16 symbols: the host classifies by bytes, no compaction on the device): a pair per
//                   lane, a 16 x 16 byte matrix + both strings per lane in LDS at an odd dword stride; `last` per column is a nibble
//                   of one 64-bit register
//   k_pairs_long  : everything else, up to 255 symbols a side: a pair per wave, the lanes run along the anti-diagonal of a strip of
//                   64 rows; `last` = the highest lower lane of the strip whose symbol is b_j (a 64-bit mask per column, built per
//                   strip) or, failing that, the per-symbol table of the rows above the strip
// LCS is the longest run of equal symbols along a diagonal; prefix / suffix the first mismatch from either end.  The score restates
// score_finish (kernels_score.hpp) term by term: same association, x / L from DeviceLexicon::quot where score_finish takes it there,
// no FMA contraction (-ffp-contract=off).
// anx_score_pairs_weighted adds the confusable weight of every pair (src/lib.rs:1733-1756): the kernels are conf.hip's
// (conf_launch_pairs), enqueued here behind the pair kernels on the chunk's uploaded blob; this file owns their buffers, the second
// download, and the host's share (pairs the device marks NaN; every pair under ANX_CONFUSABLES=host).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "engine_internal.h"

namespace anx {

#include "kernels_common.hpp"

struct PairKArgs {
  uint32_t n;               // pairs of the chunk: string i = a of pair i, string n + i = its b
  const uint32_t* off;      // [2 n + 1] byte offsets of the strings (each followed by one NUL byte)
  const uint8_t* codes;     // k_enc_strings: the codes of string i at code_off(off[i], i)
  const uint32_t* meta;     // [2 n] symbols | .. | first_is_lower << 24; 0 = empty or more than 255 symbols
  const uint32_t* idx;      // the pairs of this tier
  uint32_t count;
  anx_pair_score* out;      // [n]
  const double* quot;       // [33][33] x / L as the host divides (DeviceLexicon::quot), or nullptr
  double w_ld, w_lcs, w_prefix, w_suffix, w_case, w_sum;
};

// src/lib.rs:1433-1452 with input_length = la, as score_finish (kernels_score.hpp) writes it
__device__ inline double pair_score(const PairKArgs& k, uint32_t la, uint32_t ld, uint32_t lcs, uint32_t pre, uint32_t suf, uint32_t samecase) {
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
__device__ inline void pair_store(anx_pair_score* o, double score, uint32_t ld, uint32_t lcs, uint32_t pre, uint32_t suf, uint32_t la, uint32_t lb,
                                  uint32_t samecase, int status) {
  anx_pair_score r;
  r.score = score;
  r.ld = (uint16_t)ld; r.lcs = (uint16_t)lcs; r.prefixlen = (uint16_t)pre; r.suffixlen = (uint16_t)suf;
  r.len_a = (uint8_t)la; r.len_b = (uint8_t)lb;
  r.samecase = (uint8_t)samecase;
  r.status = (int8_t)status;
  r._pad = 0u;
  *o = r;
}
// meta == 0: the string is empty or has more than 255 symbols -- the byte length tells which
__device__ inline int pair_status(const PairKArgs& k, uint32_t p, uint32_t& ma, uint32_t& mb) {
  ma = k.meta[p];
  mb = k.meta[k.n + p];
  const uint32_t ba = k.off[p + 1u] - k.off[p] - 1u, bb = k.off[k.n + p + 1u] - k.off[k.n + p] - 1u;
  if (!ba || !bb) return ANX_EEMPTY;
  if (!ma || !mb) return ANX_ELIMIT;
  return ANX_OK;
}
__device__ inline const uint32_t* pair_codes(const PairKArgs& k, uint32_t s) { return reinterpret_cast<const uint32_t*>(k.codes + code_off(k.off[s], s)); }

// ---- short tier: a pair per lane ------------------------------------------------------------------------------------------------
constexpr uint32_t PS_THREADS = 128;
constexpr uint32_t PS_STRIDE = 73;   // dwords per lane: 64 of the matrix, 4 + 4 of the strings, one more for an odd stride (conflict-free)
__global__ __launch_bounds__(PS_THREADS) void k_pairs_short(PairKArgs k) {
  __shared__ uint32_t s_all[PS_THREADS * PS_STRIDE];
  const uint32_t t = blockIdx.x * PS_THREADS + threadIdx.x;
  if (t >= k.count) return;  // (no barrier below)
  const uint32_t p = k.idx[t];
  uint32_t ma, mb;
  int status = pair_status(k, p, ma, mb);
  const uint32_t la = ma & 0xFFu, lb = mb & 0xFFu;
  if (!status && (la > 16u || lb > 16u)) status = ANX_ELIMIT;  // (symbols <= bytes <= 16: cannot happen; the lane's matrix holds 16 x 16)
  if (status) { pair_store(k.out + p, 0.0, 0u, 0u, 0u, 0u, la, lb, 0u, status); return; }
  uint32_t* mine = s_all + threadIdx.x * PS_STRIDE;
  uint8_t* M = reinterpret_cast<uint8_t*>(mine);             // D[i][j] at (i - 1) * 16 + (j - 1), 1 <= i, j <= 16
  const uint8_t* A = reinterpret_cast<const uint8_t*>(mine + 64);
  const uint8_t* B = reinterpret_cast<const uint8_t*>(mine + 68);
  {
    const uint32_t *ca = pair_codes(k, p), *cb = pair_codes(k, k.n + p);
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) {
      mine[64 + w] = 4u * w < la ? ca[w] : 0u;
      mine[68 + w] = 4u * w < lb ? cb[w] : 0u;
    }
  }
  unsigned long long lr = 0;  // nibble j - 1: the last row before the current one whose symbol equals b_j (0: none; row 16 is never read)
  for (uint32_t i = 1; i <= la; ++i) {
    const uint32_t ai = A[i - 1u];
    uint32_t left = i, diag = i - 1u, db = 0;
    for (uint32_t j = 1; j <= lb; ++j) {
      const uint32_t up = i == 1u ? j : M[(i - 2u) * 16u + (j - 1u)];
      const bool eq = ai == B[j - 1u];
      uint32_t v = min(min(left, up) + 1u, diag + (eq ? 0u : 1u));
      const uint32_t sh = 4u * (j - 1u);
      const uint32_t last = (uint32_t)(lr >> sh) & 15u;
      if (last && db) {  // D[last - 1][db - 1]: a boundary cell when either index is 0
        const uint32_t r = last - 1u, c = db - 1u;
        const uint32_t src = r == 0u ? c : c == 0u ? r : M[(r - 1u) * 16u + (c - 1u)];
        v = min(v, src + (i - last - 1u) + 1u + (j - db - 1u));
      }
      M[(i - 1u) * 16u + (j - 1u)] = (uint8_t)v;
      if (eq) {
        db = j;
        lr = (lr & ~(15ull << sh)) | ((unsigned long long)(i & 15u) << sh);
      }
      diag = up;
      left = v;
    }
  }
  const uint32_t ld = M[(la - 1u) * 16u + (lb - 1u)];
  // longest common substring = the longest run of equal symbols on any diagonal; prefix / suffix
  uint32_t lcs = 0;
  for (int delta = -(int)la + 1; delta < (int)lb; ++delta) {
    const int i0 = delta < 0 ? -delta : 0, i1 = min((int)la, (int)lb - delta);
    if (i1 - i0 <= (int)lcs) continue;
    uint32_t run = 0;
    for (int i = i0; i < i1; ++i) {
      run = A[i] == B[i + delta] ? run + 1u : 0u;
      lcs = max(lcs, run);
    }
  }
  const uint32_t m = min(la, lb);
  uint32_t pre = 0, suf = 0;
  while (pre < m && A[pre] == B[pre]) ++pre;
  while (suf < m && A[la - 1u - suf] == B[lb - 1u - suf]) ++suf;
  const uint32_t samecase = ((ma >> 24) & 1u) == ((mb >> 24) & 1u) ? 1u : 0u;
  pair_store(k.out + p, pair_score(k, la, ld, lcs, pre, suf, samecase), ld, lcs, pre, suf, la, lb, samecase, ANX_OK);
}

// ---- long tier: a pair per wave ---------------------------------------------------------------------------------------------------
// ML = the most symbols a side may have (64 or 255: the host picks the smaller kernel when every long pair of the chunk fits it).
// Rows of the matrix are S bytes apart with S = 5 mod 8: the lanes of a step lie S - 1 bytes apart, an odd number of dwords.
template <int ML>
struct PairsLong {
  static constexpr uint32_t S = ML <= 64 ? 69u : 261u;
  static constexpr uint32_t MAT_DW = (ML * S + 3u) / 4u, STR_DW = (ML + 3u) / 4u;
  static_assert(S >= (uint32_t)ML && S % 8u == 5u, "row stride");
};
template <int ML>
__global__ __launch_bounds__(64) void k_pairs_long(PairKArgs k) {
  using P = PairsLong<ML>;
  constexpr uint32_t S = P::S;
  __shared__ unsigned long long s_mask[ML + 1];  // per column of b: the rows of the current strip (bit = lane) whose symbol equals it
  __shared__ uint32_t s_mat32[P::MAT_DW];        // D[i][j] at (i - 1) * S + (j - 1)
  __shared__ uint32_t s_a32[P::STR_DW], s_b32[P::STR_DW];
  __shared__ uint8_t s_tab[256];                 // per symbol code: its last row above the current strip (0: none)
  uint8_t* mat = reinterpret_cast<uint8_t*>(s_mat32);
  const uint8_t* A = reinterpret_cast<const uint8_t*>(s_a32);
  const uint8_t* B = reinterpret_cast<const uint8_t*>(s_b32);
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x >= k.count) return;  // block-uniform
  const uint32_t p = k.idx[blockIdx.x];
  uint32_t ma, mb;
  int status = pair_status(k, p, ma, mb);
  const uint32_t la = ma & 0xFFu, lb = mb & 0xFFu;
  if (!status && (la > (uint32_t)ML || lb > (uint32_t)ML)) status = ANX_ELIMIT;  // (the host picked ML from the byte lengths: cannot happen)
  if (status) {  // block-uniform
    if (lane == 0u) pair_store(k.out + p, 0.0, 0u, 0u, 0u, 0u, la, lb, 0u, status);
    return;
  }
  {
    const uint32_t *ca = pair_codes(k, p), *cb = pair_codes(k, k.n + p);
    for (uint32_t w = lane; w < (la + 3u) / 4u; w += 64u) s_a32[w] = ca[w];
    for (uint32_t w = lane; w < (lb + 3u) / 4u; w += 64u) s_b32[w] = cb[w];
    for (uint32_t x = lane; x < 256u; x += 64u) s_tab[x] = 0;
  }
  __syncthreads();
  // ---- prefix / suffix: the first mismatch from either end, 64 positions a round ----
  const uint32_t m = min(la, lb);
  uint32_t pre = m, suf = m;
  for (uint32_t base = 0; base < m; base += 64u) {
    const uint32_t x = base + lane;
    const unsigned long long bal = __ballot(x < m && A[x] != B[x]);
    if (bal) { pre = base + (uint32_t)__ffsll((long long)bal) - 1u; break; }
  }
  for (uint32_t base = 0; base < m; base += 64u) {
    const uint32_t x = base + lane;
    const unsigned long long bal = __ballot(x < m && A[la - 1u - x] != B[lb - 1u - x]);
    if (bal) { suf = base + (uint32_t)__ffsll((long long)bal) - 1u; break; }
  }
  // ---- longest common substring: a lane per diagonal ----
  uint32_t lcs = 0;
  for (uint32_t dg = lane; dg < la + lb - 1u; dg += 64u) {
    const int delta = (int)dg - (int)la + 1;
    const int i0 = delta < 0 ? -delta : 0, i1 = min((int)la, (int)lb - delta);
    if (i1 - i0 <= (int)lcs) continue;
    uint32_t run = 0;
    for (int i = i0; i < i1; ++i) {
      run = A[i] == B[i + delta] ? run + 1u : 0u;
      lcs = max(lcs, run);
    }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) lcs = max(lcs, (uint32_t)__shfl_xor((int)lcs, o));
  // ---- Damerau-Levenshtein: strips of 64 rows, lane = row of the strip, step t: column j = t - lane + 1 ----
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t s0 = 0; s0 < la; s0 += 64u) {
    const uint32_t i = s0 + lane + 1u, nrows = min(64u, la - s0);
    const bool rowok = lane < nrows;
    const uint32_t ai = rowok ? (uint32_t)A[i - 1u] : 0xFFFFu;
    // the strip's rows per column: one ballot per column, kept by the lane of that column, stored 64 at a time
    for (uint32_t c0 = 0; c0 < lb; c0 += 64u) {
      const uint32_t bk = c0 + lane < lb ? (uint32_t)B[c0 + lane] : 0x1FFFFu;
      const uint32_t cnt = min(64u, lb - c0);
      unsigned long long mk = 0;
      for (uint32_t jl = 0; jl < cnt; ++jl) {
        const uint32_t bv = (uint32_t)__builtin_amdgcn_readlane((int)bk, (int)jl);
        const unsigned long long hit = __ballot(ai == bv);
        mk = lane == jl ? hit : mk;
      }
      if (c0 + lane < lb) s_mask[c0 + lane] = mk;
    }
    __syncthreads();
    uint32_t left = i, diag = i - 1u, db = 0, cur = 0;
    const uint32_t steps = lb + nrows - 1u;
    for (uint32_t t = 0; t < steps; ++t) {
      const int j = (int)t - (int)lane + 1;
      const bool active = rowok && j >= 1 && j <= (int)lb;
      uint32_t up = (uint32_t)__shfl_up((int)cur, 1);  // D[i - 1][j]: what the lane above computed a step ago
      if (active) {
        const uint32_t ju = (uint32_t)j;
        if (lane == 0u) up = s0 == 0u ? ju : mat[(s0 - 1u) * S + (ju - 1u)];  // the last row of the strip above, or row 0
        const uint32_t bj = B[ju - 1u];
        const bool eq = ai == bj;
        uint32_t v = min(min(left, up) + 1u, diag + (eq ? 0u : 1u));
        if (db) {
          const unsigned long long mm = s_mask[ju - 1u] & below;
          const uint32_t last = mm ? s0 + 64u - (uint32_t)__clzll((long long)mm) : (uint32_t)s_tab[bj];
          if (last) {  // D[last - 1][db - 1]: a boundary cell when either index is 0
            const uint32_t r = last - 1u, c = db - 1u;
            const uint32_t src = r == 0u ? c : c == 0u ? r : mat[(r - 1u) * S + (c - 1u)];
            v = min(v, src + (i - last - 1u) + 1u + (ju - db - 1u));
          }
        }
        mat[(i - 1u) * S + (ju - 1u)] = (uint8_t)v;
        if (eq) db = ju;
        diag = up;
        left = v;
        cur = v;
      }
      __syncthreads();  // (one wave: orders this step's cells before the reads of the next)
    }
    // the strip's rows enter the per-symbol table: of several rows with one symbol the last
    bool superseded = false;
    for (uint32_t l = 1; l < nrows; ++l) {
      const uint32_t av = (uint32_t)__builtin_amdgcn_readlane((int)ai, (int)l);
      superseded = superseded || (l > lane && av == ai);
    }
    if (rowok && !superseded) s_tab[ai & 0xFFu] = (uint8_t)i;
    __syncthreads();
  }
  if (lane == 0u) {
    const uint32_t ld = mat[(la - 1u) * S + (lb - 1u)];
    const uint32_t samecase = ((ma >> 24) & 1u) == ((mb >> 24) & 1u) ? 1u : 0u;
    pair_store(k.out + p, pair_score(k, la, ld, lcs, pre, suf, samecase), ld, lcs, pre, suf, la, lb, samecase, ANX_OK);
  }
}

// ---- host driver --------------------------------------------------------------------------------------------------------------------
namespace {
std::atomic<uint64_t> g_cf_seen{0}, g_cf_screened{0}, g_cf_scripts{0}, g_cf_host{0};

// weight[i] on the host for the pairs `pick` selects: HostModel::confusable_weight_text, on up to 16 threads when there are many
template <typename Pick>
uint64_t weight_on_host(const HostModel& m, const PairSpan* a, const PairSpan* b, size_t n, double* weight, Pick pick) {
  std::vector<uint32_t> todo;
  for (size_t i = 0; i < n; ++i)
    if (pick(i)) todo.push_back((uint32_t)i);
  auto work = [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const uint32_t i = todo[k];
      weight[i] = m.confusable_weight_text(a[i].p, a[i].len, b[i].p, b[i].len);
    }
  };
  const size_t nt = todo.size() < 4096 ? 1 : std::min<size_t>(16, std::max(1u, usable_hw_threads()));
  if (nt <= 1) work(0, todo.size());
  else {
    std::vector<std::thread> th;
    const size_t per = (todo.size() + nt - 1) / nt;
    for (size_t t = 0; t < nt; ++t) th.emplace_back(work, std::min(todo.size(), t * per), std::min(todo.size(), (t + 1) * per));
    for (std::thread& t : th) t.join();
  }
  return todo.size();
}
}  // namespace

void pairs_conf_stats(uint64_t out[4]) {
  out[0] = g_cf_seen.load(std::memory_order_relaxed); out[1] = g_cf_screened.load(std::memory_order_relaxed);
  out[2] = g_cf_scripts.load(std::memory_order_relaxed); out[3] = g_cf_host.load(std::memory_order_relaxed);
}

// Staging, the upload, the encoder and the pair kernels of one chunk, enqueued on sc.st (engine_internal.h): what score_pairs_chunk
// downloads, and what eval.hip (anx_evaluate_gold) reads where it lies.
int pairs_chunk_enqueue(const HostModel& m, const DeviceLexicon* dl, const PairSpan* a, const PairSpan* b, size_t n, const anx_params* thr, PairScratch& sc,
                        PairsOnDevice& pd, std::string& err) {
  const size_t N2 = 2 * n;
  size_t text = 0;
  for (size_t i = 0; i < n; ++i) text += a[i].len + b[i].len + 2;
  if (text + 4 * N2 + 16 >= ((size_t)1 << 32)) { err = "pairs exceed 4 GB of text per 2^20 pairs (bytes + 4 per string)"; return ANX_ELIMIT; }
  hipStream_t st = sc.st;
  // ---- one staging block: offsets [2 n + 1] | tier lists [n] (short pairs from the front, long ones from the back) | the blob ----
  const size_t o_idx = (N2 + 1) * sizeof(uint32_t), o_blob = (o_idx + n * sizeof(uint32_t) + 15) & ~(size_t)15, in_bytes = o_blob + text + 16;
  char* h_in = static_cast<char*>(sc.pinned(in_bytes));
  if (!h_in) { err = "out of host memory"; return ANX_EINVAL; }
  uint32_t* h_off = reinterpret_cast<uint32_t*>(h_in);
  uint32_t* h_idx = reinterpret_cast<uint32_t*>(h_in + o_idx);
  char* h_blob = h_in + o_blob;
  uint32_t nshort = 0, nlong = 0;
  size_t long_max = 0;  // the longest side (bytes) of a long pair that can be scored at all
  {
    size_t pos = 0;
    for (size_t s = 0; s < N2; ++s) {
      const PairSpan& sp = s < n ? a[s] : b[s - n];
      h_off[s] = (uint32_t)pos;
      if (sp.len) memcpy(h_blob + pos, sp.p, sp.len);
      h_blob[pos + sp.len] = '\0';
      pos += sp.len + 1;
    }
    h_off[N2] = (uint32_t)pos;
    memset(h_blob + pos, 0, 16);  // (the encoder's window reads whole dwords)
    for (size_t i = 0; i < n; ++i) {
      if (a[i].len <= PAIRS_SHORT_BYTES && b[i].len <= PAIRS_SHORT_BYTES) h_idx[nshort++] = (uint32_t)i;
      else {
        h_idx[n - 1 - nlong++] = (uint32_t)i;
        if (a[i].len && b[i].len) long_max = std::max(long_max, std::max(a[i].len, b[i].len));
      }
    }
  }
  // ---- device buffers ----
  const int NP = dl->nplanes;
  char* d_in = nullptr;
  SmallEnc e{};
  anx_pair_score* d_out = nullptr;
  int rc;
  if ((rc = sc.get(&d_in, in_bytes, err)) || (rc = sc.get(&e.codes, text + 4 * N2 + 16, err)) || (rc = sc.get(&e.meta, N2, err)) ||
      (rc = sc.get(&e.bits, N2 * NBITPLANES, err)) || (rc = sc.get(&e.kind, N2, err)) || (rc = sc.get(&e.cv, N2 * (size_t)NP, err)) ||
      (rc = sc.get(&e.key, N2, err)) || (rc = sc.get(&e.sig, N2, err)) || (rc = sc.get(&e.blk, 3 * ((N2 + 255) / 256), err)) ||
      (rc = sc.get(&d_out, n, err)))
    return rc;
  HIP_TRY(hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, st));
  const uint32_t* d_off = reinterpret_cast<const uint32_t*>(d_in);
  const uint32_t* d_idx = reinterpret_cast<const uint32_t*>(d_in + o_idx);
  if ((rc = thr ? pairs_encode_launch_thr(m, dl, e, reinterpret_cast<const uint8_t*>(d_in + o_blob), d_off, (uint32_t)N2, *thr, st, err)
                : pairs_encode_launch(m, dl, e, reinterpret_cast<const uint8_t*>(d_in + o_blob), d_off, (uint32_t)N2, st, err)))
    return rc;
  PairKArgs k{};
  k.n = (uint32_t)n; k.off = d_off; k.codes = e.codes; k.meta = e.meta; k.out = d_out; k.quot = dl->quot;
  k.w_ld = m.weights.ld; k.w_lcs = m.weights.lcs; k.w_prefix = m.weights.prefix; k.w_suffix = m.weights.suffix; k.w_case = m.weights.casew;
  k.w_sum = m.weights.ld + m.weights.lcs + m.weights.prefix + m.weights.suffix + m.weights.casew;  // src/types.rs:69-73, as launch_plan.hpp
  if (nshort) {
    k.idx = d_idx; k.count = nshort;
    const int kt = ktimer_begin("k_pairs_short", st);
    hipLaunchKernelGGL(k_pairs_short, dim3((nshort + PS_THREADS - 1) / PS_THREADS), dim3(PS_THREADS), 0, st, k);
    ktimer_end(kt, st);
  }
  if (nlong) {
    k.idx = d_idx + (n - nlong); k.count = nlong;
    const int kt = ktimer_begin("k_pairs_long", st);
    if (long_max <= 64) hipLaunchKernelGGL(k_pairs_long<64>, dim3(nlong), dim3(64), 0, st, k);
    else hipLaunchKernelGGL(k_pairs_long<255>, dim3(nlong), dim3(64), 0, st, k);
    ktimer_end(kt, st);
  }
  HIP_TRY(hipGetLastError());
  pd.blob = reinterpret_cast<const uint8_t*>(d_in + o_blob); pd.off = d_off; pd.e = e; pd.out = d_out;
  return ANX_OK;
}

int score_pairs_chunk(const HostModel& m, const DeviceLexicon* dl, const PairSpan* a, const PairSpan* b, size_t n, anx_pair_score* out, std::string& err,
                      double* weight) {
  if (n == 0) return ANX_OK;
  if (!dl) { err = "model is not resident on a device"; return ANX_ENODEVICE; }
  if (n > PAIRS_CHUNK) { err = "score_pairs_chunk: more than 2^20 pairs"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(dl->device));
  PairScratch sc(dl->device);
  hipStream_t st = sc.st;
  PairsOnDevice pd;
  int rc;
  if ((rc = pairs_chunk_enqueue(m, dl, a, b, n, nullptr, sc, pd, err))) return rc;
  anx_pair_score* d_out = pd.out;
  anx_pair_score* h_out = static_cast<anx_pair_score*>(sc.pinned(n * sizeof(anx_pair_score)));
  if (!h_out) { err = "out of host memory"; return ANX_EINVAL; }
  // ---- confusable weights: on the device unless the model has no list, the switch says host, or the working set finds no room ----
  const bool weigh = weight && !m.confusables.empty();
  bool on_device = weigh && !switches().confusables_host;
  PairConfRun cr{};
  double* h_w = nullptr;  // [n] weights | 16 bytes of counters
  if (on_device) {
    cr.work_blocks = std::min<uint32_t>(PAIRS_CF_BLOCKS, (uint32_t)((n + 63) / 64));
    void* wk = nullptr;
    if (pool_malloc(&wk, conf_small_work_bytes(cr.work_blocks)) != hipSuccess) {
      (void)hipGetLastError();
      on_device = false;  // (same weights from the host)
    } else {
      sc.blocks.v.push_back(wk);
      cr.work = static_cast<uint32_t*>(wk);
      char* tmp = nullptr;
      cr.sort_tmp_bytes = conf_pairs_sort_tmp_bytes((uint32_t)n);
      if ((rc = sc.get(&cr.weight, n + 2, err)) || (rc = sc.get(&cr.need, n, err)) || (rc = sc.get(&cr.sort, 3 * n, err)) ||
          (rc = sc.get(&tmp, cr.sort_tmp_bytes, err)))
        return rc;
      cr.sort_tmp = tmp;
      cr.ctr = reinterpret_cast<uint32_t*>(cr.weight + n);
      h_w = static_cast<double*>(sc.pinned((n + 2) * sizeof(double)));
      if (!h_w) { err = "out of host memory"; return ANX_EINVAL; }
    }
  }
  if (on_device) {
    cr.n = (uint32_t)n; cr.blob = pd.blob; cr.off = pd.off; cr.rec = d_out;
    if ((rc = conf_launch_pairs(m, dl, st, cr, err))) return rc;
  }
  HIP_TRY(hipMemcpyAsync(h_out, d_out, n * sizeof(anx_pair_score), hipMemcpyDeviceToHost, st));
  if (on_device) HIP_TRY(hipMemcpyAsync(h_w, cr.weight, (n + 2) * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  memcpy(out, h_out, n * sizeof(anx_pair_score));
  if (!weight) return ANX_OK;
  g_cf_seen.fetch_add(n, std::memory_order_relaxed);
  if (!weigh) {
    std::fill(weight, weight + n, 1.0);
  } else if (on_device) {
    memcpy(weight, h_w, n * sizeof(double));
    uint32_t ctr[4];
    memcpy(ctr, h_w + n, sizeof(ctr));
    const uint64_t listed = std::min<uint64_t>(ctr[0], n);
    const uint64_t fell = ctr[1] ? weight_on_host(m, a, b, n, weight, [&](size_t i) { return std::isnan(weight[i]); }) : 0;
    g_cf_screened.fetch_add(n - listed, std::memory_order_relaxed);
    g_cf_scripts.fetch_add(listed - std::min(listed, fell), std::memory_order_relaxed);
    g_cf_host.fetch_add(fell, std::memory_order_relaxed);
  } else {
    std::fill(weight, weight + n, 1.0);
    g_cf_host.fetch_add(weight_on_host(m, a, b, n, weight, [&](size_t i) { return out[i].status == 0; }), std::memory_order_relaxed);
  }
  return ANX_OK;
}

}  // namespace anx
