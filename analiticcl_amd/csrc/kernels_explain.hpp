// kernels_explain.hpp -- anx_batch_fetch_measures: the measures behind every ranked row of a resident batch ("explain").
// Part of the single translation unit engine.hip (included inside namespace anx); gfx950 only.
//
// A ranked row (DevRow in Batch::r_rows) names a vocabulary item and, for rows reached through a variant list, the item that was
// actually scored (`via`: the survivor itself, k_compact).  These kernels join the row with what is resident anyway -- the query's
// symbols and meta word, the scored entry's symbols, meta word and anagram class -- and write one 16-byte anx_row_measures per row
// where the compact fetch puts the row (input order: off_orig[q_orig[s]] + rank):
//   k_vocab_entry_scatter : once per replica: vocabulary id -> lexicon entry (0xFFFFFFFF: the item is not indexed)
//   k_row_measures        : FLAT over the row slots, the lanes of a wave on consecutive 24-byte rows; a lane finds its query by binary
//                           search in soff (as k_eval_rows, eval.hip), resolves the scored entry and, when both sides have at most 16
//                           symbols, settles the row from the two 16-byte records q_rec[s][0] / e_rec[e][0] (a 16 x 16 byte matrix per
//                           lane in LDS); longer rows go to a dense list, one reservation per wave
//   k_row_measures_long   : one wave per listed row, up to 255 symbols a side, the matrix in LDS; a fixed grid strides over the
//                           device-side list length (no host round trip between the two kernels).  A listed row's record holds
//                           {query, entry, L1, via} in the meantime, so this kernel neither searches nor resolves again
// The distance is the UNRESTRICTED Damerau-Levenshtein of pairs.hip (byte cells, "no earlier occurrence" tested rather than stored,
// row stride 5 mod 8 in the long form) restated here: no code is shared with pairs.hip, whose kernels keep their ISA metadata.  It is
// exact for any d a caller can set, unlike the D-templated diagonals of kernels_score.hpp.  Every measure is computed whatever its
// weight; the score restates score_finish term by term (same association, DeviceLexicon::quot for x, L <= 32, the w_sum == 1.0
// shortcut, input_length = the symbols of the input) without the confusable weight and without the variant score.
// The anagram distance is the L1 of the two packed count vectors (NP x v_sad_u8): the entry's words come from cls_planes through
// scan_rec[e]'s class, the query's from q_cv or -- where the encoder left only thermometer planes -- from the planes.
#pragma once

constexpr uint32_t XM_NONE = 0xFFFFFFFFu;
constexpr uint32_t XM_THREADS = 128;      // k_row_measures: lanes per block
constexpr uint32_t XM_STRIDE = 73;        // dwords per lane: 64 of the matrix, 4 + 4 of the strings, one more for an odd stride (conflict-free)
constexpr uint32_t XM_ML = 255;           // most symbols a side
constexpr uint32_t XM_S = 261;            // row stride of the long matrix in bytes: 5 mod 8
constexpr uint32_t XM_LONG_BLOCKS = 512;  // one-wave blocks of k_row_measures_long (69 KB of LDS each: two per CU)
static_assert(XM_S >= XM_ML && XM_S % 8u == 5u, "row stride");

__global__ __launch_bounds__(256) void k_vocab_entry_scatter(uint32_t nentries, const uint32_t* __restrict__ ent_vocab, uint32_t V,
                                                             uint32_t* __restrict__ vocab_ent) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nentries) return;
  const uint32_t v = ent_vocab[e];
  if (v < V) vocab_ent[v] = e;
}

struct ExplainArgs {
  uint32_t nq, total;               // queries; row slots (soff[nq] as the host read it back)
  uint32_t V, nentries, qw, cstride, n_out;  // n_out: records in out
  int NP, bits_ok;                  // count-vector dwords; the encoder made thermometer planes (nsym <= 32)
  const uint32_t *soff, *r_count, *q_orig, *off_orig, *q_meta;
  const DevRow* r_rows;
  const uint4 *q_rec, *q_rows, *q_bits;
  const uint32_t* q_cv;
  const uint32_t* vocab_ent;        // [V] vocabulary id -> entry
  const uint4 *e_rec, *scan_rec, *rows;
  const uint32_t* cls_planes;
  const double* quot;               // [33][33] x / L as the host divides, or nullptr
  double w_ld, w_lcs, w_prefix, w_suffix, w_case, w_sum;
  uint4* out;                       // [n_results] anx_row_measures, input order
  uint32_t* list;                   // records (positions in out) left to k_row_measures_long
  uint32_t* list_n;
};

struct XmRow { uint32_t s, e, dst, qm, em, cls, via; };

// the row in slot p: its query (the last s with soff[s] <= p), its scored entry and where its record goes; false: the slot holds no ranked row
__device__ inline bool xm_resolve(const ExplainArgs& k, uint32_t p, XmRow& r) {
  uint32_t lo = 0, hi = k.nq - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (k.soff[mid] <= p) lo = mid;
    else hi = mid - 1u;
  }
  const uint32_t s0 = k.soff[lo];
  if (s0 > p || p - s0 >= k.r_count[lo]) return false;
  const uint2 head = *reinterpret_cast<const uint2*>(&k.r_rows[p]);  // {vocab_id, via}
  const uint32_t item = head.y != XM_NONE ? head.y : head.x;
  uint32_t e = item < k.V ? k.vocab_ent[item] : XM_NONE;
  if (e >= k.nentries) e = XM_NONE;
  r.s = lo;
  r.e = e;
  r.dst = k.off_orig[k.q_orig[lo]] + (p - s0);
  if (r.dst >= k.n_out) return false;  // (the offsets are the scan of these very counts: cannot happen)
  r.qm = k.q_meta[lo];
  r.via = head.y != XM_NONE ? 1u : 0u;
  r.em = 0u;
  r.cls = 0u;
  if (e != XM_NONE) {
    r.em = k.e_rec[2 * (size_t)e + 1].x;
    r.cls = k.scan_rec[e].w;
  }
  return true;
}
// dword w of the query's count vector (4 symbol slots, a byte each): from q_cv where the encoder wrote it (a symbol five times or
// more, or no planes at all), else from the thermometer planes (counts <= 4: the planes' bits add up to the length exactly then)
__device__ inline bool xm_query_has_cv(const ExplainArgs& k, const uint4 pl, uint32_t la) {
  return !k.bits_ok || (uint32_t)(__popc(pl.x) + __popc(pl.y) + __popc(pl.z) + __popc(pl.w)) != la;
}
__device__ inline uint32_t xm_query_word(const ExplainArgs& k, uint32_t s, bool has_cv, const uint4 pl, uint32_t w) {
  if (has_cv) return k.q_cv[(size_t)s * (size_t)k.NP + w];
  uint32_t word = 0;
  if (w < 8u) {
#pragma unroll
    for (uint32_t y = 0; y < 4u; ++y) {
      const uint32_t sl = 4u * w + y;
      word |= (((pl.x >> sl) & 1u) + ((pl.y >> sl) & 1u) + ((pl.z >> sl) & 1u) + ((pl.w >> sl) & 1u)) << (8u * y);
    }
  }
  return word;
}
// src/lib.rs:1433-1452 with input_length = la, as score_finish (kernels_score.hpp) writes it
__device__ inline double xm_score(const ExplainArgs& k, uint32_t la, uint32_t ld, uint32_t lcs, uint32_t pre, uint32_t suf, uint32_t samecase) {
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
// the 16-byte record as one store
__device__ inline void xm_store(uint4* o, double score, uint32_t ld, uint32_t lcs, uint32_t pre, uint32_t suf, uint32_t la, uint32_t lb, uint32_t l1,
                                uint32_t flags) {
  const unsigned long long sb = (unsigned long long)__double_as_longlong(score);
  *o = make_uint4((uint32_t)sb, (uint32_t)(sb >> 32), ld | lcs << 8 | pre << 16 | suf << 24, la | lb << 8 | min(l1, 255u) << 16 | flags << 24);
}
__device__ inline uint32_t xm_flags(const XmRow& r) { return ((((r.qm >> 24) & 1u) == ((r.em >> 8) & 1u)) ? 1u : 0u) | r.via << 1; }

__global__ __launch_bounds__(XM_THREADS) void k_row_measures(ExplainArgs k) {
  __shared__ uint32_t s_all[XM_THREADS * XM_STRIDE];
  const uint32_t p = blockIdx.x * XM_THREADS + threadIdx.x;  // (no barrier below)
  const uint32_t lane = threadIdx.x & 63u;
  XmRow r{};
  const bool live = p < k.total && p < k.soff[k.nq] && xm_resolve(k, p, r);
  const uint32_t la = live ? r.qm & 0xFFu : 0u, lb = live ? r.em & 0xFFu : 0u;
  const bool known = live && r.e != XM_NONE;
  if (live && !known) xm_store(k.out + r.dst, 0.0, 0u, 0u, 0u, 0u, la, 0u, 0u, r.via << 1);  // (an id without an entry: cannot happen for a ranked row)
  const bool is_long = known && (la > 16u || lb > 16u);
  // L1 of the two count vectors
  uint32_t l1 = 0;
  if (known) {
    const uint4 pl = k.q_bits[r.s];
    const bool has_cv = xm_query_has_cv(k, pl, la);
    for (uint32_t w = 0; w < (uint32_t)k.NP; ++w)
      l1 = __builtin_amdgcn_sad_u8(xm_query_word(k, r.s, has_cv, pl, w), k.cls_planes[(size_t)w * k.cstride + r.cls], l1);
  }
  {  // long rows: one reservation per wave; the row's record holds {query, entry, L1, via} until k_row_measures_long overwrites it
    const unsigned long long bal = __ballot(is_long);
    if (bal) {
      const uint32_t leader = (uint32_t)__ffsll((long long)bal) - 1u;
      uint32_t base = 0;
      if (lane == leader) base = atomicAdd(k.list_n, (uint32_t)__popcll(bal));
      base = (uint32_t)__shfl((int)base, (int)leader);
      if (is_long) {
        k.list[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = r.dst;
        k.out[r.dst] = make_uint4(r.s, r.e, l1, r.via);
      }
    }
  }
  if (!known || is_long) return;
  uint32_t* mine = s_all + threadIdx.x * XM_STRIDE;
  uint8_t* M = reinterpret_cast<uint8_t*>(mine);             // D[i][j] at (i - 1) * 16 + (j - 1), 1 <= i, j <= 16
  const uint8_t* A = reinterpret_cast<const uint8_t*>(mine + 64);
  const uint8_t* B = reinterpret_cast<const uint8_t*>(mine + 68);
  {
    const uint4 qa = k.q_rec[2 * (size_t)r.s], eb = k.e_rec[2 * (size_t)r.e];
    mine[64] = qa.x; mine[65] = qa.y; mine[66] = qa.z; mine[67] = qa.w;
    mine[68] = eb.x; mine[69] = eb.y; mine[70] = eb.z; mine[71] = eb.w;
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
        const uint32_t rr = last - 1u, c = db - 1u;
        const uint32_t src = rr == 0u ? c : c == 0u ? rr : M[(rr - 1u) * 16u + (c - 1u)];
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
  const uint32_t flags = xm_flags(r);
  xm_store(k.out + r.dst, xm_score(k, la, ld, lcs, pre, suf, flags & 1u), ld, lcs, pre, suf, la, lb, l1, flags);
}

// one wave per listed row: the lanes run along the anti-diagonal of a strip of 64 rows (k_pairs_long, pairs.hip)
__global__ __launch_bounds__(64) void k_row_measures_long(ExplainArgs k) {
  constexpr uint32_t S = XM_S;
  __shared__ unsigned long long s_mask[XM_ML + 1];          // per column of b: the rows of the current strip (bit = lane) whose symbol equals it
  __shared__ uint32_t s_mat32[(XM_ML * XM_S + 3u) / 4u];    // D[i][j] at (i - 1) * S + (j - 1)
  __shared__ uint32_t s_a32[(XM_ML + 3u) / 4u], s_b32[(XM_ML + 3u) / 4u];
  __shared__ uint8_t s_tab[256];                            // per symbol code: its last row above the current strip (0: none)
  uint8_t* mat = reinterpret_cast<uint8_t*>(s_mat32);
  const uint8_t* A = reinterpret_cast<const uint8_t*>(s_a32);
  const uint8_t* B = reinterpret_cast<const uint8_t*>(s_b32);
  const uint32_t lane = threadIdx.x;
  const uint32_t nlist = min(*k.list_n, k.total);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t li = blockIdx.x; li < nlist; li += gridDim.x) {  // block-uniform
    __syncthreads();  // (the row before this one has been read out of LDS)
    const uint32_t dst = k.list[li];
    if (dst >= k.n_out) continue;
    const uint4 parked = k.out[dst];  // {query, entry, L1, via}: what k_row_measures left (block-uniform)
    if (parked.x >= k.nq || parked.y >= k.nentries) continue;  // (cannot happen: only resolved rows are listed)
    XmRow r{};
    r.qm = k.q_meta[parked.x];
    const uint4 e1 = k.e_rec[2 * (size_t)parked.y + 1];  // {meta, row offset, freq, 0}
    r.em = e1.x;
    r.via = parked.w & 1u;
    const uint32_t l1 = parked.z;
    const uint32_t la = r.qm & 0xFFu, lb = r.em & 0xFFu;
    if (la == 0u || lb == 0u) continue;
    {
      const uint32_t* ca = reinterpret_cast<const uint32_t*>(k.q_rows + (size_t)parked.x * k.qw);
      const uint32_t* cb = reinterpret_cast<const uint32_t*>(k.rows + e1.y);
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
              const uint32_t rr = last - 1u, c = db - 1u;
              const uint32_t src = rr == 0u ? c : c == 0u ? rr : mat[(rr - 1u) * S + (c - 1u)];
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
      const uint32_t flags = xm_flags(r);
      xm_store(k.out + dst, xm_score(k, la, ld, lcs, pre, suf, flags & 1u), ld, lcs, pre, suf, la, lb, l1, flags);
    }
  }
}
