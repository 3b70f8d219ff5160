// csweep.hip -- anx_evaluate_sweep_confusables: candidate confusable patterns with one weight per pattern and set, swept over gold pairs
// WITHOUT a model, a batch run or an edit script per set (gfx950 / CDNA4).
//
// The candidates of an input are fixed by k, d and StopAtExactMatch; their measures and their unweighted scores by the model's score
// weights; whether pattern j is found in the edit script of (input, candidate) by the two texts.  The list's weights enter as a product
// over the matching patterns in list order (src/lib.rs:1743-1752), applied to the kept rows before the sort (early, :1505-1508) or to
// the cropped list before a re-sort and the cutoff (late, :1591-1622).  So on the chunk's device:
//   once per group (csweep_group_begin), behind reweigh.hip's base rows (k_rw_base / k_rw_pre, shared, not copied):
//     k_cs_score    : flat over the rows: the f64 score under the model's weights (rw_score, reweigh_shared.hpp), stored once
//     k_cs_ranges   : flat over the rows: where every pair's rows begin and end (the late weight kernel looks a ranked row up there)
//     k_cs_inbits   : a lane per pair: the ASCII presence bits of the input from its bytes, and whether the bytes are well-formed
//     k_cs_screen   : flat over the rows, on presence bits alone (k_pairs_conf_screen's two looks, the candidate's side from the
//                     vocabulary copy): a row no pattern can match gets mask 0, the others a place in a dense list with the shape key of
//                     their script; ONE reservation per wave
//     the radix pass of conf.hip over the shape keys (conf_sort_enqueue)
//     k_cs_mask_*   : one lane per listed row in shape-key order, the lane memories of a wave interleaved (conf_lane.hpp), at most
//                     CF_BLOCKS one-wave blocks, in passes of four kernels -- prep (the input decoded from the pair side's blob, the
//                     candidate from the vocabulary copy, mask_live), diff, clean, find (confusables_core.hpp confusable_mask's steps)
//                     -> one uint64_t; a row the lane memory cannot hold is listed for the host
//     one wait; the host computes the listed rows' masks with the same body and patches them in
//   once per set (csweep_group_set), no edit script, no host round trip before the download:
//     k_cs_count    : rows with score >= score_threshold per pair -- the UNWEIGHTED score in both modes (:1475 precedes :1506)
//     the exclusive scan (prefix_scan_enqueue)
//     k_cs_fill     : the kept rows as SurvRow; early: score * w(mask, set)
//     k_rank        : engine.hip's kernel (rank_rows_enqueue); late: without a cutoff, as the batch path ranks before k_conf_apply_late
//     k_cs_slot_w   : late: the weight of every ranked slot, the base row found by its vocabulary id in the pair's range of base rows
//     k_conf_apply_late : conf.hip's kernel (conf_apply_late_enqueue): multiply, stable re-sort, cutoff -- not restated
//     k_rw_classify : reweigh.hip's kernel (reweigh_group_finish) with the model's weights: THRESHOLD from the direct pair's unweighted
//                     score, the top row's weighted dist_score, the integer reduction; 624 bytes down (+ 32 n with the records)
// The front of a late set -- k_cs_count .. k_rank -- is also csweep_group_rank_late's: the confusable fit (fit.hip) cuts its state from
// the unweighted cropped lists and runs neither k_cs_slot_w nor k_conf_apply_late on them.
// w(mask, set) = 1.0 times the set's weights of the set bits in ascending pattern order, f64, -ffp-contract=off; the set's weights reach
// the lanes through LDS.  Every append is bounds-checked against the scan's own offsets and the row capacity.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "engine_internal.h"
#include "conf_lane.hpp"
#include "csweep.h"

namespace anx {

#include "kernels_common.hpp"
#include "kernels_gold.hpp"
#include "gold_host.hpp"
#include "reweigh_shared.hpp"

namespace {
std::atomic<uint64_t> g_stats[CS_NSTATS];
}  // namespace

void csweep_stats_add(int which, uint64_t v) {
  if (which >= 0 && which < CS_NSTATS) g_stats[which].fetch_add(v, std::memory_order_relaxed);
}
void csweep_stats(uint64_t out[CS_NSTATS]) {
  for (int i = 0; i < CS_NSTATS; ++i) out[i] = g_stats[i].load(std::memory_order_relaxed);
}

constexpr uint32_t CS_MAXP = 64;         // patterns per call: the bits of a mask
constexpr uint32_t CS_IN_BAD = 2u;       // CharSet::other of an input: bit 0 a non-ASCII byte, bit 1 malformed UTF-8 (pairs_side_bits)
constexpr uint32_t CS_KEY_LAST = 0x1B7Fu;  // the largest shape key: where a row with malformed input bytes is put

// ---- once per group -------------------------------------------------------------------------------------------------------------------
struct CsScoreArgs {
  uint32_t n, R;
  const uint4* info;
  const uint2* meas;
  RwWeights w;                   // the model's
  double* score;                 // [R]
  uint32_t *rbeg, *rend;         // [n] the pair's base rows (cleared before)
};
__global__ __launch_bounds__(GOLD_BLOCK) void k_cs_score(CsScoreArgs k) {
  const uint32_t r = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  if (r >= k.R) return;
  double s = 0.0;
  if (k.info[r].x < k.n) {
    const uint2 m = k.meas[r];
    s = rw_score(k.w, m.y & 0xFFu, m.x & 0xFFu, (m.x >> 8) & 0xFFu, (m.x >> 16) & 0xFFu, m.x >> 24, (m.y >> 8) & 1u);
  }
  k.score[r] = s;
}
// a pair's rows lie side by side (one section, one run of its offsets): the first row of a run writes where it begins, the last where it ends
__global__ __launch_bounds__(GOLD_BLOCK) void k_cs_ranges(CsScoreArgs k) {
  const uint32_t r = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  if (r >= k.R) return;
  const uint32_t pair = k.info[r].x;
  if (pair >= k.n) return;
  if (r == 0u || k.info[r - 1u].x != pair) k.rbeg[pair] = r;
  if (r + 1u == k.R || k.info[r + 1u].x != pair) k.rend[pair] = r + 1u;
}

struct CsMaskArgs {
  uint32_t n, R;
  const uint4* info;               // [R] {pair, ., ., vocabulary id}
  const uint8_t* blob;             // the chunk's strings: input i = blob[off[i] .. off[i + 1] - 1)
  const uint32_t* off;
  cdiff::CharSet* in_cs;           // [n]
  cdiff::Patterns P;
  const uint32_t* v_pool; const uint32_t* v_off; const cdiff::CharSet* v_cs; uint32_t nvocab;
  const uint32_t (*alpha)[2]; uint32_t nalpha;
  unsigned long long* mask;        // [R]
  uint32_t* list;                  // [R] the rows that need an edit script
  uint32_t* key;                   // [R] shape key per list entry, preset to all ones behind the list
  const uint32_t* sorted;          // [R] the list in shape-key order
  uint32_t* hostrows;              // [R] rows left to the host
  uint32_t* ctr;                   // [0] list length, [1] rows left to the host
  uint32_t* work;                  // [blocks][CF_WORDS][64]
};
__global__ __launch_bounds__(GOLD_BLOCK) void k_cs_inbits(CsMaskArgs a) {
  const uint32_t i = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  cdiff::CharSet cs;
  const bool bad = pairs_side_bits(a.blob, a.off[i], a.off[i + 1u] - 1u, cs);
  if (bad) cs.other |= CS_IN_BAD;
  a.in_cs[i] = cs;
}

// One lane per base row: k_pairs_conf_screen's two looks -- the presence bits of the whole strings, then of the middles (what is left
// between the common ASCII prefix and suffix) -- with the input's side from its bytes and the candidate's from the vocabulary copy.
// Necessary conditions of found_in only: a row that passes is decided by the mask pass.
__global__ __launch_bounds__(GOLD_BLOCK) void k_cs_screen(CsMaskArgs a) {
  const uint32_t r = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  bool need = false;
  uint32_t key = CS_KEY_LAST;
  if (r < a.R) {
    const uint4 inf = a.info[r];
    const uint32_t i = inf.x, id = inf.w;
    if (i < a.n && id < a.nvocab) {
      const cdiff::CharSet ins = a.in_cs[i], cs = a.v_cs[id];
      const bool in_other = (ins.other & 1u) != 0u, forced = (ins.other & CS_IN_BAD) != 0u;  // malformed bytes: the mask kernel decides
      need = forced;
      for (uint32_t j = 0; j < a.P.nconf && !need; ++j) {
        const cdiff::FlatConf& cf = a.P.conf[j];
        bool may = true;
        for (uint32_t o_ = 0; o_ < cf.nops && may; ++o_) {
          const cdiff::FlatOp& o = a.P.ops[cf.op_begin + o_];
          const bool tail = cf.strictend && o_ == cf.nops - 1 && o.op != '=';
          if (o.simple && !tail) {
            uint64_t h0 = o.bits[0], h1 = o.bits[1];
            if (o.op != '+') { h0 &= ins.w[0]; h1 &= ins.w[1]; }
            if (o.op != '-') { h0 &= cs.w[0]; h1 &= cs.w[1]; }
            if (!(h0 | h1)) may = false;
          } else if (!o.simple) {
            uint64_t s0 = ~0ull, s1 = ~0ull;
            bool other = true;
            if (o.op != '+') { s0 &= ins.w[0]; s1 &= ins.w[1]; other = other && in_other; }
            if (o.op != '-') { s0 &= cs.w[0]; s1 &= cs.w[1]; other = other && cs.other; }
            may = pairs_opt_may(a.P, o, s0, s1, other);
          }
        }
        need = may;
      }
      if (need && !forced) {  // the middles: prefix and suffix on the input's bytes, stopping at the first non-ASCII byte
        const uint32_t t0 = a.off[i], t1 = a.off[i + 1u] - 1u, na = t1 - t0;
        const uint32_t c0 = a.v_off[id], nb = a.v_off[id + 1u] - c0, nmin = na < nb ? na : nb;
        uint32_t pre = 0;
        while (pre < nmin) {
          const uint32_t x = a.blob[t0 + pre];
          if (x >= 128u || x != a.v_pool[c0 + pre]) break;
          ++pre;
        }
        uint32_t sfx = 0;
        while (sfx < nmin - pre) {
          const uint32_t x = a.blob[t1 - 1u - sfx];
          if (x >= 128u || x != a.v_pool[c0 + nb - 1u - sfx]) break;
          ++sfx;
        }
        {  // the shape of the script as k_conf_key sees it: middle lengths, prefix / suffix flags, then the length
          const uint32_t ma = na - pre - sfx, mb = nb - pre - sfx;
          key = ((ma < 6u ? ma : 6u) << 5) | ((mb < 6u ? mb : 6u) << 2) | (pre ? 2u : 0u) | (sfx ? 1u : 0u);
          key = key << 5 | (na < 31u ? na : 31u);
        }
        uint64_t im0 = 0, im1 = 0, cm0 = 0, cm1 = 0;
        bool imo = false, cmo = false;  // (prefix and suffix stop at the first non-ASCII character: those are all in the middles)
        for (uint32_t x = pre; x < na - sfx; ++x) {
          const uint32_t ch = a.blob[t0 + x];
          if (ch < 64u) im0 |= 1ull << ch; else if (ch < 128u) im1 |= 1ull << (ch - 64u); else imo = true;
        }
        for (uint32_t x = pre; x < nb - sfx; ++x) {
          const uint32_t ch = a.v_pool[c0 + x];
          if (ch < 64u) cm0 |= 1ull << ch; else if (ch < 128u) cm1 |= 1ull << (ch - 64u); else cmo = true;
        }
        need = false;
        for (uint32_t j = 0; j < a.P.nconf && !need; ++j) {
          const cdiff::FlatConf& cf = a.P.conf[j];
          bool may = true;
          for (uint32_t o_ = 0; o_ < cf.nops && may; ++o_) {
            const cdiff::FlatOp& o = a.P.ops[cf.op_begin + o_];
            if (!o.simple) {
              may = o.op == '-' ? pairs_opt_may(a.P, o, im0, im1, imo) : o.op == '+' ? pairs_opt_may(a.P, o, cm0, cm1, cmo)
                                : pairs_opt_may(a.P, o, ins.w[0] & cs.w[0], ins.w[1] & cs.w[1], in_other && cs.other);
              continue;
            }
            uint64_t h0 = o.bits[0], h1 = o.bits[1];
            if (o.op == '-') { h0 &= im0; h1 &= im1; }
            else if (o.op == '+') { h0 &= cm0; h1 &= cm1; }
            else { h0 &= ins.w[0] & cs.w[0]; h1 &= ins.w[1] & cs.w[1]; }
            if (!(h0 | h1)) may = false;
          }
          need = may;
        }
      }
    }
    a.mask[r] = 0ull;
  }
  // every lane is still here: one reservation per wave
  const unsigned long long bal = __ballot(need);
  if (!bal) return;  // (wave-uniform)
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t first = 0;
  if (lane == 0u) first = atomicAdd(&a.ctr[0], (uint32_t)__popcll(bal));
  first = (uint32_t)__shfl((int)first, 0);
  if (need) {
    const uint32_t pos = first + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (pos < a.R) {  // (cannot fail: every row is listed once at most)
      a.list[pos] = r;
      a.key[pos] = key;
    }
  }
}

// ---- the mask pass: four kernels per pass over the list ---------------------------------------------------------------------------------
// The edit script's body keeps more scalar state alive than the 102 SGPRs hold (k_conf_script spills 86 of them into VGPR lanes), so the
// row's work is cut where the body's own steps end -- prepare, diff, clean up, find -- and each step is a kernel of its own that keeps
// every scalar in registers.  Between the kernels the row's state lies in the lane memory (the two texts, the arena, the diffs) and in
// 32 bytes per lane slot; a lane slot therefore holds ONE row per pass, and the host enqueues ceil(R / slots) passes (the list's length
// is the device's: a slot behind the list does nothing).
struct CsSlot { uint32_t row, na, nb, nd, state, arena_used, live_lo, live_hi; };  // state: CS_RUN .. CS_HOST
constexpr uint32_t CS_IDLE = 0, CS_RUN = 1, CS_OVERFLOW = 2, CS_HOST = 3;  // no row / a script to compute / the context overflowed / the lane memory cannot hold the texts
struct CsScriptArgs {
  uint32_t n, R, first;            // first: the list position of lane slot 0 in this pass
  const uint4* info;
  const uint8_t* blob;
  const uint32_t* off;
  cdiff::Patterns P;
  const uint32_t* v_pool; const uint32_t* v_off; const cdiff::CharSet* v_cs; uint32_t nvocab;
  const uint32_t (*alpha)[2]; uint32_t nalpha;
  unsigned long long* mask;
  const uint32_t* sorted;
  uint32_t* hostrows;
  uint32_t* ctr;
  uint32_t* work;
  CsSlot* slot;                    // [blocks * 64]
};
__device__ __forceinline__ cdiff::Ctx cs_ctx(const CsScriptArgs& a) {
  cdiff::Ctx c;
  c.mem = a.work + (size_t)blockIdx.x * CF_WORDS * 64u + threadIdx.x * CF_G;
  c.arena_off = CF_ARENA_OFF; c.arena_cap = CF_ARENA; c.arena_used = 0;
  c.d_off = CF_D_OFF; c.d_cap = CF_DIFFS; c.nd = 0;
  c.v_off = CF_V_OFF; c.v_cap = CF_V;
  c.f_off = CF_F_OFF; c.frame_cap = CF_FRAMES;
  c.alpha = a.alpha; c.nalpha = a.nalpha;
  c.overflow = false;
  return c;
}
// One lane per listed row of the pass: both texts into the lane memory and the patterns that can match at all (mask_live).
__global__ __launch_bounds__(CF_THREADS) void k_cs_mask_prep(CsScriptArgs a) {
  const uint32_t s = blockIdx.x * CF_THREADS + threadIdx.x, k = a.first + s;
  CsSlot st{0xFFFFFFFFu, 0u, 0u, 0u, CS_IDLE, 0u, 0u, 0u};
  if (k >= a.first && k < min(a.ctr[0], a.R)) {
    const uint32_t r = a.sorted[k];
    if (r < a.R) {  // (the first ctr[0] sorted entries are the list)
      const uint4 inf = a.info[r];
      const uint32_t i = inf.x, id = inf.w;
      if (i < a.n && id < a.nvocab) {  // (k_cs_screen lists no other row)
        cdiff::Ctx c = cs_ctx(a);
        uint32_t na = 0;
        const uint32_t c0 = a.v_off[id], nb = a.v_off[id + 1u] - c0;
        st.row = r;
        if (pairs_conf_decode(c, a.blob, a.off[i], a.off[i + 1u] - 1u, CF_IN_OFF, &na) && nb <= CF_MAXCP) {
          for (uint32_t x = 0; x < nb; ++x) DC::W(c, CF_CAND_OFF + x) = a.v_pool[c0 + x];  // the candidate joins the lane memory
          const cdiff::View in = cdiff::mk(CF_IN_OFF, na), cand = cdiff::mk(CF_CAND_OFF, nb);
          const uint64_t live = DC::mask_live(c, a.P, in, DC::charset_of(c, in), cand, a.v_cs[id]);
          st.na = na; st.nb = nb; st.live_lo = (uint32_t)live; st.live_hi = (uint32_t)(live >> 32);
          st.state = live ? CS_RUN : CS_IDLE;  // (no pattern can match: the mask stays 0)
        } else st.state = CS_HOST;
      }
    }
  }
  a.slot[s] = st;
}
// diff_main of the slot's row (edit_script_begin)
__global__ __launch_bounds__(CF_THREADS) void k_cs_mask_diff(CsScriptArgs a) {
  const uint32_t s = blockIdx.x * CF_THREADS + threadIdx.x;
  CsSlot st = a.slot[s];
  if (st.state != CS_RUN) return;
  cdiff::Ctx c = cs_ctx(a);
  DC::edit_script_begin(c, cdiff::mk(CF_IN_OFF, st.na), cdiff::mk(CF_CAND_OFF, st.nb));
  st.nd = c.nd; st.arena_used = c.arena_used;
  if (c.overflow) st.state = CS_OVERFLOW;
  a.slot[s] = st;
}
// the clean-ups and the compaction (edit_script_finish).  The alphabetic table's address and length are moved into vector registers:
// the body reads them in its innermost scoring loop, and as scalars they are the two values too many for this step.
__global__ __launch_bounds__(CF_THREADS) void k_cs_mask_clean(CsScriptArgs a) {
  const uint32_t s = blockIdx.x * CF_THREADS + threadIdx.x;
  CsSlot st = a.slot[s];
  if (st.state != CS_RUN) return;
  cdiff::Ctx c = cs_ctx(a);
  {
    uint32_t lo = (uint32_t)(uintptr_t)a.alpha, hi = (uint32_t)((uintptr_t)a.alpha >> 32), q = a.nalpha;
    asm volatile("" : "+v"(lo), "+v"(hi), "+v"(q));
    c.alpha = (const uint32_t(*)[2])((uintptr_t)hi << 32 | lo); c.nalpha = q;
  }
  c.nd = st.nd; c.arena_used = st.arena_used;
  if (!DC::edit_script_finish(c)) st.state = CS_OVERFLOW;
  st.nd = c.nd;
  a.slot[s] = st;
}
// found_in per pattern that can match (mask_found) -> the row's mask; a row the lane memory could not hold is listed for the host
__global__ __launch_bounds__(CF_THREADS) void k_cs_mask_find(CsScriptArgs a) {
  const uint32_t s = blockIdx.x * CF_THREADS + threadIdx.x;
  const CsSlot st = a.slot[s];
  if (st.state == CS_IDLE || st.row >= a.R) return;
  if (st.state == CS_RUN) {
    cdiff::Ctx c = cs_ctx(a);
    c.nd = st.nd;
    a.mask[st.row] = DC::mask_found(c, a.P, (uint64_t)st.live_hi << 32 | st.live_lo);
  } else {
    const uint32_t pos = atomicAdd(&a.ctr[1], 1u);
    if (pos < a.R) a.hostrows[pos] = st.row;
  }
}

// ---- once per set ---------------------------------------------------------------------------------------------------------------------
struct CsSetArgs {
  uint32_t n, R;
  const uint4* info;
  const double* score;             // [R] unweighted
  const unsigned long long* mask;  // [R]
  const double* weights;           // the set's [np]
  uint32_t np;
  int early;
  double score_threshold;
  uint32_t* cnt;                   // [n] kept rows per pair
  const uint32_t* soff;            // [n + 1] exclusive scan of cnt
  uint32_t* cur;                   // [n] starts as soff[0 .. n)
  uint4* c_rows;                   // [row_cap] SurvRow as two 16-byte words
  uint32_t row_cap;
  // late: the ranked slots
  const uint32_t *rbeg, *rend, *r_count;
  const DevRow* r_rows;
  double* slot_w;                  // [row_cap]
};
// the set's weights into LDS (every thread of the block calls this), then w(mask) = ((1.0 * w_a) * w_b) * ...: ascending pattern order
__device__ __forceinline__ void cs_weights_load(const CsSetArgs& k, double* s_w) {
  if (threadIdx.x < CS_MAXP) s_w[threadIdx.x] = threadIdx.x < k.np ? k.weights[threadIdx.x] : 1.0;
  __syncthreads();
}
__device__ __forceinline__ double cs_weight(const double* s_w, unsigned long long mask) {
  double w = 1.0;
  for (unsigned long long m = mask; m; m &= m - 1ull) w *= s_w[__ffsll((long long)m) - 1];
  return w;
}
__global__ __launch_bounds__(GOLD_BLOCK) void k_cs_count(CsSetArgs k) {
  const uint32_t r = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  uint32_t pair = GOLD_NONE;
  bool keep = false;
  if (r < k.R) {
    pair = k.info[r].x;
    if (pair < k.n) keep = k.score[r] >= k.score_threshold;  // src/lib.rs:1475, on the unweighted score
    else pair = GOLD_NONE;
  }
  const RwRun run = rw_run(pair);
  const uint32_t c = (uint32_t)__popcll(__ballot(keep) & run.lanes);
  if ((threadIdx.x & 63u) == run.end && pair != GOLD_NONE && c) atomicAdd(&k.cnt[pair], c);
}
__global__ __launch_bounds__(GOLD_BLOCK) void k_cs_fill(CsSetArgs k) {
  __shared__ double s_w[CS_MAXP];
  cs_weights_load(k, s_w);
  const uint32_t r = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint4 inf = make_uint4(GOLD_NONE, 0u, 0u, 0u);
  double s = 0.0;
  bool keep = false;
  if (r < k.R) {
    inf = k.info[r];
    if (inf.x < k.n) {
      s = k.score[r];
      keep = s >= k.score_threshold;  // (the test k_cs_count counted with, on the same stored value)
    } else inf.x = GOLD_NONE;
  }
  const RwRun run = rw_run(inf.x);
  const unsigned long long km = __ballot(keep) & run.lanes;
  uint32_t base = 0;
  if (lane == run.start && km) base = atomicAdd(&k.cur[inf.x], (uint32_t)__popcll(km));
  base = (uint32_t)__shfl((int)base, (int)run.start);
  if (!keep) return;
  const uint32_t pos = base + (uint32_t)__popcll(km & ((1ull << lane) - 1ull));
  if (pos >= k.soff[inf.x + 1u] || pos >= k.row_cap) return;  // (cannot happen: the offsets are the scan of these very counts)
  if (k.early) s = s * cs_weight(s_w, k.mask[r]);  // src/lib.rs:1505-1508 (x * 1.0 == x)
  const unsigned long long sb = (unsigned long long)__double_as_longlong(s), ord = (unsigned long long)inf.y << 20;
  k.c_rows[2 * (size_t)pos] = make_uint4((uint32_t)sb, (uint32_t)(sb >> 32), (uint32_t)ord, (uint32_t)(ord >> 32));
  k.c_rows[2 * (size_t)pos + 1] = make_uint4(inf.w, inf.z, GOLD_NONE, 0u);  // {vocab, freq, no via, pad}
}
// late: one lane per slot of the ranked segments: slot x belongs to the pair whose segment holds it (a binary search over the offsets);
// a ranked row's base row is the one of its pair with the same vocabulary id (an instance per item and input)
__global__ __launch_bounds__(GOLD_BLOCK) void k_cs_slot_w(CsSetArgs k) {
  __shared__ double s_w[CS_MAXP];
  cs_weights_load(k, s_w);
  const uint32_t x = blockIdx.x * GOLD_BLOCK + threadIdx.x;
  const uint32_t total = min(k.soff[k.n], k.row_cap);
  if (x >= total) return;
  uint32_t lo = 0, hi = k.n;  // the last pair with soff[pair] <= x
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (k.soff[mid] <= x) lo = mid; else hi = mid;
  }
  double w = 1.0;
  if (x - k.soff[lo] < k.r_count[lo]) {
    const uint32_t vocab = k.r_rows[x].vocab_id, e = min(k.rend[lo], k.R);
    for (uint32_t r = k.rbeg[lo]; r < e; ++r) {
      const uint4 inf = k.info[r];
      if (inf.x == lo && inf.w == vocab) { w = cs_weight(s_w, k.mask[r]); break; }
    }
  }
  k.slot_w[x] = w;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
struct CsCall {
  const HostModel* m = nullptr;
  const DeviceLexicon* dl = nullptr;
  HostModel::ConfTables tables;    // the host body's patterns (the fallback and ANX_CONFUSABLES=host)
  PoolBlocks blocks;
  cdiff::Patterns P{};             // on the device
  double* d_weights = nullptr;     // [n_sets][np]
  uint32_t np = 0;
  size_t n_sets = 0;
  ConfVocabView voc{};
};

void csweep_call_end(CsCall* c) {
  if (!c) return;
  (void)hipSetDevice(c->dl->device);
  (void)hipDeviceSynchronize();
  c->blocks.release();
  delete c;
}

int csweep_call_begin(const HostModel& m, const DeviceLexicon* dl, const HostModel::ConfTables& t, const double* weights, size_t n_sets, CsCall** out, std::string& err) {
  *out = nullptr;
  if (!dl) { err = "model is not resident on a device"; return ANX_ENODEVICE; }
  if (t.conf.empty() || t.conf.size() > CS_MAXP) { err = "confusable sweep: 1 .. 64 patterns"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(dl->device));
  CsCall* c = new CsCall;
  struct Guard { CsCall* c; ~Guard() { if (c) csweep_call_end(c); } } guard{c};
  c->m = &m; c->dl = dl; c->tables = t; c->np = (uint32_t)t.conf.size(); c->n_sets = n_sets;
  if (int rc = conf_vocab_view(m, dl, &c->voc, err)) return rc;
  cdiff::FlatConf* d_conf = nullptr; cdiff::FlatOp* d_ops = nullptr; cdiff::FlatOpt* d_opts = nullptr; uint32_t* d_pool = nullptr;
  int rc;
  if ((rc = c->blocks.get(&d_conf, t.conf.size(), err)) || (rc = c->blocks.get(&d_ops, std::max<size_t>(t.ops.size(), 1), err)) ||
      (rc = c->blocks.get(&d_opts, std::max<size_t>(t.opts.size(), 1), err)) || (rc = c->blocks.get(&d_pool, std::max<size_t>(t.pool.size(), 1), err)) ||
      (rc = c->blocks.get(&c->d_weights, n_sets * c->np, err)))
    return rc;
  HIP_TRY(hipMemcpy(d_conf, t.conf.data(), t.conf.size() * sizeof(cdiff::FlatConf), hipMemcpyHostToDevice));
  if (!t.ops.empty()) HIP_TRY(hipMemcpy(d_ops, t.ops.data(), t.ops.size() * sizeof(cdiff::FlatOp), hipMemcpyHostToDevice));
  if (!t.opts.empty()) HIP_TRY(hipMemcpy(d_opts, t.opts.data(), t.opts.size() * sizeof(cdiff::FlatOpt), hipMemcpyHostToDevice));
  if (!t.pool.empty()) HIP_TRY(hipMemcpy(d_pool, t.pool.data(), t.pool.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->d_weights, weights, n_sets * c->np * sizeof(double), hipMemcpyHostToDevice));
  c->P.conf = d_conf; c->P.nconf = c->np; c->P.ops = d_ops; c->P.opts = d_opts; c->P.pool = d_pool;
  guard.c = nullptr;
  *out = c;
  return ANX_OK;
}

struct CsGroup {
  CsCall* call = nullptr;
  RwGroup* g = nullptr;            // the base rows; its pool blocks hold this group's buffers too
  unsigned long long* mask = nullptr;
  uint32_t *rbeg = nullptr, *rend = nullptr;
  double* slot_w = nullptr;
};

void csweep_group_end(CsGroup* g) {
  if (!g) return;
  reweigh_group_end(g->g);
  delete g;
}

namespace {
// mask[k] of the rows rows[k] = {pair, ., ., vocabulary id} with the host body, on up to 16 threads when there are many
void masks_on_host(const CsCall& c, const PairSpan* inputs, size_t n, const uint4* rows, size_t count, uint64_t* mask) {
  const HostModel& m = *c.m;
  auto work = [&](size_t lo, size_t hi) {
    for (size_t k = lo; k < hi; ++k) {
      const uint32_t i = rows[k].x, id = rows[k].w;
      mask[k] = 0;
      if (i >= n || id >= m.decoder.size()) continue;
      const std::string& t = m.decoder[id].text;
      mask[k] = confusable_mask_text(c.tables, inputs[i].p, inputs[i].len, t.data(), t.size());
    }
  };
  const size_t nt = count < 4096 ? 1 : std::min<size_t>(16, std::max(1u, usable_hw_threads()));
  if (nt <= 1) { work(0, count); return; }
  std::vector<std::thread> th;
  const size_t per = (count + nt - 1) / nt;
  for (size_t t = 0; t < nt; ++t) th.emplace_back(work, std::min(count, t * per), std::min(count, (t + 1) * per));
  for (std::thread& t : th) t.join();
}
}  // namespace

int csweep_group_begin(CsCall* c, const SweepChunkView& v, const anx_params& group, const std::vector<LearnSection>& secs, const std::vector<size_t>& sec_rows,
                       const std::vector<const anx_row_measures*>& sec_meas, bool want_records, const PairSpan* inputs, CsGroup** out, std::string& err) {
  *out = nullptr;
  RwGroup* g = nullptr;
  if (int rc = reweigh_group_begin(v, group, secs, sec_rows, sec_meas, want_records, &g, err)) return rc;
  CsGroup* cg = new CsGroup;
  cg->call = c; cg->g = g;
  struct Guard { CsGroup* g; ~Guard() { if (g) csweep_group_end(g); } } guard{cg};
  const size_t n = g->n, R = g->R, Rc = std::max<size_t>(R, 1);
  const DeviceLexicon* dl = v.dl;
  hipStream_t st = reinterpret_cast<hipStream_t>(v.stream);
  const bool host_mode = switches().confusables_host != 0;
  cdiff::CharSet* in_cs = nullptr;
  uint32_t *list = nullptr, *key = nullptr, *hostrows = nullptr, *ctr = nullptr;
  int rc;
  if ((rc = g->get(&cg->mask, Rc, err)) || (rc = g->get(&cg->rbeg, n, err)) || (rc = g->get(&cg->rend, n, err)) || (rc = g->get(&cg->slot_w, Rc, err))) return rc;
  HIP_TRY(hipMemsetAsync(cg->rbeg, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(cg->rend, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(cg->mask, 0, Rc * sizeof(unsigned long long), st));
  const anx_weights& w = v.m->weights;
  CsScoreArgs ks{};
  ks.n = (uint32_t)n; ks.R = (uint32_t)R; ks.info = g->info; ks.meas = g->meas;
  ks.w = RwWeights{w.ld, w.lcs, w.prefix, w.suffix, w.casew, w.ld + w.lcs + w.prefix + w.suffix + w.casew, dl->quot};  // w_sum: src/types.rs:69-73, as launch_plan.hpp
  ks.score = g->score; ks.rbeg = cg->rbeg; ks.rend = cg->rend;
  if (R) {
    const int kt = ktimer_begin("k_cs_score", st);
    hipLaunchKernelGGL(k_cs_score, dim3(gold_grid(R)), dim3(GOLD_BLOCK), 0, st, ks);
    ktimer_end(kt, st);
    hipLaunchKernelGGL(k_cs_ranges, dim3(gold_grid(R)), dim3(GOLD_BLOCK), 0, st, ks);
  }
  csweep_stats_add(CS_BASE_ROWS, R);
  uint32_t h_ctr[4] = {0, 0, 0, 0};
  uint32_t cf_blocks = 0;
  void* work = nullptr;
  if (!host_mode && R) {
    // one wave per 64 rows, at most CF_BLOCKS of them in flight (the mask pass takes that many rows at a time): the working set follows the group's rows
    cf_blocks = std::min<uint32_t>(CF_BLOCKS, (uint32_t)((R + 63) / 64));
    if (pool_malloc(&work, (size_t)cf_blocks * CF_WORDS * 64u * sizeof(uint32_t)) != hipSuccess) {
      (void)hipGetLastError();
      work = nullptr;  // no room for the working set: the host body computes the masks (same results)
    } else g->blocks.v.push_back(work);
  }
  const bool on_device = work != nullptr;
  if (on_device) {
    const size_t tmp_bytes = conf_pairs_sort_tmp_bytes((uint32_t)R);
    uint8_t* tmp = nullptr;
    CsSlot* slots = nullptr;
    if ((rc = g->get(&in_cs, n, err)) || (rc = g->get(&list, Rc, err)) || (rc = g->get(&key, 3 * Rc, err)) || (rc = g->get(&hostrows, Rc, err)) ||
        (rc = g->get(&ctr, 4, err)) || (rc = g->get(&tmp, std::max<size_t>(tmp_bytes, 16), err)) || (rc = g->get(&slots, (size_t)cf_blocks * CF_THREADS, err)))
      return rc;
    HIP_TRY(hipMemsetAsync(ctr, 0, 4 * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(key, 0xFF, R * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(list, 0xFF, R * sizeof(uint32_t), st));  // (behind the list: no row)
    CsMaskArgs a{};
    a.n = (uint32_t)n; a.R = (uint32_t)R; a.info = g->info; a.blob = v.blob; a.off = v.off; a.in_cs = in_cs; a.P = c->P;
    a.v_pool = c->voc.v_pool; a.v_off = c->voc.v_off; a.v_cs = c->voc.v_cs; a.nvocab = c->voc.nvocab; a.alpha = c->voc.alpha; a.nalpha = c->voc.nalpha;
    a.mask = cg->mask; a.list = list; a.key = key; a.sorted = key + 2 * R; a.hostrows = hostrows; a.ctr = ctr; a.work = static_cast<uint32_t*>(work);
    hipLaunchKernelGGL(k_cs_inbits, dim3(gold_grid(n)), dim3(GOLD_BLOCK), 0, st, a);
    {
      const int kt = ktimer_begin("k_cs_screen", st);
      hipLaunchKernelGGL(k_cs_screen, dim3(gold_grid(R)), dim3(GOLD_BLOCK), 0, st, a);
      ktimer_end(kt, st);
    }
    {
      const int kt = ktimer_begin("k_cs_order", st);
      if ((rc = conf_sort_enqueue(tmp, tmp_bytes, key, key + R, list, key + 2 * R, (uint32_t)R, st, err))) return rc;
      ktimer_end(kt, st);
    }
    {
      const int kt = ktimer_begin("k_cs_mask", st);
      CsScriptArgs sa{};
      sa.n = a.n; sa.R = a.R; sa.info = a.info; sa.blob = a.blob; sa.off = a.off; sa.P = a.P; sa.v_pool = a.v_pool; sa.v_off = a.v_off; sa.v_cs = a.v_cs; sa.nvocab = a.nvocab;
      sa.alpha = a.alpha; sa.nalpha = a.nalpha; sa.mask = a.mask; sa.sorted = a.sorted; sa.hostrows = a.hostrows; sa.ctr = a.ctr; sa.work = a.work; sa.slot = slots;
      const size_t lanes = (size_t)cf_blocks * CF_THREADS;
      for (size_t first = 0; first < R; first += lanes) {  // (the list is at most R long; a pass behind its end finds every slot idle)
        sa.first = (uint32_t)first;
        hipLaunchKernelGGL(k_cs_mask_prep, dim3(cf_blocks), dim3(CF_THREADS), 0, st, sa);
        hipLaunchKernelGGL(k_cs_mask_diff, dim3(cf_blocks), dim3(CF_THREADS), 0, st, sa);
        hipLaunchKernelGGL(k_cs_mask_clean, dim3(cf_blocks), dim3(CF_THREADS), 0, st, sa);
        hipLaunchKernelGGL(k_cs_mask_find, dim3(cf_blocks), dim3(CF_THREADS), 0, st, sa);
      }
      ktimer_end(kt, st);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_ctr, ctr, sizeof h_ctr, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));  // the group's wait
  if (on_device) {
    if (h_ctr[0] > R || h_ctr[1] > R) { err = "confusable sweep: the mask pass listed more rows than there are"; return ANX_EINVAL; }
    csweep_stats_add(CS_ROWS_LISTED, h_ctr[0]);
  }
  if (on_device && h_ctr[1]) {  // the rows the lane memory could not hold: their masks alone, with the host body
    const size_t cnt = h_ctr[1];
    std::vector<uint32_t> rows(cnt);
    HIP_TRY(hipMemcpy(rows.data(), hostrows, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<uint4> inf(cnt);
    std::vector<uint64_t> hm(cnt);
    const bool few = cnt <= 1024;
    std::vector<uint4> all;
    if (few) {
      for (size_t k = 0; k < cnt; ++k) {
        if (rows[k] >= R) { err = "confusable sweep: a row beyond the group's rows was left to the host"; return ANX_EINVAL; }
        HIP_TRY(hipMemcpy(&inf[k], g->info + rows[k], sizeof(uint4), hipMemcpyDeviceToHost));
      }
    } else {
      all.resize(R);
      HIP_TRY(hipMemcpy(all.data(), g->info, R * sizeof(uint4), hipMemcpyDeviceToHost));
      for (size_t k = 0; k < cnt; ++k) {
        if (rows[k] >= R) { err = "confusable sweep: a row beyond the group's rows was left to the host"; return ANX_EINVAL; }
        inf[k] = all[rows[k]];
      }
    }
    masks_on_host(*c, inputs, n, inf.data(), cnt, hm.data());
    for (size_t k = 0; k < cnt; ++k) HIP_TRY(hipMemcpy(cg->mask + rows[k], &hm[k], sizeof(uint64_t), hipMemcpyHostToDevice));
    csweep_stats_add(CS_ROWS_PATCHED, cnt);
  } else if (!on_device && R) {  // ANX_CONFUSABLES=host (or no room for the working set): every mask with the host body
    std::vector<uint4> inf(R);
    std::vector<uint64_t> hm(R);
    HIP_TRY(hipMemcpy(inf.data(), g->info, R * sizeof(uint4), hipMemcpyDeviceToHost));
    masks_on_host(*c, inputs, n, inf.data(), R, hm.data());
    HIP_TRY(hipMemcpy(cg->mask, hm.data(), R * sizeof(uint64_t), hipMemcpyHostToDevice));
    csweep_stats_add(CS_ROWS_HOST_MODE, R);
  }
  guard.g = nullptr;
  *out = cg;
  return ANX_OK;
}

namespace {
// The front of a set: the rows with an unweighted score >= p.score_threshold as SurvRow (early: score times the weight of the row's mask
// under set `set`), then k_rank -- late without a cutoff, as the batch path ranks before k_conf_apply_late.  k: the set's kernel arguments.
int cs_rank_enqueue(CsGroup* cg, const anx_params& p, size_t set, bool early, CsSetArgs& k, std::string& err) {
  RwGroup* g = cg->g;
  const CsCall* c = cg->call;
  const SweepChunkView& v = g->v;
  const size_t n = g->n, R = g->R;
  HIP_TRY(hipSetDevice(v.dl->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(v.stream);
  HIP_TRY(hipMemsetAsync(g->cnt, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(g->r_count, 0, n * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(g->d_sum, 0, sizeof(anx_gold_summary), st));
  k.n = (uint32_t)n; k.R = (uint32_t)R; k.info = g->info; k.score = g->score; k.mask = cg->mask;
  k.weights = c->d_weights + set * c->np; k.np = c->np; k.early = early ? 1 : 0; k.score_threshold = p.score_threshold;
  k.cnt = g->cnt; k.soff = g->soff; k.cur = g->cur; k.c_rows = reinterpret_cast<uint4*>(g->c_rows); k.row_cap = (uint32_t)R;
  k.rbeg = cg->rbeg; k.rend = cg->rend; k.r_count = g->r_count; k.r_rows = g->r_rows; k.slot_w = cg->slot_w;
  if (R) hipLaunchKernelGGL(k_cs_count, dim3(gold_grid(R)), dim3(GOLD_BLOCK), 0, st, k);
  if (prefix_scan_enqueue(g->cnt, (uint32_t)n, g->soff, g->tmp, st, g->cur)) { err = "confusable sweep: the prefix sum could not be enqueued"; return ANX_ENODEVICE; }
  if (R) {
    const int kt = ktimer_begin("k_cs_fill", st);
    hipLaunchKernelGGL(k_cs_fill, dim3(gold_grid(R)), dim3(GOLD_BLOCK), 0, st, k);
    ktimer_end(kt, st);
  }
  {
    // late: the crop, no cutoff yet -- as the batch path ranks before k_conf_apply_late (launch_plan.hpp rank_args_of)
    const int kt = ktimer_begin("k_rank (confusable sweep)", st);
    rank_rows_enqueue(RankPlain{early ? p.cutoff_threshold : 0.0, p.max_matches, p.freq_weight, v.m->have_freq ? 1 : 0}, st, (uint32_t)n, g->soff, g->c_rows, g->maxf,
                      g->t_key, g->r_rows, g->r_count, (uint32_t)R, g->ovf);
    ktimer_end(kt, st);
  }
  return ANX_OK;
}
}  // namespace

int csweep_group_rank_late(CsGroup* cg, const anx_params& p, CsRankedView* out, std::string& err) {
  RwGroup* g = cg->g;
  CsSetArgs k{};
  if (int rc = cs_rank_enqueue(cg, p, 0, false, k, err)) return rc;
  HIP_TRY(hipGetLastError());
  out->dl = g->v.dl; out->stream = g->v.stream; out->n = g->n; out->R = g->R;
  out->info = g->info; out->mask = cg->mask; out->rbeg = cg->rbeg; out->rend = cg->rend; out->soff = g->soff; out->r_count = g->r_count;
  out->gid = g->v.gid; out->r_rows = g->r_rows; out->scan_tmp = g->tmp;
  return ANX_OK;
}

int csweep_group_set(CsGroup* cg, const anx_params& p, size_t set, bool early, bool baseline, anx_gold_summary* sum, anx_gold_eval* out, std::string& err) {
  RwGroup* g = cg->g;
  const CsCall* c = cg->call;
  if (out && !g->d_out) { err = "csweep_group_set: the group keeps no record buffer"; return ANX_EINVAL; }
  if (set >= c->n_sets) { err = "csweep_group_set: no such set"; return ANX_EINVAL; }
  const SweepChunkView& v = g->v;
  const size_t n = g->n, R = g->R;
  hipStream_t st = reinterpret_cast<hipStream_t>(v.stream);
  CsSetArgs k{};
  if (int rc = cs_rank_enqueue(cg, p, set, early, k, err)) return rc;
  if (!early) {
    if (R) {
      const int kt = ktimer_begin("k_cs_slot_w", st);
      hipLaunchKernelGGL(k_cs_slot_w, dim3(gold_grid(R)), dim3(GOLD_BLOCK), 0, st, k);
      ktimer_end(kt, st);
    }
    const int kt = ktimer_begin("k_conf_apply_late (confusable sweep)", st);
    conf_apply_late_enqueue(st, (uint32_t)n, (uint32_t)R, g->soff, g->r_rows, cg->slot_w, g->ovf, p.cutoff_threshold, p.freq_weight, g->r_count);
    ktimer_end(kt, st);
  }
  HIP_TRY(hipGetLastError());
  size_t bytes = 0;
  if (int rc = reweigh_group_finish(g, p, v.m->weights, baseline, sum, out, &bytes, err)) return rc;
  csweep_stats_add(CS_BYTES_DOWN, bytes);
  return ANX_OK;
}

int csweep_group_masks(CsGroup* cg, std::vector<uint32_t>& pair, std::vector<uint32_t>& vocab, std::vector<uint64_t>& mask, std::string& err) {
  RwGroup* g = cg->g;
  const size_t R = g->R;
  HIP_TRY(hipSetDevice(g->v.dl->device));
  HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(g->v.stream)));
  std::vector<uint4> inf(R);
  std::vector<uint64_t> hm(R);
  if (R) {
    HIP_TRY(hipMemcpy(inf.data(), g->info, R * sizeof(uint4), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hm.data(), cg->mask, R * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  pair.clear(); vocab.clear(); mask.clear();
  for (size_t r = 0; r < R; ++r)
    if (inf[r].x < g->n) { pair.push_back(inf[r].x); vocab.push_back(inf[r].w); mask.push_back(hm[r]); }
  return ANX_OK;
}

}  // namespace anx
