// mine.hip -- anx_mine_confusables ON THE DEVICE (gfx950 / CDNA4): from a chunk of (observed, correct) string pairs to the change sites of
// their edit scripts and the histogram of distinct sites.  The script is confusables_core.hpp's edit_script, the source the host and
// conf.hip compile too; what conf.hip does with a script is match patterns against it, here the script itself is the result.
//   k_mine_script : a lane per pair on a fixed grid that strides over the pairs, wave-interleaved lane memories (conf_lane.hpp): decode
//                   both sides, edit_script, walk the diffs.  A site is a maximal run of non-`=` diffs; per site one record and one
//                   64-bit key -- a hash of (anchor flags if asked, left context, separator, deleted, separator, inserted, separator,
//                   right context) over code points.  Positions in the record / key arrays are reserved with ONE atomic per wave and
//                   round (the lanes' site counts are scanned over the wave first), as k_pairs_conf_screen reserves its list.
//                   Byte-equal sides emit nothing.  A side above CF_MAXCP code points or a lane-memory overflow -- k_pairs_conf_script's
//                   rule -- and a site that is not -[..], +[..] or -[..]+[..] put the pair on the host list.
//   histogram     : learn.hip's scheme (k_lf_head / k_lf_rep): stable radix sort of (key, site); k_mine_head + max-scan = run starts;
//                   k_mine_rep: a site's representative is the first site of its hash run with the same code points, so a hash
//                   collision never merges two texts; a second sort by representative makes every text's sites contiguous whatever the
//                   runs held; sums of `sites` and `count` per representative by reduce_by_key (integers; no float atomics);
//                   k_mine_pattern writes the pattern index back into every site record; k_mine_rows gathers the distinct table.
//   site list     : per-pair site counts -> exclusive scan = offsets; k_mine_emit scatters the records to offsets[pair] + position in the
//                   pair with their FINAL pattern indices (the host's merged, ordered table) -- mine_chunk_emit, once the table is known.
// The host (mine_capi.cpp) builds the texts from the representatives' pairs, scripts the handed-back pairs and merges the chunks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>

#include "engine_internal.h"
#include "conf_lane.hpp"
#include "mine.h"

namespace anx {

#include "kernels_common.hpp"  // (DeviceLexicon)

namespace {
constexpr int MN_BLOCK = 256;
constexpr uint32_t MN_MAX_SITES = (CF_DIFFS + 1) / 2;  // of a pair: sites alternate with identities
constexpr uint32_t MN_SEP = 0xFFFFFFFFu;               // between the parts of a key (no code point)

struct MineRec {      // one site, 24 bytes
  uint32_t pair;      // chunk-relative
  uint32_t pos;       // a_pos | a_len << 8 | b_pos << 16 | b_len << 24 (code points, each <= 64)
  uint32_t abyte;     // where the left context (or, without one, the deleted text) starts in the blob
  uint32_t bbyte;     // where the inserted text starts in the blob
  uint32_t meta;      // left context | right context << 4 (code points) | first << 8 | last << 9 | position in the pair << 16
  uint32_t pattern;   // index in the chunk's table
};
struct MineSum { unsigned long long count, sites; };
struct MineSumPlus {
  __host__ __device__ MineSum operator()(const MineSum& x, const MineSum& y) const { return MineSum{x.count + y.count, x.sites + y.sites}; }
};

struct MineArgs {
  uint32_t n, cap, context, anchors;
  const uint8_t* blob;
  const uint32_t* off;            // [2 n + 1]: a of pair p = string p, b = string n + p; string s = blob[off[s] .. off[s + 1] - 1)
  const uint32_t (*alpha)[2]; uint32_t nalpha;
  uint32_t* work;                 // [blocks][CF_WORDS][64]
  MineRec* rec;                   // [cap]
  unsigned long long* key;        // [cap]
  uint32_t* val;                  // [cap] = the site's own index
  uint32_t* cnt;                  // [n + 1] sites per pair ([n] = 0)
  uint32_t* hostlist;             // [n]
  uint32_t* ctr;                  // [0] sites, [1] host pairs, [2] of them for a site's shape, [3] hash runs with more than one text
  unsigned long long hmask;
};

// byte length of the character at p of a string that ends at t1: pairs_conf_decode's rule (the lead byte alone; 1 when the string is too short)
__device__ inline uint32_t mine_len_at(const uint8_t* __restrict__ blob, uint32_t p, uint32_t t1) {
  const uint32_t b0 = blob[p];
  const uint32_t len = b0 < 0x80u ? 1u : (b0 >> 5) == 0x6u ? 2u : (b0 >> 4) == 0xEu ? 3u : (b0 >> 3) == 0x1Eu ? 4u : 1u;
  return len > t1 - p ? 1u : len;
}
__device__ inline uint32_t mine_cp_at(const uint8_t* __restrict__ blob, uint32_t p, uint32_t t1, uint32_t* len_out) {
  const uint32_t b0 = blob[p], len = mine_len_at(blob, p, t1);
  uint32_t cp = b0;
  if (len == 2u) cp = ((b0 & 0x1Fu) << 6) | (blob[p + 1] & 0x3Fu);
  else if (len == 3u) cp = ((b0 & 0x0Fu) << 12) | ((blob[p + 1] & 0x3Fu) << 6) | (blob[p + 2] & 0x3Fu);
  else if (len == 4u) cp = ((b0 & 0x07u) << 18) | ((blob[p + 1] & 0x3Fu) << 12) | ((blob[p + 2] & 0x3Fu) << 6) | (blob[p + 3] & 0x3Fu);
  *len_out = len;
  return cp;
}
// the byte position of character `ncp` of the string [t0, t1)
__device__ inline uint32_t mine_skip(const uint8_t* __restrict__ blob, uint32_t t0, uint32_t t1, uint32_t ncp) {
  uint32_t p = t0;
  for (uint32_t k = 0; k < ncp && p < t1; ++k) p += mine_len_at(blob, p, t1);
  return p;
}
__device__ inline void mine_mix(unsigned long long& h, uint32_t v) { h ^= v; h *= 1099511628211ull; }

__global__ __launch_bounds__(CF_THREADS) void k_mine_script(MineArgs a) {
  static_assert(CF_THREADS == 64, "one wave per block: the lane memories of a wave interleave");
  cdiff::Ctx c;
  c.mem = a.work + (size_t)blockIdx.x * CF_WORDS * 64u + threadIdx.x * CF_G;
  c.arena_off = CF_ARENA_OFF; c.arena_cap = CF_ARENA; c.arena_used = 0;
  c.d_off = CF_D_OFF; c.d_cap = CF_DIFFS; c.nd = 0;
  c.v_off = CF_V_OFF; c.v_cap = CF_V;
  c.f_off = CF_F_OFF; c.frame_cap = CF_FRAMES;
  c.alpha = a.alpha; c.nalpha = a.nalpha;
  c.overflow = false;
  const uint32_t lane = threadIdx.x;
  // (the loop is wave-uniform: every lane stays for the reservation of its round)
  for (uint32_t base = blockIdx.x * CF_THREADS; base < a.n; base += gridDim.x * CF_THREADS) {
    const uint32_t p = base + lane;
    const bool live = p < a.n;
    uint32_t nsite = 0, a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    bool tohost = false, odd = false;
    if (live) {
      a0 = a.off[p]; a1 = a.off[p + 1u] - 1u; b0 = a.off[a.n + p]; b1 = a.off[a.n + p + 1u] - 1u;
      bool equal = a1 - a0 == b1 - b0;
      for (uint32_t x = 0; equal && x < a1 - a0; ++x) equal = a.blob[a0 + x] == a.blob[b0 + x];
      if (!equal) {
        uint32_t na = 0, nb = 0;
        bool ok = pairs_conf_decode(c, a.blob, a0, a1, CF_IN_OFF, &na) && pairs_conf_decode(c, a.blob, b0, b1, CF_CAND_OFF, &nb);
        if (ok) ok = DC::edit_script(c, cdiff::mk(CF_IN_OFF, na), cdiff::mk(CF_CAND_OFF, nb));
        if (!ok) tohost = true;
        else {
          for (uint32_t i = 0; i < c.nd;) {
            if (DC::d_op(c, i) == '=') { ++i; continue; }
            uint32_t j = i;
            while (j < c.nd && DC::d_op(c, j) != '=') ++j;
            if (!(j - i == 1u || (j - i == 2u && DC::d_op(c, i) == '-' && DC::d_op(c, i + 1u) == '+'))) odd = true;
            ++nsite;
            i = j;
          }
          if (odd || nsite > MN_MAX_SITES) { tohost = true; nsite = 0; }
        }
      }
    }
    uint32_t incl = nsite;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
      if ((int)lane >= o) incl += up;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63);
    uint32_t first = 0;
    if (total) {  // (wave-uniform)
      if (lane == 0u) first = atomicAdd(&a.ctr[0], total);
      first = (uint32_t)__shfl((int)first, 0);
    }
    const bool fits = total && first <= a.cap && total <= a.cap - first;  // (else the host sees ctr[0] > cap and repeats the chunk with room for every site)
    if (live) {
      a.cnt[p] = fits ? nsite : 0u;
      if (tohost) {
        a.hostlist[atomicAdd(&a.ctr[1], 1u)] = p;  // (rare; at most once per pair: the list holds n)
        if (odd) atomicAdd(&a.ctr[2], 1u);
      }
    }
    uint32_t slot = first + incl - nsite, seq = 0, apos = 0, bpos = 0;
    for (uint32_t i = 0; fits && nsite && i < c.nd;) {
      if (DC::d_op(c, i) == '=') { const uint32_t l = DC::d_len(c, i); apos += l; bpos += l; ++i; continue; }
      uint32_t j = i, dl = 0, il = 0;
      for (; j < c.nd && DC::d_op(c, j) != '='; ++j) {
        if (DC::d_op(c, j) == '-') dl += DC::d_len(c, j);
        else il += DC::d_len(c, j);
      }
      const uint32_t lc = i > 0u ? min(a.context, DC::d_len(c, i - 1u)) : 0u, rc = j < c.nd ? min(a.context, DC::d_len(c, j)) : 0u;
      const uint32_t fl = (i == 0u ? 1u : 0u) | (j == c.nd ? 2u : 0u);
      unsigned long long h = 1469598103934665603ull;
      if (a.anchors) mine_mix(h, 0x100u | fl);
      for (uint32_t x = apos - lc; x < apos; ++x) mine_mix(h, DC::W(c, CF_IN_OFF + x));
      mine_mix(h, MN_SEP);
      for (uint32_t x = apos; x < apos + dl; ++x) mine_mix(h, DC::W(c, CF_IN_OFF + x));
      mine_mix(h, MN_SEP);
      for (uint32_t x = bpos; x < bpos + il; ++x) mine_mix(h, DC::W(c, CF_CAND_OFF + x));
      mine_mix(h, MN_SEP);
      for (uint32_t x = apos + dl; x < apos + dl + rc; ++x) mine_mix(h, DC::W(c, CF_IN_OFF + x));
      h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;  // (the low bits are what a narrowed hash keeps)
      if (slot < a.cap && seq < MN_MAX_SITES) {
        MineRec r;
        r.pair = p;
        r.pos = apos | dl << 8 | bpos << 16 | il << 24;
        r.abyte = mine_skip(a.blob, a0, a1, apos - lc);
        r.bbyte = mine_skip(a.blob, b0, b1, bpos);
        r.meta = lc | rc << 4 | fl << 8 | seq << 16;
        r.pattern = 0u;
        a.rec[slot] = r;
        a.key[slot] = h & a.hmask;
        a.val[slot] = slot;
      }
      ++slot; ++seq;
      apos += dl; bpos += il;
      i = j;
    }
  }
}

__global__ void k_mine_head(uint32_t S, const unsigned long long* __restrict__ skey, uint32_t* __restrict__ head) {
  const uint32_t p = blockIdx.x * MN_BLOCK + threadIdx.x;
  if (p >= S) return;
  head[p] = (p > 0 && skey[p] == skey[p - 1]) ? 0u : p;
}

// the same text: the same lengths of the four parts (and anchors, if they are part of the text) and the same code points -- decoded
// from the bytes again, since two byte strings can decode alike (malformed UTF-8)
__device__ inline bool mine_site_eq(const MineArgs& a, const MineRec& x, const MineRec& y) {
  const uint32_t mmask = a.anchors ? 0x3FFu : 0xFFu;
  if ((x.meta & mmask) != (y.meta & mmask) || ((x.pos ^ y.pos) & 0xFF00FF00u)) return false;
  const uint32_t na = (x.meta & 0xFu) + ((x.pos >> 8) & 0xFFu) + ((x.meta >> 4) & 0xFu), nb = x.pos >> 24;
  const uint32_t xa1 = a.off[x.pair + 1u] - 1u, ya1 = a.off[y.pair + 1u] - 1u, xb1 = a.off[a.n + x.pair + 1u] - 1u, yb1 = a.off[a.n + y.pair + 1u] - 1u;
  uint32_t px = x.abyte, py = y.abyte;
  for (uint32_t k = 0; k < na; ++k) {
    if (px >= xa1 || py >= ya1) return false;  // (never: the records were cut from these strings)
    uint32_t lx, ly;
    if (mine_cp_at(a.blob, px, xa1, &lx) != mine_cp_at(a.blob, py, ya1, &ly)) return false;
    px += lx; py += ly;
  }
  px = x.bbyte; py = y.bbyte;
  for (uint32_t k = 0; k < nb; ++k) {
    if (px >= xb1 || py >= yb1) return false;
    uint32_t lx, ly;
    if (mine_cp_at(a.blob, px, xb1, &lx) != mine_cp_at(a.blob, py, yb1, &ly)) return false;
    px += lx; py += ly;
  }
  return true;
}

// sorted position p: the first site of its hash run with the same code points is its representative (a site that matches none before
// it is one itself, and the first to match is always one: it matched none before it either).  rep[p] = that site's SORTED position.
__global__ void k_mine_rep(MineArgs a, uint32_t S, const uint32_t* __restrict__ sval, const uint32_t* __restrict__ rstart, uint32_t* __restrict__ rep,
                           uint32_t* __restrict__ iota, uint32_t* __restrict__ runflag) {
  const uint32_t p = blockIdx.x * MN_BLOCK + threadIdx.x;
  if (p >= S) return;
  const MineRec x = a.rec[sval[p]];
  uint32_t r = p;
  for (uint32_t q = rstart[p]; q < p; ++q)
    if (mine_site_eq(a, x, a.rec[sval[q]])) { r = q; break; }
  rep[p] = r;
  iota[p] = p;
  if (r == p && p != rstart[p] && atomicExch(&runflag[rstart[p]], 1u) == 0u) atomicAdd(&a.ctr[3], 1u);  // (a second text in the run: collisions only)
}

// x: position in the order by representative.  The site's summand and whether a new text starts here
__global__ void k_mine_seg(uint32_t S, const MineRec* __restrict__ rec, const uint32_t* __restrict__ sval, const uint32_t* __restrict__ rkey,
                           const uint32_t* __restrict__ rval, const uint32_t* __restrict__ count, MineSum* __restrict__ w, uint32_t* __restrict__ head) {
  const uint32_t x = blockIdx.x * MN_BLOCK + threadIdx.x;
  if (x >= S) return;
  const uint32_t pair = rec[sval[rval[x]]].pair;
  w[x] = MineSum{count ? (unsigned long long)count[pair] : 1ull, 1ull};
  head[x] = (x == 0 || rkey[x] != rkey[x - 1]) ? 1u : 0u;
}
__global__ void k_mine_pattern(uint32_t S, MineRec* __restrict__ rec, const uint32_t* __restrict__ sval, const uint32_t* __restrict__ rval,
                               const uint32_t* __restrict__ segid) {
  const uint32_t x = blockIdx.x * MN_BLOCK + threadIdx.x;
  if (x >= S) return;
  rec[sval[rval[x]]].pattern = segid[x] - 1u;
}
// row u of the chunk's table: the representative's record and the sums (uniq[u] = its sorted position)
__global__ void k_mine_rows(uint32_t S, const uint32_t* __restrict__ nuniq, const uint32_t* __restrict__ uniq, const MineSum* __restrict__ agg,
                            const MineRec* __restrict__ rec, const uint32_t* __restrict__ sval, MineRow* __restrict__ rows) {
  const uint32_t u = blockIdx.x * MN_BLOCK + threadIdx.x;
  if (u >= S || u >= *nuniq || uniq[u] >= S) return;
  const MineRec r = rec[sval[uniq[u]]];
  MineRow o;
  o.pair = r.pair; o.pos = r.pos; o.meta = r.meta & 0x3FFu; o._pad = 0u;
  o.count = agg[u].count; o.sites = agg[u].sites;
  rows[u] = o;
}
__global__ void k_mine_emit(uint32_t S, uint32_t n, const MineRec* __restrict__ rec, const uint32_t* __restrict__ off, const uint32_t* __restrict__ remap,
                            uint32_t nrows, uint32_t pair_base, anx_mine_site* __restrict__ out) {
  const uint32_t s = blockIdx.x * MN_BLOCK + threadIdx.x;
  if (s >= S) return;
  const MineRec r = rec[s];
  if (r.pair >= n) return;
  const uint32_t o = off[r.pair] + (r.meta >> 16);
  if (o >= S) return;
  anx_mine_site t;
  t.pair = pair_base + r.pair;
  t.a_pos = r.pos & 0xFFu; t.a_len = (r.pos >> 8) & 0xFFu; t.b_pos = (r.pos >> 16) & 0xFFu; t.b_len = r.pos >> 24;
  t.pattern = r.pattern < nrows ? remap[r.pattern] : 0xFFFFFFFFu;
  t.flags = (r.meta >> 8) & 3u;
  t._pad = 0u;
  out[o] = t;
}

inline unsigned grid_of(size_t n) { return (unsigned)std::max<size_t>(1, (n + MN_BLOCK - 1) / MN_BLOCK); }
}  // namespace

struct MineChunk {
  int device = 0;
  uint32_t n = 0, S = 0;
  MineRec* rec = nullptr;
  uint32_t* off = nullptr;  // [n + 1]
};
void mine_chunk_free(MineChunk* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->rec) pool_free(c->rec);
  if (c->off) pool_free(c->off);
  delete c;
}
size_t mine_chunk_sites(const MineChunk* c) { return c ? c->S : 0; }

int mine_chunk_run(const DeviceLexicon* dl, const PairSpan* a, const PairSpan* b, const uint32_t* counts, size_t n, uint32_t context, bool anchors,
                   bool keep_sites, MineChunk** chunk, std::vector<MineRow>& rows, std::vector<uint32_t>& host_pairs, uint64_t* stats,
                   uint64_t* bytes_up, uint64_t* bytes_down, std::string& err) {
  rows.clear();
  host_pairs.clear();
  *chunk = nullptr;
  if (n == 0) return ANX_OK;
  if (!dl) { err = "model is not resident on a device"; return ANX_ENODEVICE; }
  if (n > PAIRS_CHUNK || context > MINE_MAX_CONTEXT) { err = "mine_chunk_run: more than 2^20 pairs, or context beyond 8"; return ANX_EINVAL; }
  const size_t N2 = 2 * n;
  size_t text = 0;
  for (size_t i = 0; i < n; ++i) text += a[i].len + b[i].len + 2;
  if (text + 16 >= ((size_t)1 << 32)) { err = "pairs exceed 4 GB of text per 2^20 pairs"; return ANX_ELIMIT; }
  HIP_TRY(hipSetDevice(dl->device));
  PairScratch sc(dl->device);
  hipStream_t st = sc.st;
  // ---- one staging block: offsets [2 n + 1] | counts [n] | the blob ----
  const size_t o_cnt = (N2 + 1) * sizeof(uint32_t), o_blob = (o_cnt + (counts ? n : 0) * sizeof(uint32_t) + 15) & ~(size_t)15, in_bytes = o_blob + text + 16;
  char* h_in = static_cast<char*>(sc.pinned(in_bytes));
  if (!h_in) { err = "out of host memory"; return ANX_EINVAL; }
  {
    uint32_t* h_off = reinterpret_cast<uint32_t*>(h_in);
    char* h_blob = h_in + o_blob;
    size_t pos = 0;
    for (size_t s = 0; s < N2; ++s) {
      const PairSpan& sp = s < n ? a[s] : b[s - n];
      h_off[s] = (uint32_t)pos;
      if (sp.len) memcpy(h_blob + pos, sp.p, sp.len);
      h_blob[pos + sp.len] = '\0';
      pos += sp.len + 1;
    }
    h_off[N2] = (uint32_t)pos;
    memset(h_blob + pos, 0, 16);
    if (counts) memcpy(h_in + o_cnt, counts, n * sizeof(uint32_t));
  }
  char* d_in = nullptr;
  uint32_t *d_alpha = nullptr, *d_cnt = nullptr, *d_host = nullptr, *d_ctr = nullptr;
  uint32_t na = 0;
  const uint32_t(*al)[2] = alphabetic_ranges(&na);
  int rc;
  if ((rc = sc.get(&d_in, in_bytes, err)) || (rc = sc.get(&d_alpha, (size_t)na * 2, err)) || (rc = sc.get(&d_cnt, n + 1, err)) ||
      (rc = sc.get(&d_host, n, err)) || (rc = sc.get(&d_ctr, 4, err)))
    return rc;
  HIP_TRY(hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_alpha, al, (size_t)na * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  *bytes_up += in_bytes + (size_t)na * 8;
  const uint32_t blocks = std::min<uint32_t>(PAIRS_CF_BLOCKS, (uint32_t)((n + 63) / 64));
  void* wk = nullptr;
  if (pool_malloc(&wk, conf_small_work_bytes(blocks)) != hipSuccess) {  // no room for the working set: the chunk on the host (same results)
    (void)hipGetLastError();
    host_pairs.resize(n);
    for (size_t i = 0; i < n; ++i) host_pairs[i] = (uint32_t)i;
    return ANX_OK;
  }
  sc.blocks.v.push_back(wk);
  const int bits = switches().mine_hash_bits;
  MineArgs A{};
  A.n = (uint32_t)n; A.context = context; A.anchors = anchors ? 1u : 0u;
  A.blob = reinterpret_cast<const uint8_t*>(d_in + o_blob); A.off = reinterpret_cast<const uint32_t*>(d_in);
  A.alpha = reinterpret_cast<const uint32_t(*)[2]>(d_alpha); A.nalpha = na;
  A.work = static_cast<uint32_t*>(wk); A.cnt = d_cnt; A.hostlist = d_host; A.ctr = d_ctr;
  A.hmask = bits >= 63 ? 0x7FFFFFFFFFFFFFFFull : (1ull << bits) - 1;
  const uint32_t* d_count = counts ? reinterpret_cast<const uint32_t*>(d_in + o_cnt) : nullptr;
  // ---- the scripts.  Room for 8 sites per pair at first; a chunk with more is repeated with room for every site a pair can have ----
  struct RecHold { MineRec* p; hipStream_t st; ~RecHold() { if (p) { (void)hipStreamSynchronize(st); pool_free(p); } } } rec{nullptr, st};  // (nothing enqueued may still read it)
  uint32_t ctr[4] = {0, 0, 0, 0};
  for (int attempt = 0;; ++attempt) {
    const size_t full = n * MN_MAX_SITES, cap = attempt ? full : std::min<size_t>(full, 8 * n + 64);
    if (rec.p) { pool_free(rec.p); rec.p = nullptr; }
    HIP_TRY(pool_malloc(reinterpret_cast<void**>(&rec.p), cap * sizeof(MineRec)));
    if ((rc = sc.get(&A.key, cap, err)) || (rc = sc.get(&A.val, cap, err))) { (void)hipStreamSynchronize(st); return rc; }
    A.rec = rec.p; A.cap = (uint32_t)cap;
    HIP_TRY(hipMemsetAsync(d_ctr, 0, 16, st));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, (n + 1) * sizeof(uint32_t), st));
    const int kt = ktimer_begin("k_mine_script", st);
    hipLaunchKernelGGL(k_mine_script, dim3(blocks), dim3(CF_THREADS), 0, st, A);
    ktimer_end(kt, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ctr, d_ctr, 16, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); err = std::string("k_mine_script: ") + hipGetErrorString(e); return ANX_ENODEVICE; }
    if (ctr[0] <= cap) break;
    if (attempt) { err = "mine: more sites than a chunk can have"; return ANX_EINVAL; }
  }
  const uint32_t S = ctr[0], nh = std::min<uint32_t>(ctr[1], (uint32_t)n);
  stats[5] += ctr[2];
  if (nh) {
    host_pairs.resize(nh);
    HIP_TRY(hipMemcpyAsync(host_pairs.data(), d_host, nh * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::sort(host_pairs.begin(), host_pairs.end());
    *bytes_down += nh * sizeof(uint32_t);
  }
  *bytes_down += 16;
  if (S == 0) return ANX_OK;
  // ---- the histogram ----
  unsigned long long* d_skey = nullptr;
  uint32_t *d_sval = nullptr, *d_head = nullptr, *d_rep = nullptr, *d_iota = nullptr, *d_flag = nullptr, *d_rkey = nullptr, *d_rval = nullptr, *d_seg = nullptr,
           *d_uniq = nullptr, *d_nuniq = nullptr;
  MineSum *d_w = nullptr, *d_agg = nullptr;
  MineRow* d_rows = nullptr;
  if ((rc = sc.get(&d_skey, S, err)) || (rc = sc.get(&d_sval, S, err)) || (rc = sc.get(&d_head, S, err)) || (rc = sc.get(&d_rep, S, err)) ||
      (rc = sc.get(&d_iota, S, err)) || (rc = sc.get(&d_flag, S, err)) || (rc = sc.get(&d_rkey, S, err)) || (rc = sc.get(&d_rval, S, err)) ||
      (rc = sc.get(&d_seg, S, err)) || (rc = sc.get(&d_uniq, S, err)) || (rc = sc.get(&d_nuniq, 4, err)) || (rc = sc.get(&d_w, S, err)) ||
      (rc = sc.get(&d_agg, S, err)) || (rc = sc.get(&d_rows, S, err)))
    return rc;
  uint32_t sbits = 1;
  while (sbits < 32 && (1ull << sbits) < S) ++sbits;
  size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, t1, A.key, d_skey, A.val, d_sval, (size_t)S, 0, 64, st));
  HIP_TRY(rocprim::inclusive_scan(nullptr, t2, d_head, d_head, (size_t)S, rocprim::maximum<uint32_t>(), st));
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, t3, d_rep, d_rkey, d_iota, d_rval, (size_t)S, 0u, sbits, st));
  HIP_TRY(rocprim::inclusive_scan(nullptr, t4, d_head, d_seg, (size_t)S, rocprim::plus<uint32_t>(), st));
  HIP_TRY(rocprim::reduce_by_key(nullptr, t5, d_rkey, d_w, (size_t)S, d_uniq, d_agg, d_nuniq, MineSumPlus(), rocprim::equal_to<uint32_t>(), st));
  char* tmp = nullptr;
  const size_t tbytes = std::max({t1, t2, t3, t4, t5}) + 16;
  if ((rc = sc.get(&tmp, tbytes, err))) return rc;
  HIP_TRY(hipMemsetAsync(d_flag, 0, (size_t)S * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(d_nuniq, 0, 16, st));
  const int ks = ktimer_begin("k_mine_sort", st);
  HIP_TRY(rocprim::radix_sort_pairs(tmp, t1, A.key, d_skey, A.val, d_sval, (size_t)S, 0, 64, st));
  ktimer_end(ks, st);
  const int kr = ktimer_begin("k_mine_reduce", st);
  hipLaunchKernelGGL(k_mine_head, dim3(grid_of(S)), dim3(MN_BLOCK), 0, st, S, d_skey, d_head);
  HIP_TRY(rocprim::inclusive_scan(tmp, t2, d_head, d_head, (size_t)S, rocprim::maximum<uint32_t>(), st));
  hipLaunchKernelGGL(k_mine_rep, dim3(grid_of(S)), dim3(MN_BLOCK), 0, st, A, S, d_sval, d_head, d_rep, d_iota, d_flag);
  HIP_TRY(rocprim::radix_sort_pairs(tmp, t3, d_rep, d_rkey, d_iota, d_rval, (size_t)S, 0u, sbits, st));
  hipLaunchKernelGGL(k_mine_seg, dim3(grid_of(S)), dim3(MN_BLOCK), 0, st, S, rec.p, d_sval, d_rkey, d_rval, d_count, d_w, d_head);
  HIP_TRY(rocprim::inclusive_scan(tmp, t4, d_head, d_seg, (size_t)S, rocprim::plus<uint32_t>(), st));
  HIP_TRY(rocprim::reduce_by_key(tmp, t5, d_rkey, d_w, (size_t)S, d_uniq, d_agg, d_nuniq, MineSumPlus(), rocprim::equal_to<uint32_t>(), st));
  hipLaunchKernelGGL(k_mine_pattern, dim3(grid_of(S)), dim3(MN_BLOCK), 0, st, S, rec.p, d_sval, d_rval, d_seg);
  hipLaunchKernelGGL(k_mine_rows, dim3(grid_of(S)), dim3(MN_BLOCK), 0, st, S, d_nuniq, d_uniq, d_agg, rec.p, d_sval, d_rows);
  ktimer_end(kr, st);
  uint32_t* d_off = nullptr;
  if (keep_sites) {
    HIP_TRY(pool_malloc(reinterpret_cast<void**>(&d_off), (n + 1) * sizeof(uint32_t)));
    size_t t6 = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, t6, d_cnt, d_off, 0u, n + 1, rocprim::plus<uint32_t>(), st);
    char* tmp6 = nullptr;
    if (e == hipSuccess && sc.get(&tmp6, t6 + 16, err)) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = rocprim::exclusive_scan(tmp6, t6, d_cnt, d_off, 0u, n + 1, rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); pool_free(d_off); err = std::string("mine: site offsets: ") + hipGetErrorString(e); return ANX_ENODEVICE; }
  }
  struct OffHold { uint32_t* p; hipStream_t st; ~OffHold() { if (p) { (void)hipStreamSynchronize(st); pool_free(p); } } } offh{d_off, st};
  HIP_TRY(hipGetLastError());
  uint32_t tot[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(&tot[0], d_nuniq, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&tot[1], d_ctr + 3, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint32_t D = tot[0];
  if (D == 0 || D > S) { err = "mine: inconsistent totals"; return ANX_EINVAL; }
  stats[4] += tot[1];
  rows.resize(D);
  HIP_TRY(hipMemcpyAsync(rows.data(), d_rows, (size_t)D * sizeof(MineRow), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *bytes_down += (size_t)D * sizeof(MineRow) + 8;
  if (keep_sites) {
    MineChunk* c = new MineChunk();
    c->device = dl->device; c->n = (uint32_t)n; c->S = S; c->rec = rec.p; c->off = d_off;
    rec.p = nullptr;
    offh.p = nullptr;
    *chunk = c;
  }
  return ANX_OK;
}

int mine_chunk_emit(MineChunk* c, const uint32_t* remap, size_t nrows, uint32_t pair_base, anx_mine_site* out, uint32_t* off, uint64_t* bytes_down,
                    std::string& err) {
  if (!c || !c->S) return ANX_OK;
  HIP_TRY(hipSetDevice(c->device));
  PairScratch sc(c->device);
  hipStream_t st = sc.st;
  uint32_t* d_remap = nullptr;
  anx_mine_site* d_out = nullptr;
  int rc;
  if ((rc = sc.get(&d_remap, nrows, err)) || (rc = sc.get(&d_out, c->S, err))) return rc;
  HIP_TRY(hipMemcpyAsync(d_remap, remap, nrows * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_out, 0xFF, (size_t)c->S * sizeof(anx_mine_site), st));
  hipLaunchKernelGGL(k_mine_emit, dim3(grid_of(c->S)), dim3(MN_BLOCK), 0, st, c->S, c->n, c->rec, c->off, d_remap, (uint32_t)nrows, pair_base, d_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)c->S * sizeof(anx_mine_site), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(off, c->off, ((size_t)c->n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *bytes_down += (size_t)c->S * sizeof(anx_mine_site) + ((size_t)c->n + 1) * sizeof(uint32_t);
  return ANX_OK;
}

}  // namespace anx
