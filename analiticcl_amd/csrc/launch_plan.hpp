// launch_plan.hpp -- how a find_variants run launches its kernels: ONE copy of every rule the two host drivers share
// Part of the single translation unit engine.hip (included inside namespace anx, ahead of the batch pipeline); gfx950 only.
//
// batch_launch (engine.hip) and small_find (small_path.hpp) enqueue the same chain, scan -> filter/score -> compact -> rank.  Here: the lexicon
// side of the kernel arguments, the scoring plan and the dispatch over every template parameter.  What differs between the two on purpose
// (chunk and block sizes, use_nw8, when k_score_fast8 runs, the FsCold upload, error handling) stays at their call sites.  Plain inline
// functions: the one-input small call takes 66 us end to end and this code is on its path.
#pragma once

// ---- scan ------------------------------------------------------------------------------------------------------------------------------
// One scan stage: everything of ScanArgs that is not the lexicon's.  The batch path (engine.hip scan_stage_launch), the small call
// (launch_scan_small below) and the test hook debug_scan_pairs fill this and nothing else.
struct ScanStage {
  const Tile* tiles;       // in launch order: [tiles that stream an adjacency list | other bit-plane tiles | count-vector tiles]
  uint32_t ntiles;
  uint32_t n_adj_tiles, n_sad_tiles;  // the batch path's launch split (the small call's one launch looks at every tile itself)
  const uint32_t *q_bits, *q_cv;
  const uint4* q_rec;
  const uint32_t* qexact;
  uint2* raw;
  uint32_t region_cap;     // pair-list slots per region
  uint32_t* rctr;
  uint32_t chunk, chunk_fused, chunk_first;
  int want_exact, drop_len, fuse, twins;
  uint32_t* qpairs;        // per-query pair counts, or nullptr
  int dbg;
};
// the ONE fill of the kernels' arguments: the lexicon side and the stage
static inline ScanArgs scan_args_of(const DeviceLexicon* dl, const ScanStage& S) {
  ScanArgs A{};
  A.cls_bits = dl->cls_bits; A.cls_planes = dl->cls_planes; A.scan_rec = dl->scan_rec; A.scan_rec34 = dl->scan_rec34; A.pad_rec = dl->nentries; A.cstride = dl->cstride; A.pad_class = dl->nclasses;
  A.cls_len = dl->cls_len; A.cls_off = dl->cls_off; A.sig = dl->sig; A.sig_e = dl->sig_e; A.sig_cbeg = dl->sig_cbeg; A.sighash = dl->sighash; A.sighash_e = dl->sighash_e; A.hash_mask = dl->hash_mask; A.ball = dl->ball;
  A.adj_hdr = dl->adj_hdr; A.adj_planes = dl->adj_planes; A.adj_ids = dl->adj_ids;
  A.e_rec = dl->e_rec;
  A.tiles = S.tiles; A.ntiles = S.ntiles; A.q_bits = S.q_bits; A.q_cv = S.q_cv; A.q_rec = S.q_rec; A.qexact = S.qexact;
  A.raw = S.raw; A.region_cap = S.region_cap; A.rctr = S.rctr;
  A.chunk = S.chunk; A.chunk_fused = S.chunk_fused; A.chunk_first = S.chunk_first;
  A.want_exact = S.want_exact; A.drop_len = S.drop_len; A.fuse = S.fuse; A.twins = S.twins;
  A.qpairs = S.qpairs; A.dbg = S.dbg;
  return A;
}
// f(std::integral_constant<int, NP>) for the count-vector width the kernels of the SAD tiles are instantiated for (launch_scan<NP>, k_scan_small<NP>)
template <typename F>
static inline void with_nplanes(int nplanes, F&& f) {
  switch (nplanes) {
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 24: f(std::integral_constant<int, 24>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 42>{}); break;
  }
}
// the small call's flat reservations (SCAN_CHUNK / SCAN_CHUNK_FUSED of the batch path: 256 / 128 -- a wave here holds a share of ONE query's pairs)
constexpr uint32_t SMALL_CHUNK = 64, SMALL_CHUNK_FUSED = 32, SMALL_CHUNK_FIRST = 64;
// the small call's scan as small_find and the test hook both launch it: ONE launch of k_scan_small over every tile slot, a wave per slot
static inline void launch_scan_small(const DeviceLexicon* dl, const ScanStage& S, hipStream_t st) {
  const ScanArgs A = scan_args_of(dl, S);
  const dim3 grid((A.ntiles + 3) / 4);
  const int kt = ktimer_begin("k_scan_small", st);  // (off unless anx_debug_kernel_timer(1): no event, no launch)
  with_nplanes(dl->nplanes, [&](auto np) { hipLaunchKernelGGL(k_scan_small<decltype(np)::value>, grid, dim3(256), 0, st, A); });
  ktimer_end(kt, st);
}

// ---- score -----------------------------------------------------------------------------------------------------------------------------
struct ScorePlan {
  ScoreArgs sa;        // everything but dbg and store_pairs (0 here: the caller's)
  uint32_t threads;    // lanes per block of k_score_pairs: 256, 128 or 64 -- the most whose per-lane state fits the 64 KB of LDS; 0: not even 64 do
  int fastD;           // 1..3: k_filter_score scores a short pair inline (register DL for this d); 0: every pair goes to the slot lists
  bool have_long_q;    // some query row is wider than 16 symbols
  int enable_filter;   // ANX_PREFILTER (0: every length-compatible pair goes to the DL)
  bool split_wide;     // the 8-word prefilter of the wide pairs (a string of 17..32 symbols) runs in k_filter_wide: its state inline costs the fused kernel 105 instead of 70 VGPRs
  bool b7;             // the one-add zero test of the prefilter: every symbol code (classes, unknown = A + 1) below the masked paddings 0x7E / 0x7F
  bool planes;         // symbol planes instead of byte rows for the inline DL and its tail (codes + 1 in six bits)
  bool fits() const { return threads != 0; }
  size_t lds_bytes() const { return (size_t)threads * sa.stride; }  // dynamic LDS of k_score_pairs / k_small_lists
};
// qw: 16-byte words per query row, d: the largest edit distance of the run.  The switches are read once per plan.
static inline ScorePlan score_plan_of(const HostModel& m, const DeviceLexicon* dl, double score_threshold, uint32_t qw, uint32_t d) {
  const Switches& sw = switches();
  ScorePlan pl{};
  ScoreArgs& sa = pl.sa;
  sa.quot = dl->quot;
  sa.w_ld = m.weights.ld; sa.w_lcs = m.weights.lcs; sa.w_prefix = m.weights.prefix; sa.w_suffix = m.weights.suffix; sa.w_case = m.weights.casew;
  sa.w_sum = m.weights.ld + m.weights.lcs + m.weights.prefix + m.weights.suffix + m.weights.casew;  // src/types.rs:69-73
  sa.score_threshold = score_threshold;
  sa.have_freq = m.have_freq ? 1 : 0;
  sa.any_variants = dl->any_variants;  // the scoring kernels count a survivor's EXPANDED rows into qsurv and set qexpand
  sa.lqp = qw * 16;
  sa.lcp = (dl->max_len + 15) / 16 * 16;
  uint32_t stride = sa.lqp + sa.lcp + (d + 2) * (2 * d + 3);  // per lane: query row, candidate row, the rows of the DL
  stride = (stride + 3) / 4;
  if ((stride & 1) == 0) stride++;  // an odd number of dwords: conflict-free ds access
  sa.stride = stride * 4;
  sa.qw = qw;
  pl.threads = 256;
  while (pl.threads > 64 && (size_t)pl.threads * sa.stride > 64 * 1024) pl.threads >>= 1;
  if ((size_t)pl.threads * sa.stride > 64 * 1024) pl.threads = 0;
  pl.have_long_q = qw > 1;
  pl.enable_filter = sw.prefilter;
  pl.fastD = (sw.score_fast && d >= 1 && d <= 3) ? (int)d : 0;
  pl.split_wide = sw.fs_split != 0;
  pl.b7 = sw.fs_b7 && m.alphabet.size() + 1 < 0x7E;
  pl.planes = pl.b7 && sw.fs_planes && (int)m.alphabet.size() <= kSymbolPlanesMaxA;
  return pl;
}
// the three slot lists of the pairs k_filter_score does not score inline, their counters side by side in lctr
struct SlotLists { SlotList l8, lg, lw; };  // strings of 17..32 symbols (8-word kernel) | everything else | wide pairs not yet prefiltered
static inline SlotLists slot_lists_of(uint32_t* list8, uint32_t* listg, uint32_t* listw, uint32_t* lctr, uint32_t cap) {
  return SlotLists{{list8, lctr, cap}, {listg, lctr + SCAN_REGIONS * RC_STRIDE, cap}, {listw, lctr + 2 * SCAN_REGIONS * RC_STRIDE, cap}};
}
// the lexicon side and the run's arrays (p_score / p_meta: the per-slot outputs of the debug view of every pair, or nullptr)
static inline PairArgs pair_args_of(const DeviceLexicon* dl, const uint2* raw, const uint32_t* q_meta, const uint4* q_rows, const uint4* q_rec, double* p_score, uint32_t* p_meta,
                                    uint32_t* qmaxfreq, uint32_t* qsurv, uint32_t* qexpand) {
  return PairArgs{raw, q_meta, q_rows, q_rec, dl->e_rec, dl->ent_meta, dl->ent_rowoff, dl->rows, dl->ent_freq, dl->ent_var_off, p_score, p_meta, qmaxfreq, qsurv, qexpand, dl->e_planes};
}

// k_filter_score<D, WIDE, MODE>: D = fastD, WIDE = !split_wide, MODE 0 byte rows / 1 byte rows + b7 / 2 symbol planes (only without WIDE):
// the 20 instances, named here and nowhere else
template <int D, bool WIDE, int MODE>
static inline void launch_filter_score_as(dim3 grid, hipStream_t st, const FilterArgs& fa, const PairArgs& pa, const FsCold* cold) {
  hipLaunchKernelGGL((k_filter_score<D, WIDE, MODE>), grid, dim3(256), 0, st, fa, pa, cold);
}
template <bool WIDE, int MODE>
static inline void launch_filter_score_d(int fastD, dim3 grid, hipStream_t st, const FilterArgs& fa, const PairArgs& pa, const FsCold* cold) {
  switch (fastD) {
    case 1: launch_filter_score_as<1, WIDE, MODE>(grid, st, fa, pa, cold); break;
    case 2: launch_filter_score_as<2, WIDE, MODE>(grid, st, fa, pa, cold); break;
    case 3: launch_filter_score_as<3, WIDE, MODE>(grid, st, fa, pa, cold); break;
    default: launch_filter_score_as<0, WIDE, MODE>(grid, st, fa, pa, cold); break;
  }
}
static inline void launch_filter_score(const ScorePlan& pl, dim3 grid, hipStream_t st, const FilterArgs& fa, const PairArgs& pa, const FsCold* cold) {
  if (pl.split_wide) {
    if (pl.planes) launch_filter_score_d<false, 2>(pl.fastD, grid, st, fa, pa, cold);
    else if (pl.b7) launch_filter_score_d<false, 1>(pl.fastD, grid, st, fa, pa, cold);
    else launch_filter_score_d<false, 0>(pl.fastD, grid, st, fa, pa, cold);
  } else {  // (ANX_FS_SPLIT=0, A/B: byte rows)
    if (pl.b7) launch_filter_score_d<true, 1>(pl.fastD, grid, st, fa, pa, cold);
    else launch_filter_score_d<true, 0>(pl.fastD, grid, st, fa, pa, cold);
  }
}
// k_score_fast8<fastD> over list8 (fastD = 1..3)
static inline void launch_score_fast8(int fastD, dim3 grid, hipStream_t st, const SlotList& l8, const PairArgs& pa, const ScoreArgs& sa, const SurvOut& so) {
  if (fastD == 1) hipLaunchKernelGGL(k_score_fast8<1>, grid, dim3(256), 0, st, l8, pa, sa, so);
  else if (fastD == 2) hipLaunchKernelGGL(k_score_fast8<2>, grid, dim3(256), 0, st, l8, pa, sa, so);
  else hipLaunchKernelGGL(k_score_fast8<3>, grid, dim3(256), 0, st, l8, pa, sa, so);
}
// k_small_lists<fastD>: k_filter_wide + k_score_fast8 + k_score_pairs as one launch of 256 threads, a block per region
static inline void launch_small_lists(const ScorePlan& pl, hipStream_t st, const SmallListArgs& L, const FilterArgs& fa, const PairArgs& pa, const SurvOut& so) {
  const dim3 grid(SCAN_REGIONS);
  const size_t dyn = pl.lds_bytes();
  if (pl.fastD == 1) hipLaunchKernelGGL(k_small_lists<1>, grid, dim3(256), dyn, st, L, fa, pa, pl.sa, so);
  else if (pl.fastD == 2) hipLaunchKernelGGL(k_small_lists<2>, grid, dim3(256), dyn, st, L, fa, pa, pl.sa, so);
  else if (pl.fastD == 3) hipLaunchKernelGGL(k_small_lists<3>, grid, dim3(256), dyn, st, L, fa, pa, pl.sa, so);
  else hipLaunchKernelGGL(k_small_lists<0>, grid, dim3(256), dyn, st, L, fa, pa, pl.sa, so);
}

// the one launch as small_find and the scoring door (engine.hip score_stage_launch) both make it, for a plan of 256 threads: the deferred wide
// prefilter when the plan splits it off, k_score_fast8's part whenever the batch has the inline DL (long queries or not: use_nw8 is on then)
static inline void launch_small_lists_of(const ScorePlan& pl, hipStream_t st, const SlotLists& sl, const FilterArgs& fa, const PairArgs& pa, const SurvOut& so) {
  const int do_wide = (pl.split_wide && pl.enable_filter) ? 1 : 0;
  launch_small_lists(pl, st, SmallListArgs{sl.lw, sl.l8, sl.lg, do_wide, pl.fastD ? 1 : 0, pl.fastD}, fa, pa, so);
}

// ---- rank ------------------------------------------------------------------------------------------------------------------------------
// cutoff: the caller's cutoff_threshold, or 0 when something after k_rank cuts off instead (batch path, late device confusables)
static inline RankArgs rank_args_of(const HostModel& m, const DeviceLexicon* dl, const anx_params& p, double cutoff) {
  RankArgs ra{};
  ra.cutoff_threshold = cutoff;
  ra.max_matches = p.max_matches;
  ra.freq_weight = p.freq_weight;
  ra.have_freq = m.have_freq ? 1 : 0;
  ra.any_variants = dl->any_variants;
  return ra;
}
// k_rank<true> for models without variant lists at freq_weight == 0, k_rank<false> otherwise
static inline void launch_rank(const RankArgs& ra, hipStream_t st, uint32_t nq, const uint32_t* soff, const SurvRow* c_rows, const uint32_t* qmaxfreq, const uint32_t* qexpand, double* t_key,
                               DevRow* r_rows, uint32_t* r_count, uint32_t row_cap, const uint32_t* overflow, const SegRows& seg) {
  const dim3 grid((nq + 4 * RANK_QPW - 1) / (4 * RANK_QPW));
  if (!ra.any_variants && ra.freq_weight == 0.0f) hipLaunchKernelGGL(k_rank<true>, grid, dim3(256), 0, st, nq, soff, c_rows, qmaxfreq, qexpand, ra, t_key, r_rows, r_count, row_cap, overflow, seg);
  else hipLaunchKernelGGL(k_rank<false>, grid, dim3(256), 0, st, nq, soff, c_rows, qmaxfreq, qexpand, ra, t_key, r_rows, r_count, row_cap, overflow, seg);
}
