// small_path.hpp -- the small call: find_variants for a handful of inputs at the reference's own granularity
// Part of the single translation unit engine.hip (included inside namespace anx, after the batch pipeline); gfx950 only.
// How the chain is launched -- kernel arguments, the scoring plan, every template dispatch -- is launch_plan.hpp, shared with batch_launch.
//
// The reference's callers hand find_variants ONE string (/root/reference/src/lib.rs:972) and fan out in batches of 1 000
// (src/bin/analiticcl.rs:416,445-448; bindings/python/src/lib.rs:704-749).  The batch pipeline above is built for a million queries:
// ~45 launches and 5 host waits in its encoder (radix sorts, tile sort), ~35 commands and a dozen pool allocations per run, events,
// a pageable download -- 0.3 ms for one query, 0.65 ms for a thousand (round 6, tools/fresh_batch.py small).  A call of at most
// SMALL_MAX inputs of at most SMALL_MAX_BYTES bytes takes this path instead:
//   * a context (stream, pinned staging, every device buffer at its fixed capacity) is checked out of a per-device pool: no allocation,
//     no event, no memset command per call;
//   * the inputs are packed into pinned memory the encoder kernels read over PCIe; queries stay in INPUT order (no sort, no
//     permutation), one scan tile per query (k_small_tiles), capacities are fixed and every append is bounds-checked as always;
//   * nine launches -- k_enc_strings, k_small_tiles (with k_enc_gather's work) | k_scan_small (all three scan bodies in one launch) |
//     k_filter_score, k_small_lists (k_filter_wide + k_score_fast8 + k_score_pairs, a block per region) | k_small_offsets,
//     k_compact_grouped, k_rank | k_small_fetch (rows and offsets straight into pinned host memory, with the run's fills) -- and ONE host wait
//     (eleven in the first version: 66 us for one input);
//   * a model with variant lists launches k_compact_expand in k_compact_grouped's place (a survivor's rows: its VariantOf references, then
//     itself unless TRANSPARENT) and k_rank<false>; the launch count and the one host wait stay.  The expanded rows meet the same fixed
//     capacities: an entry with many references first fills the caller's block of ranked rows (16 n + 64 rows: what survives dedup and crop
//     of a call of n inputs), and only for the largest calls the context's candidate rows (16 * 4096 + 1024 for the call, before the crop);
//   * a model with a confusable list (weighted on the device: conf.hip) adds four launches, conf_launch_small -- k_conf_screen,
//     k_small_conf_order (a single-block LDS counting sort in place of the batch path's key / iota / radix sort), k_conf_script, k_conf_apply_* --
//     after k_rank (late: k_rank without the cutoff, k_conf_apply_late cuts off) or between the compaction and k_rank (early,
//     confusables_before_pruning): thirteen launches, still one host wait.  k_enc_strings leaves the bytes it staged on the device for them;
//     the weights, the list, its order and k_conf_script's working set (SMALL_CF_BLOCKS waves, 60 MB) are the context's, created the first time it
//     serves such a model.  A row the fixed working memory cannot weight (a string beyond 64 code points) discards the run like an overflow;
//   * a run whose fills exceeded a fixed capacity (a handful of very short queries can) is discarded and the call takes the batch path.
// Same kernels, same arithmetic as the batch path: the results are identical (tests/test_gpu_small.py: against the batch path and the oracle).
#pragma once

constexpr uint32_t SMALL_MAX_BYTES = 64;     // longest input (bytes) the small path takes: query rows of <= 4 words
constexpr uint32_t SMALL_SHIFT = 15;         // pair-list slots per region (2 M slots in all)
constexpr uint32_t SMALL_SURV_CAP = 16384;   // survivor records / slot-list entries per region
constexpr uint32_t SMALL_LIST_BLOCKS = 2;    // blocks per region of the slot-list kernels (LIST_P of the batch path: 64)
constexpr uint32_t SMALL_FS_BLK = 512;       // pair-list slots per block of k_filter_score (FS_BLK = 4096 in the batch path)
constexpr uint32_t SMALL_FETCH_BLOCKS = 8;   // blocks of k_small_fetch: each computes the offsets, copies a share of the rows
constexpr uint32_t SMALL_ROWS_PER_Q = 16;    // candidate rows per query the row buffers hold on average
constexpr uint32_t SMALL_CF_BLOCKS = 160;    // one-wave blocks of k_conf_script (it strides): 160 x 371 KB = 60 MB of working set per context, not the 386 MB one wave per 64 row slots would be

struct SmallCtx {
  int device = 0;
  hipStream_t st = nullptr;
  char* h_in = nullptr;        // pinned: [blob | offsets u32[SMALL_MAX + 1]]
  char* h_out = nullptr;       // pinned: [SmallCtl | offsets u64[SMALL_MAX + 1]]
  SmallEnc enc;
  uint32_t *counters = nullptr, *rctr = nullptr, *sctr = nullptr, *lctr = nullptr, *qsurv = nullptr, *soff = nullptr, *qcur = nullptr, *qmaxfreq = nullptr, *qexpand = nullptr,
           *r_count = nullptr;
  uint2* raw = nullptr;
  SurvRec* surv = nullptr;
  uint32_t *list8 = nullptr, *listg = nullptr, *listw = nullptr;
  SurvRow* c_rows = nullptr;
  DevRow* r_rows = nullptr;
  double* t_key = nullptr;
  FsCold* d_cold = nullptr;
  FsCold h_cold_last;          // what d_cold holds (uploaded again only when it changes: cold_key)
  double cold_key[13] = {};
  bool cold_valid = false;
  int nplanes = 0;             // count-vector dwords the buffers were sized for
  std::vector<void*> blocks;   // device allocations (pool)
  size_t row_cap = 0;
  SmallConf cf;                // confusable weighting: created by small_ctx_conf the first time the context serves a model with confusables
  bool cf_ready = false;
};
constexpr size_t SMALL_IN_BLOB = (size_t)SMALL_MAX * (SMALL_MAX_BYTES + 1) + 64;

static void small_ctx_destroy(SmallCtx* c) {  // (the current device is the context's)
  if (!c) return;
  if (c->st) (void)hipStreamSynchronize(c->st);
  for (void* p : c->blocks) pool_free(p);
  if (c->h_in) (void)hipHostFree(c->h_in);
  if (c->h_out) (void)hipHostFree(c->h_out);
  if (c->st) (void)hipStreamDestroy(c->st);
  delete c;
}
static SmallCtx* small_ctx_create(const DeviceLexicon* dl, std::string& err) {
  std::unique_ptr<SmallCtx, void (*)(SmallCtx*)> c(new SmallCtx(), small_ctx_destroy);
  c->device = dl->device;
  c->nplanes = 42;  // the widest count vector: a context serves every model of the device
  c->st = static_cast<hipStream_t>(make_stream(true));
  if (!c->st) { err = "small path: no stream"; return nullptr; }
  auto pinned = [&](char** p, size_t bytes) { return hipHostMalloc(reinterpret_cast<void**>(p), bytes, hipHostMallocDefault) == hipSuccess; };
  if (!pinned(&c->h_in, SMALL_IN_BLOB + (SMALL_MAX + 1) * sizeof(uint32_t)) || !pinned(&c->h_out, 64 + (SMALL_MAX + 1) * sizeof(unsigned long long))) {
    (void)hipGetLastError();
    err = "small path: pinned staging";
    return nullptr;
  }
  bool ok = true;
  auto dev = [&](auto** p, size_t count) {
    void* q = nullptr;
    if (!ok || pool_malloc(&q, std::max<size_t>(count * sizeof(**p), 16)) != hipSuccess) { ok = false; return; }
    c->blocks.push_back(q);
    *p = static_cast<std::remove_reference_t<decltype(*p)>>(q);
  };
  const size_t N = SMALL_MAX, NP = (size_t)c->nplanes, QW = (SMALL_MAX_BYTES + 15) / 16;
  SmallEnc& e = c->enc;
  dev(&e.codes, SMALL_IN_BLOB + 4 * N + 16); dev(&e.meta, N); dev(&e.bits, N * NBITPLANES); dev(&e.kind, N); dev(&e.cv, N * NP); dev(&e.blk, 3 * (N / 256 + 1));
  dev(&e.perm, N); dev(&e.key, N); dev(&e.sig, N);
  dev(&e.q_rec, 2 * N); dev(&e.q_rows, N * QW); dev(&e.q_bits, N * NBITPLANES); dev(&e.q_cv, N * NP); dev(&e.q_meta, N); dev(&e.q_orig, N); dev(&e.qexact, N);
  dev(&e.s_kind, N); dev(&e.s_sig, N); dev(&e.tiles, 8 * N);
  dev(&c->counters, CTR_N); dev(&c->rctr, SCAN_REGIONS * RC_STRIDE); dev(&c->sctr, SCAN_REGIONS * RC_STRIDE); dev(&c->lctr, 3 * SCAN_REGIONS * RC_STRIDE);
  dev(&c->qsurv, N); dev(&c->soff, N + 1); dev(&c->qcur, N); dev(&c->qmaxfreq, N); dev(&c->qexpand, N); dev(&c->r_count, N);
  dev(&c->raw, (size_t)SCAN_REGIONS << SMALL_SHIFT);
  dev(&c->surv, (size_t)SCAN_REGIONS * SMALL_SURV_CAP);
  dev(&c->list8, (size_t)SCAN_REGIONS * SMALL_SURV_CAP); dev(&c->listg, (size_t)SCAN_REGIONS * SMALL_SURV_CAP); dev(&c->listw, (size_t)SCAN_REGIONS * SMALL_SURV_CAP);
  c->row_cap = N * SMALL_ROWS_PER_Q + 1024;
  dev(&c->c_rows, c->row_cap); dev(&c->r_rows, c->row_cap); dev(&c->t_key, c->row_cap);
  dev(&c->d_cold, 1);
  if (!ok) { (void)hipGetLastError(); err = "small path: device buffers"; return nullptr; }
  if (small_iota(e.perm, SMALL_MAX, c->st) != ANX_OK || hipStreamSynchronize(c->st) != hipSuccess) { err = "small path: set-up kernel"; return nullptr; }
  return c.release();
}
// The buffers of the confusable chain, once per context; false: no room (the call takes the batch path, a later call tries again)
static bool small_ctx_conf(SmallCtx* c) {
  if (c->cf_ready) return true;
  const size_t mark = c->blocks.size();
  bool ok = true;
  auto dev = [&](auto** p, size_t bytes) {
    void* q = nullptr;
    if (!ok || pool_malloc(&q, bytes) != hipSuccess) { ok = false; return; }
    c->blocks.push_back(q);
    *p = static_cast<std::remove_reference_t<decltype(*p)>>(q);
  };
  SmallConf f;
  uint8_t* text = nullptr;
  uint32_t* textoff = nullptr;
  dev(&f.weight, c->row_cap * sizeof(double)); dev(&f.need, c->row_cap * sizeof(uint2)); dev(&f.key, c->row_cap * sizeof(uint32_t)); dev(&f.order, c->row_cap * sizeof(uint32_t));
  dev(&f.ctr, 8 * sizeof(uint32_t)); dev(&text, SMALL_IN_BLOB); dev(&textoff, (SMALL_MAX + 1) * sizeof(uint32_t));
  dev(&f.work, conf_small_work_bytes(SMALL_CF_BLOCKS));
  if (!ok) {
    (void)hipGetLastError();
    for (size_t i = mark; i < c->blocks.size(); ++i) pool_free(c->blocks[i]);
    c->blocks.resize(mark);
    return false;
  }
  f.work_blocks = SMALL_CF_BLOCKS;
  c->cf = f; c->enc.text = text; c->enc.textoff = textoff;
  c->cf_ready = true;
  return true;
}
// the idle contexts of a device, checked out per call
namespace {
struct SmallIdle { std::mutex mu; std::vector<SmallCtx*> v; };
SmallIdle& small_idle_of(int device) {
  static SmallIdle idle[64];
  return idle[device >= 0 && device < 64 ? device : 0];
}
}  // namespace
static SmallCtx* small_ctx_acquire(const DeviceLexicon* dl, std::string& err) {
  SmallIdle& si = small_idle_of(dl->device);
  {
    std::lock_guard<std::mutex> g(si.mu);
    if (!si.v.empty()) { SmallCtx* c = si.v.back(); si.v.pop_back(); return c; }
  }
  return small_ctx_create(dl, err);
}
static void small_ctx_release(SmallCtx* c) {
  SmallIdle& si = small_idle_of(c->device);
  std::lock_guard<std::mutex> g(si.mu);
  si.v.push_back(c);
}
void small_ctxs_destroy(int device) {  // (the current device is `device`; runtime.hip pool_trim, before it empties the pool)
  SmallIdle& si = small_idle_of(device);
  std::vector<SmallCtx*> drop;
  { std::lock_guard<std::mutex> g(si.mu); drop.swap(si.v); }
  for (SmallCtx* c : drop) small_ctx_destroy(c);
}

static std::atomic<uint64_t> g_small_taken{0}, g_small_overflow{0};
void small_stats(uint64_t* out) { out[0] = g_small_taken.load(); out[1] = g_small_overflow.load(); }
static std::atomic<uint64_t> g_small_conf_taken{0}, g_small_conf_scripts{0}, g_small_conf_unweightable{0};
// include/anx.h: calls answered with device confusables, edit scripts run on them, calls discarded for a row the device cannot weight
extern "C" int anx_debug_small_conf_stats(uint64_t* out) {
  if (!out) return ANX_EINVAL;
  out[0] = g_small_conf_taken.load(); out[1] = g_small_conf_scripts.load(); out[2] = g_small_conf_unweightable.load();
  return ANX_OK;
}

// 0: done (*out_rows: a block of the pinned result cache, *out_offs: malloc'd); 1: not taken (the caller uses the batch path);
// negative: an error of the device
int small_find(const HostModel& m, const DeviceLexicon* dl, const char* const* utf8, size_t n, const anx_params& p, anx_result** out_rows, size_t** out_offs,
               std::string& err) {
  if (!dl || n == 0 || n > SMALL_MAX || !switches().small_path || p.stop_at_exact_match || dl->nplanes > 42) return 1;
  // confusables: 0 none, 1 late (after the crop, then re-rank + cutoff), 2 early (before the crop) -- Batch::conf_mode.  `p` is the caller's
  // own parameter set; host-side weighting (ANX_CONFUSABLES=host) belongs to the batch path
  const int conf_mode = m.confusables.empty() ? 0 : m.confusables_before_pruning ? 2 : 1;
  if (conf_mode && switches().confusables_host) return 1;
  uint32_t lens[SMALL_MAX];
  uint32_t maxbytes = 0;
  for (size_t i = 0; i < n; ++i) {
    const size_t l = utf8[i] ? strlen(utf8[i]) : 0;
    if (l > SMALL_MAX_BYTES) return 1;
    lens[i] = (uint32_t)l;
    maxbytes = std::max(maxbytes, (uint32_t)l);
  }
  if (hipSetDevice(dl->device) != hipSuccess) { err = "hipSetDevice failed"; return ANX_ENODEVICE; }
  SmallCtx* c = small_ctx_acquire(dl, err);
  if (!c) { (void)hipGetLastError(); return 1; }  // (no context: the batch path still works)
  struct Release { SmallCtx* c; ~Release() { small_ctx_release(c); } } rel{c};
  hipStream_t st = c->st;
  if (conf_mode && !small_ctx_conf(c)) return 1;  // (no room for the working set: the batch path answers)
  // ---- inputs -> pinned staging -----------------------------------------------------------------------------------------------------
  uint32_t* h_off = reinterpret_cast<uint32_t*>(c->h_in + SMALL_IN_BLOB);
  {
    size_t pos = 0;
    for (size_t i = 0; i < n; ++i) {
      h_off[i] = (uint32_t)pos;
      if (lens[i]) memcpy(c->h_in + pos, utf8[i], lens[i]);
      c->h_in[pos + lens[i]] = '\0';
      pos += (size_t)lens[i] + 1;
    }
    h_off[n] = (uint32_t)pos;
    memset(c->h_in + pos, 0, 16);  // (the encoder's 16-byte window may read past the last string)
  }
  const uint32_t n32 = (uint32_t)n;
  const uint32_t qw = std::max<uint32_t>(1u, (maxbytes + 15u) / 16u);                      // symbols <= bytes
  const uint32_t d = (uint32_t)clamp_threshold(p.max_edit_distance, (int)maxbytes, kMaxEditDistance);  // >= every query's clamped d (monotone in the length)
  // ---- the caller's rows: a block of the pinned result cache the last kernel writes into -----------------------------------------
  const size_t row_cap = std::min<size_t>(c->row_cap, n * (size_t)SMALL_ROWS_PER_Q + 64);
  anx_result* rows = static_cast<anx_result*>(host_result_alloc(row_cap * sizeof(anx_result)));
  if (!rows) return 1;
  // Every exit but the successful one gives the block back; once kernels may have been enqueued (`drain`) the stream is waited for first:
  // a failed launch must not let the block and the context (rel, destroyed after this) return to their pools while a kernel enqueued
  // before it still writes to them
  struct RowsGuard {
    anx_result* rows; hipStream_t st; bool drain;
    ~RowsGuard() { if (!rows) return; if (drain) (void)hipStreamSynchronize(st); host_result_free(rows); }
  } guard{rows, st, false};
  if (!host_result_is_pinned(rows)) return 1;  // (pinning failed: the kernel could not write into it)
  SmallCtl* h_ctl = reinterpret_cast<SmallCtl*>(c->h_out);
  unsigned long long* h_off64 = reinterpret_cast<unsigned long long*>(c->h_out + 64);
  h_ctl->rows = 0xFFFFFFFEu;
  // ---- encode + tiles (+ the counters cleared) ----------------------------------------------------------------------------------------
  SmallZero z{};
  {
    uint32_t* zp[8] = {c->counters, c->rctr, c->sctr, c->lctr, c->qsurv, c->qmaxfreq, c->qexpand, conf_mode ? c->cf.ctr : nullptr};
    const uint32_t zn[8] = {CTR_N, SCAN_REGIONS * RC_STRIDE, SCAN_REGIONS * RC_STRIDE, 3 * SCAN_REGIONS * RC_STRIDE, n32, n32, n32, conf_mode ? 8u : 0u};
    for (int i = 0; i < 8; ++i) { z.p[i] = zp[i]; z.n[i] = zn[i]; }
  }
  // the encoder kernels read the pinned staging buffer themselves (k_enc_strings<true>: a coalesced burst per block into LDS): a copy
  // command ahead of the first kernel cost 15-18 us of the call (round 6 traces)
  const uint8_t* in_blob = reinterpret_cast<const uint8_t*>(c->h_in);
  const uint32_t* in_off = h_off;
  // tile slots per query: 8 at 4096 inputs, up to 32 for the smallest calls (the rows of a query's adjacency list are shared out over them)
  // (a list of R rows is cut into min(slots, R / 8) parts: 2-3 for the typical list; every unused slot is still a wave that starts and
  // returns: 1 000 inputs 164 -> 156 us with 8 instead of 32 slots per query)
  const uint32_t slots = n32 <= 128u ? 32u : n32 <= 512u ? 16u : 8u;
  guard.drain = true;
  SmallEnc enc = c->enc;
  if (!conf_mode) enc.text = nullptr, enc.textoff = nullptr;  // (a plain model's call on a context that has served confusables: nothing to keep)
  int rc = small_encode_launch(m, dl, enc, in_blob, in_off, n32, qw, p, z, slots, true, h_off, st, err);
  if (rc) return rc;
  // ---- scan -----------------------------------------------------------------------------------------------------------------------------
  const uint32_t region_cap = 1u << SMALL_SHIFT;
  {
    ScanStage S{};
    S.tiles = c->enc.tiles; S.ntiles = slots * n32; S.q_bits = c->enc.q_bits; S.q_cv = c->enc.q_cv;
    S.chunk = SMALL_CHUNK; S.chunk_fused = SMALL_CHUNK_FUSED; S.chunk_first = SMALL_CHUNK_FIRST;  // flat reservations (launch_plan.hpp)
    S.raw = c->raw; S.region_cap = region_cap; S.rctr = c->rctr; S.qexact = c->enc.qexact; S.want_exact = 0; S.drop_len = 1;
    S.q_rec = c->enc.q_rec;
    S.fuse = (switches().fuse_prefilter && switches().prefilter) ? 1 : 0;  // (the batch path: only with drop_len, which is always 1 here)
    S.twins = switches().scan_twins;
    S.qpairs = nullptr; S.dbg = 0;
    launch_scan_small(dl, S, st);
  }
  // ---- score: the plan of the batch path (launch_plan.hpp) at fixed capacities ------------------------------------------------------------
  ScorePlan plan = score_plan_of(m, dl, p.score_threshold, qw, d);
  plan.sa.dbg = 0; plan.sa.store_pairs = 0;
  if (!plan.fits()) return 1;  // per-lane scoring state beyond the LDS budget: the batch path reports it (ANX_ELIMIT)
  const ScoreArgs& sa = plan.sa;
  const uint32_t threads = plan.threads;
  const int fastD = plan.fastD;
  const SurvOut so{c->surv, c->sctr, SMALL_SURV_CAP, nullptr, 0u};
  const SlotLists sl = slot_lists_of(c->list8, c->listg, c->listw, c->lctr, SMALL_SURV_CAP);  // (fixed buffers: always present)
  const PairArgs pa = pair_args_of(dl, c->raw, c->enc.q_meta, c->enc.q_rows, c->enc.q_rec, nullptr, nullptr, c->qmaxfreq, c->qsurv, c->qexpand);
  // slots per region the scoring grid covers: the whole region from a few hundred inputs on, less for the smallest calls (a region filled
  // beyond it hands the call to the batch path, like every other capacity)
  uint32_t fs_cap = 2048;
  while (fs_cap < region_cap && fs_cap < n32 * 12u + 2048u) fs_cap *= 2u;
  FilterArgs fa;
  fa.region_shift = SMALL_SHIFT; fa.rctr = c->rctr; fa.qexact = c->enc.qexact; fa.stop = 0; fa.enable = plan.enable_filter;
  // pairs with a string of 17..32 symbols go to the 8-word register DL also when no QUERY is that long (the batch path leaves a short-query
  // batch's few long candidates to the general LDS kernel: there its extra launch costs more than it saves; here both run inside k_small_lists and
  // one round of the general kernel is 25 us of a 170 us call)
  const bool use8 = fastD > 0 && threads == 256;
  fa.use_nw8 = (plan.have_long_q || use8) ? 1 : 0; fa.counters = c->counters; fa.stat_ctr = c->sctr; fa.fill_cap = fs_cap; fa.blk = SMALL_FS_BLK;
  {
    // k_filter_score's rarely used arguments live in device memory (FsCold): uploaded again only when they change (another model,
    // other weights / thresholds / row width) -- compared field by field (struct padding is not).  any_variants is part of the key: a
    // model with variant lists and one without share the context pool of a device.  (The batch path uploads its pinned copy with every run.)
    // Nothing of FsCold depends on the confusable mode or the cutoff (both reach k_rank / k_conf_apply_late as launch arguments).
    // sa.quot is the one lexicon-side pointer in FsCold, so the WHOLE pointer is in the key (low and high half: each exact in a double): the
    // replicas of a multi-device model that live on one device share this pool, their tables can lie a multiple of 4 GB apart, and a context
    // that last served one replica must not hand the other a pointer into a lexicon its owner may free
    const double key[13] = {sa.w_ld, sa.w_lcs, sa.w_prefix, sa.w_suffix, sa.w_case, sa.w_sum, sa.score_threshold, (double)sa.have_freq + 2.0 * (double)sa.any_variants, (double)sa.lqp, (double)sa.lcp, (double)sa.stride,
                            (double)sa.qw + 1e3 * (double)(reinterpret_cast<uintptr_t>(sa.quot) & 0xFFFFFFFFu), (double)((uint64_t)reinterpret_cast<uintptr_t>(sa.quot) >> 32)};
    if (!c->cold_valid || memcmp(key, c->cold_key, sizeof key) != 0) {
      memcpy(c->cold_key, key, sizeof key);
      c->h_cold_last = FsCold{sa, so, sl.l8, sl.lg, sl.lw};
      if (hipMemcpyAsync(c->d_cold, &c->h_cold_last, sizeof(FsCold), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        err = "small path: argument upload";
        return ANX_ENODEVICE;
      }
      c->cold_valid = true;
    }
  }
  launch_filter_score(plan, dim3(((fs_cap + SMALL_FS_BLK - 1) / SMALL_FS_BLK) * SCAN_REGIONS), st, fa, pa, static_cast<const FsCold*>(c->d_cold));
  const int do_wide = (plan.split_wide && plan.enable_filter) ? 1 : 0;
  if (threads == 256) {  // the slot-list kernels as one launch, a block per region (k_small_lists): k_score_fast8's part also for the long candidates of short queries
    launch_small_lists_of(plan, st, sl, fa, pa, so);  // (use8 == fastD > 0 here: k_score_fast8's part runs whenever the inline DL does)
  } else {  // the per-lane state of k_score_pairs does not fit 256 lanes: the three kernels one by one, SMALL_LIST_BLOCKS blocks per region
    const dim3 lgrid(SMALL_LIST_BLOCKS * SCAN_REGIONS);
    if (do_wide) hipLaunchKernelGGL(k_filter_wide, lgrid, dim3(256), 0, st, sl.lw, fa, pa, sa, fastD, sl.l8, sl.lg);
    if (fastD && plan.have_long_q) launch_score_fast8(fastD, lgrid, st, sl.l8, pa, sa, so);  // (use_nw8 follows have_long_q alone here; the batch path: whenever fastD)
    hipLaunchKernelGGL(k_score_pairs, lgrid, dim3(threads), plan.lds_bytes(), st, sl.lg, pa, sa, so);
  }
  // ---- compact + rank + the rows into the caller's block ---------------------------------------------------------------------------------
  // late confusables: k_rank crops without the cutoff, k_conf_apply_late re-ranks and cuts off afterwards (Run::compact_rank)
  const RankArgs ra = rank_args_of(m, dl, p, conf_mode == 1 ? 0.0 : p.cutoff_threshold);
  const uint32_t crow_cap = (uint32_t)c->row_cap;
  hipLaunchKernelGGL(k_small_offsets, dim3(1), dim3(SMALL_T), 0, st, c->qsurv, n32, c->soff, c->qcur);
  if (dl->any_variants)  // variant lists: a survivor expands to a row per VariantOf reference (+ itself), within the same fixed capacity
    hipLaunchKernelGGL(k_compact_expand, dim3(EXPAND_P * SCAN_REGIONS), dim3(EXPAND_B), 0, st, c->surv, c->sctr, SMALL_SURV_CAP, m.have_freq ? 1 : 0, c->qcur, dl->ent_rec,
                       dl->ent_var_off, dl->var_target, dl->var_target_freq, dl->var_score, c->c_rows, c->soff + n32, crow_cap, c->counters + CTR_OVERFLOW);
  else
    hipLaunchKernelGGL(k_compact_grouped, dim3(SCAN_REGIONS), dim3(COMPACT_B), 0, st, c->surv, c->sctr, SMALL_SURV_CAP, m.have_freq ? 1 : 0, c->qcur, dl->ent_rec, c->c_rows,
                       c->soff + n32, crow_cap, c->counters + CTR_OVERFLOW);
  const SmallConfRun cr{n32, crow_cap, conf_mode == 2, c->soff, c->r_count, c->counters + CTR_OVERFLOW, c->enc.q_orig, c->enc.text, c->enc.textoff, c->c_rows, c->r_rows,
                        p.cutoff_threshold, p.freq_weight};
  if (conf_mode == 2 && (rc = conf_launch_small(m, dl, st, c->cf, cr, c->r_count, err))) return rc;
  launch_rank(ra, st, n32, c->soff, c->c_rows, c->qmaxfreq, c->qexpand, c->t_key, c->r_rows, c->r_count, crow_cap, c->counters + CTR_OVERFLOW, SegRows{nullptr, 0u, nullptr});
  if (conf_mode == 1 && (rc = conf_launch_small(m, dl, st, c->cf, cr, c->r_count, err))) return rc;
  hipLaunchKernelGGL(k_small_fetch, dim3(n32 > 256u ? SMALL_FETCH_BLOCKS : 1u), dim3(SMALL_T), 0, st, n32, c->soff, c->r_count, c->r_rows, c->rctr, c->sctr, c->lctr, c->counters,
                     conf_mode ? c->cf.ctr : nullptr, h_off64, rows, (uint32_t)row_cap, crow_cap, h_ctl);
  // one check for the whole chain (the batch path: HIP_TRY per call)
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    err = std::string("small path: ") + hipGetErrorString(hipGetLastError());
    return ANX_ENODEVICE;
  }
  guard.drain = false;  // (nothing in flight any more)
  // ---- did the run fit the fixed capacities? -----------------------------------------------------------------------------------------------
  const SmallCtl ctl = *h_ctl;
  // (conf_unweightable: a row beyond conf.hip's fixed working memory -- the batch path repeats such a batch with the host-side weighting;
  // the list of rows to weight has a slot per candidate row, so conf_scripts > crow_cap cannot happen while total_surv fits)
  if (ctl.rows > row_cap || ctl.maxfill > fs_cap || ctl.surv_fill > SMALL_SURV_CAP || ctl.list_fill > SMALL_SURV_CAP || ctl.total_surv > crow_cap || ctl.overflow ||
      ctl.conf_unweightable || ctl.conf_scripts > crow_cap) {
    g_small_overflow.fetch_add(1, std::memory_order_relaxed);
    if (ctl.conf_unweightable) g_small_conf_unweightable.fetch_add(1, std::memory_order_relaxed);
    return 1;  // the batch path sizes its buffers from what it measures
  }
  size_t* offs = static_cast<size_t*>(malloc((n + 1) * sizeof(size_t)));
  if (!offs) { err = "out of memory"; return ANX_EINVAL; }
  static_assert(sizeof(size_t) == sizeof(unsigned long long), "offsets are copied as they are");
  memcpy(offs, h_off64, (n + 1) * sizeof(size_t));
  guard.rows = nullptr;  // the caller's now
  *out_rows = rows;
  *out_offs = offs;
  g_small_taken.fetch_add(1, std::memory_order_relaxed);
  if (conf_mode) {
    g_small_conf_taken.fetch_add(1, std::memory_order_relaxed);
    g_small_conf_scripts.fetch_add(ctl.conf_scripts, std::memory_order_relaxed);
  }
  return ANX_OK;
}
