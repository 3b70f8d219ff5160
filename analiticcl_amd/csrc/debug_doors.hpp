// debug_doors.hpp -- the test doors of the pipeline: the band-match bound, the prefix sum, k_rank and the scoring and scan stages alone.
// Part of the translation unit engine.hip (included inside namespace anx, after small_path.hpp): the doors launch through the
// file-static stage launchers of a run and borrow the small call's contexts; gfx950 only.
#pragma once
// ---- test hook: the band-match bound alone (anx_debug_band_bound; tests/test_gpu_switches.py) ------------------------------------
// One lane per pair, rows as the kernels see them (first 16 symbols, query padded with 0xFE, candidate with 0xFF); the three forms
// in use: 0 the scan's fused filter (B7 masks, wave-uniform d, words by the wave's longest string), 1 k_filter_score's (B7, per-lane
// d), 2 the general zero test (alphabets above 124 classes).  out[i] = 1: the bound says damerau_levenshtein(q, c) > d.
__global__ __launch_bounds__(64) void k_debug_band_bound(const uint4* __restrict__ q, const uint4* __restrict__ c, const uint8_t* __restrict__ lqs,
                                                         const uint8_t* __restrict__ lcs, uint32_t n, int d, int form, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  const bool act = i < n;
  const uint4 Q = act ? q[i] : make_uint4(0xFEFEFEFEu, 0xFEFEFEFEu, 0xFEFEFEFEu, 0xFEFEFEFEu);
  const uint4 C = act ? c[i] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
  const int lq = act ? lqs[i] : 1, lc = act ? lcs[i] : 1;
  const int ml = lq > lc ? lq : lc;
  bool rej;
  if (form == 2) {
    constexpr uint32_t M = 0xFFFFFFFFu;
    if (__any(act && ml > 12)) { const uint32_t q4[4] = {Q.x, Q.y, Q.z, Q.w}, c6[6] = {M, C.x, C.y, C.z, C.w, M}; rej = band_bound_rejects<4, false>(q4, c6, act, d, lq, lc); }
    else if (__any(act && ml > 8)) { const uint32_t q3[3] = {Q.x, Q.y, Q.z}, c5[5] = {M, C.x, C.y, C.z, M}; rej = band_bound_rejects<3, false>(q3, c5, act, d, lq, lc); }
    else { const uint32_t q2[2] = {Q.x, Q.y}, c4[4] = {M, C.x, C.y, M}; rej = band_bound_rejects<2, false>(q2, c4, act, d, lq, lc); }
  } else {
    constexpr uint32_t M = 0x7F7F7F7Fu;
    const uint32_t q4[4] = {Q.x & M, Q.y & M, Q.z & M, Q.w & M}, c6[6] = {M, C.x & M, C.y & M, C.z & M, C.w & M, M};
    const uint32_t q3[3] = {q4[0], q4[1], q4[2]}, c5[5] = {M, c6[1], c6[2], c6[3], M};
    const uint32_t q2[2] = {q4[0], q4[1]}, c4[4] = {M, c6[1], c6[2], M};
    if (form == 0) {
      if (__any(act && ml > 12)) rej = band_bound_rejects<4, true, true>(q4, c6, act, d, lq, lc);
      else if (__any(act && ml > 8)) rej = band_bound_rejects<3, true, true>(q3, c5, act, d, lq, lc);
      else rej = band_bound_rejects<2, true, true>(q2, c4, act, d, lq, lc);
    } else {
      if (__any(act && ml > 12)) rej = band_bound_rejects<4, true>(q4, c6, act, d, lq, lc);
      else if (__any(act && ml > 8)) rej = band_bound_rejects<3, true>(q3, c5, act, d, lq, lc);
      else rej = band_bound_rejects<2, true>(q2, c4, act, d, lq, lc);
    }
  }
  if (act) out[i] = rej ? 1 : 0;
}
int debug_band_bound(int device, const uint8_t* q_rows, const uint8_t* c_rows, const uint8_t* lq, const uint8_t* lc, size_t n, int d, int form,
                     uint8_t* out, std::string& err) {
  if (n == 0) return ANX_OK;
  if (n > (1u << 30) || d < 0 || d > 3 || form < 0 || form > 2) { err = "band bound: bad arguments"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(device));
  uint4 *dq = nullptr, *dc = nullptr;
  uint8_t *dlq = nullptr, *dlc = nullptr, *dout = nullptr;
  int rc = ANX_OK;
  auto cleanup = [&]() { for (void* p : {(void*)dq, (void*)dc, (void*)dlq, (void*)dlc, (void*)dout}) if (p) (void)hipFree(p); };
  auto fail_hip = [&](hipError_t e) { err = std::string("HIP: ") + hipGetErrorString(e); cleanup(); return ANX_ENODEVICE; };
  hipError_t e;
  if ((e = hipMalloc(reinterpret_cast<void**>(&dq), n * 16)) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&dc), n * 16)) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&dlq), n)) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&dlc), n)) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&dout), n)) != hipSuccess)
    return fail_hip(e);
  if ((e = hipMemcpy(dq, q_rows, n * 16, hipMemcpyHostToDevice)) != hipSuccess || (e = hipMemcpy(dc, c_rows, n * 16, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(dlq, lq, n, hipMemcpyHostToDevice)) != hipSuccess || (e = hipMemcpy(dlc, lc, n, hipMemcpyHostToDevice)) != hipSuccess)
    return fail_hip(e);
  hipLaunchKernelGGL(k_debug_band_bound, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, 0, dq, dc, dlq, dlc, (uint32_t)n, d, form, dout);
  if ((e = hipDeviceSynchronize()) != hipSuccess || (e = hipMemcpy(out, dout, n, hipMemcpyDeviceToHost)) != hipSuccess) return fail_hip(e);
  cleanup();
  return rc;
}

// ---- test hook: the run's prefix sum alone (anx_debug_exclusive_scan; tests/test_gpu_prefix_sum.py) -----------------------------------
// out[0 .. n] = the exclusive prefix sum of in[0 .. n) as exclusive_scan computes it on the device (out[n] = the total), copy (may be
// nullptr) = out[0 .. n) through the kernel's second output.
int debug_exclusive_scan(int device, const uint32_t* in, size_t n, uint32_t* out, uint32_t* copy, std::string& err) {
  if (n >= ((size_t)1 << 31)) { err = "prefix sum: more than 2^31 elements"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(device));
  uint32_t *din = nullptr, *dout = nullptr, *dcopy = nullptr, *dtmp = nullptr;
  auto cleanup = [&]() { for (void* p : {(void*)din, (void*)dout, (void*)dcopy, (void*)dtmp}) if (p) (void)hipFree(p); };
  auto fail_hip = [&](hipError_t e) { err = std::string("HIP: ") + hipGetErrorString(e); cleanup(); return ANX_ENODEVICE; };
  hipError_t e;
  if ((e = hipMalloc(reinterpret_cast<void**>(&din), (n + 1) * 4)) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&dout), (n + 1) * 4)) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&dcopy), (n + 1) * 4)) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&dtmp), scan_tmp_bytes(n))) != hipSuccess)
    return fail_hip(e);
  if (n && (e = hipMemcpy(din, in, n * 4, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e);
  if (exclusive_scan(din, (uint32_t)n, dout, dtmp, 0, copy ? dcopy : nullptr)) return fail_hip(hipGetLastError());
  if ((e = hipDeviceSynchronize()) != hipSuccess || (e = hipMemcpy(out, dout, (n + 1) * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
      (copy && n && (e = hipMemcpy(copy, dcopy, n * 4, hipMemcpyDeviceToHost)) != hipSuccess))
    return fail_hip(e);
  cleanup();
  return ANX_OK;
}

// ---- test hook: k_rank alone on hand-made candidate rows (anx_debug_rank_rows; tests/test_gpu_rank_rows.py) ---------------------------
// soff = the exclusive sum of counts; the rows as a run lays them out (c_rows, or segments of seg_cap records + ent_rec + surplus in
// c_rows); t_key / r_rows / r_count sized by the total whatever row_cap says, r_rows and r_count filled with 0xFF bytes; launch_rank.
int debug_rank_rows(int device, const DebugRankIn& in, uint32_t* out_count, void* out_rows, std::string& err) {
  const size_t nq = in.nq;
  if (nq == 0) return ANX_OK;
  if (nq >= ((size_t)1 << 28)) { err = "rank rows: too many queries"; return ANX_EINVAL; }
  std::vector<uint32_t> soff(nq + 1, 0u);
  uint64_t total64 = 0;
  for (size_t q = 0; q < nq; ++q) { soff[q] = (uint32_t)total64; total64 += in.counts[q]; if (total64 >= (1ull << 31)) { err = "rank rows: more than 2^31 rows"; return ANX_EINVAL; } }
  soff[nq] = (uint32_t)total64;
  const size_t total = (size_t)total64, C = in.seg_cap;
  for (size_t r = 0; r < total; ++r) {
    if (in.position[r] >= (1u << 20)) { err = "rank rows: expansion position beyond 2^20"; return ANX_EINVAL; }
    if (C && (in.position[r] != 0 || (in.via && in.via[r] != 0xFFFFFFFFu))) { err = "rank rows: segments hold rows without expansion position and via only"; return ANX_EINVAL; }
  }
  if (C && in.any_variants) { err = "rank rows: no segments with variant lists"; return ANX_EINVAL; }
  if (C && nq * C >= ((size_t)1 << 31)) { err = "rank rows: segments too large"; return ANX_EINVAL; }
  std::vector<SurvRow> rows(total ? total : 1, SurvRow{0.0, 0ull, 0u, 0u, 0xFFFFFFFFu, 0u});
  std::vector<SurvSeg> seg(nq * C + 1, SurvSeg{0.0, 0u, 0u});  // (one spare record behind the last segment)
  std::vector<EntRec> ent(C && total ? total : 1, EntRec{0u, 0u, 0u, 0u});
  for (size_t q = 0; q < nq; ++q)
    for (size_t i = 0; i < in.counts[q]; ++i) {
      const size_t e = soff[q] + i;
      if (i < C) {
        seg[q * C + i] = SurvSeg{in.score[e], (uint32_t)e, 0u};
        ent[e] = EntRec{in.vocab[e], in.freq[e], in.order[e], 0u};
      } else {
        rows[e - C] = SurvRow{in.score[e], (unsigned long long)in.order[e] << 20 | in.position[e], in.vocab[e], in.freq[e], in.via ? in.via[e] : 0xFFFFFFFFu, 0u};
      }
    }
  HIP_TRY(hipSetDevice(device));
  uint32_t *d_soff = nullptr, *d_maxf = nullptr, *d_qex = nullptr, *d_count = nullptr, *d_ovf = nullptr;
  SurvRow* d_rows = nullptr;
  SurvSeg* d_seg = nullptr;
  EntRec* d_ent = nullptr;
  double* d_tkey = nullptr;
  DevRow* d_out = nullptr;
  auto cleanup = [&]() { for (void* p : {(void*)d_soff, (void*)d_maxf, (void*)d_qex, (void*)d_count, (void*)d_ovf, (void*)d_rows, (void*)d_seg, (void*)d_ent, (void*)d_tkey, (void*)d_out}) if (p) (void)hipFree(p); };
  auto fail_hip = [&](hipError_t e) { err = std::string("HIP: ") + hipGetErrorString(e); cleanup(); return ANX_ENODEVICE; };
  const size_t out_bytes = (total ? total : 1) * sizeof(DevRow);
  hipError_t e;
  if ((e = hipMalloc(reinterpret_cast<void**>(&d_soff), (nq + 1) * 4)) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&d_maxf), nq * 4)) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&d_qex), nq * 4)) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&d_count), nq * 4)) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&d_ovf), 4)) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&d_rows), rows.size() * sizeof(SurvRow))) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&d_seg), seg.size() * sizeof(SurvSeg))) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&d_ent), ent.size() * sizeof(EntRec))) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&d_tkey), (total ? total : 1) * 8)) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&d_out), out_bytes)) != hipSuccess)
    return fail_hip(e);
  if ((e = hipMemcpy(d_soff, soff.data(), (nq + 1) * 4, hipMemcpyHostToDevice)) != hipSuccess || (e = hipMemcpy(d_maxf, in.maxfreq, nq * 4, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d_qex, in.qexpand, nq * 4, hipMemcpyHostToDevice)) != hipSuccess || (e = hipMemcpy(d_ovf, &in.overflow, 4, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d_rows, rows.data(), rows.size() * sizeof(SurvRow), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d_seg, seg.data(), seg.size() * sizeof(SurvSeg), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(d_ent, ent.data(), ent.size() * sizeof(EntRec), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemset(d_tkey, 0, (total ? total : 1) * 8)) != hipSuccess || (e = hipMemset(d_count, 0xFF, nq * 4)) != hipSuccess || (e = hipMemset(d_out, 0xFF, out_bytes)) != hipSuccess)
    return fail_hip(e);
  RankArgs ra{};
  ra.cutoff_threshold = in.cutoff_threshold;
  ra.max_matches = in.max_matches;
  ra.freq_weight = in.freq_weight;
  ra.have_freq = in.have_freq;
  ra.any_variants = in.any_variants;
  launch_rank(ra, 0, (uint32_t)nq, d_soff, d_rows, d_maxf, d_qex, d_tkey, d_out, d_count, in.row_cap, d_ovf, C ? SegRows{d_seg, (uint32_t)C, d_ent} : SegRows{nullptr, 0u, nullptr});
  if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess || (e = hipMemcpy(out_count, d_count, nq * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
      (total && (e = hipMemcpy(out_rows, d_out, total * sizeof(DevRow), hipMemcpyDeviceToHost)) != hipSuccess))
    return fail_hip(e);
  cleanup();
  return ANX_OK;
}

// ---- test hook: the scoring stage alone on a pair list the caller laid out (anx_debug_score_slots; tests/test_gpu_score_slots.py) ------
// The band-match bound (kernels_swar.hpp band_bound_rejects) on the host: positions of either string without an equal symbol of the other
// one within +-d positions; more than d of them on a side rejects the pair.
static bool host_band_bound_rejects(const uint8_t* q, int lq, const uint8_t* c, int lc, int d) {
  int unA = 0, unB = 0;
  for (int i = 0; i < lq; ++i) {
    bool hit = false;
    for (int j = std::max(0, i - d); j <= std::min(lc - 1, i + d); ++j) hit = hit || q[i] == c[j];
    unA += !hit;
  }
  for (int j = 0; j < lc; ++j) {
    bool hit = false;
    for (int i = std::max(0, j - d); i <= std::min(lq - 1, j + d); ++i) hit = hit || q[i] == c[j];
    unB += !hit;
  }
  return unA > d || unB > d;
}
// Everything is checked on the host before the first launch (a wrong test input is refused, never gathered from); the device buffers of
// the stage are the hook's own (the batch keeps its pair list and results), filled with 0xFF bytes, and launched through
// score_stage_launch like a run's.
int debug_score_slots(const HostModel& m, const DeviceLexicon* dl, const Batch* b, const DebugScoreIn& in, const DebugScoreOut& out, std::string& err) {
  if (!dl || !b) { err = "score slots: the model is not resident on a device"; return ANX_ENODEVICE; }
  const size_t nq = b->nq, n_input = b->n_input, C = in.seg_cap;
  const uint32_t region_cap = 1u << (in.region_shift & 31u);
  auto refuse = [&](const std::string& msg) { err = "score slots: " + msg; return ANX_EINVAL; };
  if (in.region_shift < 10 || in.region_shift > 16) return refuse("region_shift outside 10 .. 16");
  if (in.surv_region_cap == 0 || in.list_cap == 0) return refuse("a capacity of 0");
  if (in.surv_region_cap > (1u << 16) || in.list_cap > (1u << 16)) return refuse("a capacity beyond 65536 per region");
  if (in.blk == 0 || in.blk % 256 != 0 || in.blk > FS_BLK) return refuse("blk is no multiple of 256 up to " + std::to_string(FS_BLK));
  if (nq == 0 || nq >= ((size_t)1 << 20)) return refuse("the batch holds no query (or more than 2^20)");
  if (C && (C > 1024 || seg_wanted(b) == 0 || dl->any_variants)) return refuse("no per-query segments for this model and batch (variant lists, StopAtExactMatch, freq_weight, switch)");
  for (uint32_t r = 0; r < SCAN_REGIONS; ++r)
    if (in.fills[r] > region_cap) return refuse("fill of region " + std::to_string(r) + " beyond the region");
  HIP_TRY(hipSetDevice(dl->device));
  { const int rc = ensure_order(b, err); if (rc) return rc; }
  const int stop = b->params.stop_at_exact_match ? 1 : 0;
  ScorePlan plan;
  { const int rc = score_stage_plan(m, dl, b->params.score_threshold, b->qw, b->dmax, true, plan, err); if (rc) return rc; }
  if (in.one_launch && plan.threads != 256) return refuse("the one-launch list kernels take 256 threads: the per-lane state of this model and batch allows " + std::to_string(plan.threads));
  // what the checks read: the queries' and entries' records (first 16 symbols, meta)
  std::vector<uint32_t> pos_of(n_input, 0xFFFFFFFFu);
  for (size_t q = 0; q < nq; ++q) if (b->order[q] < n_input) pos_of[b->order[q]] = (uint32_t)q;
  std::vector<uint4> qrec(2 * nq), erec(2 * (size_t)dl->nentries + 2);
  HIP_TRY(hipMemcpy(qrec.data(), b->q_rec, 2 * nq * sizeof(uint4), hipMemcpyDeviceToHost));
  if (dl->nentries) HIP_TRY(hipMemcpy(erec.data(), dl->e_rec, 2 * (size_t)dl->nentries * sizeof(uint4), hipMemcpyDeviceToHost));
  const bool bit_planes = dl->nsym <= 32 && !switches().scan_sad;
  std::vector<uint2> raw((size_t)SCAN_REGIONS << in.region_shift, make_uint2(RAW_INVALID, 0xFFFFFFFFu));
  {
    size_t i = 0;
    for (uint32_t r = 0; r < SCAN_REGIONS; ++r)
      for (uint32_t k = 0; k < in.fills[r]; ++k, ++i) {
        const uint32_t qi = in.slots[2 * i], ew = in.slots[2 * i + 1];
        if (qi == RAW_INVALID) continue;
        const std::string at = " (slot " + std::to_string(k) + " of region " + std::to_string(r) + ")";
        if (qi >= n_input || pos_of[qi] == 0xFFFFFFFFu) return refuse("query index out of range or not encoded" + at);
        // the entry id as the GENERAL round reads it (30 bits): a flagged slot of a mixed wave is gathered there, not under the short round's 26-bit mask
        const uint32_t q = pos_of[qi], e = ew & RAW_ENTRY_MASK;
        if (e >= dl->nentries) return refuse("entry id out of range" + at);
        if ((ew & 0x80000000u) && !stop) return refuse("bit 31 (exact class) outside a StopAtExactMatch batch" + at);
        if (ew & RAW_PREFILTERED) {  // the scan's contract (kernels_scan.hpp, the fused prefilter of emit_dense)
          const uint32_t qm = qrec[2 * (size_t)q + 1].x, em = erec[2 * (size_t)e + 1].x;
          const int lq = qm & 0xFF, d = (qm >> 16) & 0xFF, lc = em & 0xFF;
          if (!bit_planes || stop || (ew & 0x80000000u)) return refuse("RAW_PREFILTERED outside a bit-plane model or in a StopAtExactMatch batch" + at);
          if (e >= (1u << 26)) return refuse("RAW_PREFILTERED with an entry id beyond 2^26" + at);
          if (lq > 16 || lc > 16 || d > 3 || std::abs(lq - lc) > d) return refuse("RAW_PREFILTERED on a pair the scan does not filter (lengths, d)" + at);
          if (host_band_bound_rejects(reinterpret_cast<const uint8_t*>(&qrec[2 * (size_t)q]), lq, reinterpret_cast<const uint8_t*>(&erec[2 * (size_t)e]), lc, d))
            return refuse("RAW_PREFILTERED on a pair the band-match bound rejects" + at);
        }
        raw[((size_t)r << in.region_shift) + k] = make_uint2(q, ew);
      }
  }
  // ---- device buffers of the stage ------------------------------------------------------------------------------------------------------
  const size_t R = raw.size(), nsurv = (size_t)SCAN_REGIONS * in.surv_region_cap, nlist = (size_t)SCAN_REGIONS * in.list_cap;
  uint2* d_raw = nullptr;
  double* d_pscore = nullptr;
  uint32_t *d_pmeta = nullptr, *d_ctl = nullptr, *d_q3 = nullptr, *d_lists = nullptr;
  SurvRec* d_surv = nullptr;
  SurvSeg* d_seg = nullptr;
  void* d_cold = nullptr;
  FsCold* h_cold = nullptr;
  auto cleanup = [&]() {
    for (void* p : {(void*)d_raw, (void*)d_pscore, (void*)d_pmeta, (void*)d_ctl, (void*)d_q3, (void*)d_lists, (void*)d_surv, (void*)d_seg, d_cold}) if (p) (void)hipFree(p);
    if (h_cold) (void)hipHostFree(h_cold);
  };
  auto fail_hip = [&](hipError_t e) { err = std::string("HIP: ") + hipGetErrorString(e); cleanup(); return ANX_ENODEVICE; };
  hipError_t e;
  if ((e = hipMalloc(reinterpret_cast<void**>(&d_raw), R * sizeof(uint2))) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&d_pscore), R * 8)) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&d_pmeta), R * 4)) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&d_ctl), HR_N * 4)) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&d_q3), 3 * nq * 4)) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&d_lists), 3 * nlist * 4)) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&d_surv), nsurv * sizeof(SurvRec))) != hipSuccess || (e = hipMalloc(reinterpret_cast<void**>(&d_seg), (nq * C + 1) * sizeof(SurvSeg))) != hipSuccess ||
      (e = hipMalloc(&d_cold, sizeof(FsCold))) != hipSuccess || (e = hipHostMalloc(reinterpret_cast<void**>(&h_cold), sizeof(FsCold), hipHostMallocDefault)) != hipSuccess)
    return fail_hip(e);
  std::vector<uint32_t> ctl(HR_N, 0u);
  for (uint32_t r = 0; r < SCAN_REGIONS; ++r) ctl[HR_RCTR + r * RC_STRIDE + RC_RAW] = in.fills[r];
  if ((e = hipMemcpy(d_raw, raw.data(), R * sizeof(uint2), hipMemcpyHostToDevice)) != hipSuccess || (e = hipMemcpy(d_ctl, ctl.data(), HR_N * 4, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemset(d_pscore, 0xFF, R * 8)) != hipSuccess || (e = hipMemset(d_pmeta, 0xFF, R * 4)) != hipSuccess || (e = hipMemset(d_q3, 0xFF, 3 * nq * 4)) != hipSuccess ||
      (e = hipMemset(d_lists, 0xFF, 3 * nlist * 4)) != hipSuccess || (e = hipMemset(d_surv, 0xFF, nsurv * sizeof(SurvRec))) != hipSuccess ||
      (e = hipMemset(d_seg, 0xFF, (nq * C + 1) * sizeof(SurvSeg))) != hipSuccess)
    return fail_hip(e);
  ScoreStage S{};
  S.nq = (uint32_t)nq; S.stop = stop; S.region_shift = in.region_shift; S.fill_cap = region_cap; S.blk = in.blk; S.one_launch = in.one_launch != 0;
  S.raw = d_raw; S.q_meta = b->q_meta; S.q_rows = b->q_rows; S.q_rec = b->q_rec; S.qexact = b->qexact; S.p_score = d_pscore; S.p_meta = d_pmeta;
  S.qsurv = d_q3; S.rctr = d_ctl + HR_RCTR; S.sctr = d_ctl + HR_SCTR; S.lctr = d_ctl + HR_LCTR; S.counters = d_ctl + HR_CTR;
  S.so = SurvOut{d_surv, d_ctl + HR_SCTR, in.surv_region_cap, C ? d_seg : nullptr, (uint32_t)C};
  S.need_lists = score_stage_needs_lists(plan, dl); S.list8 = d_lists; S.listg = d_lists + nlist; S.listw = d_lists + 2 * nlist; S.list_cap = in.list_cap;
  S.h_cold = h_cold; S.d_cold = d_cold; S.ev_fs0 = nullptr; S.ev_fs1 = nullptr;
  { const int rc = score_stage_launch(dl, plan, S, 0, err); if (rc) { cleanup(); return rc; } }
  // ---- everything back, in the caller's terms (input indices, slots in the caller's order) ---------------------------------------------
  std::vector<uint32_t> pmeta(R), q3(3 * nq);
  std::vector<double> pscore(R);
  std::vector<SurvRec> surv(nsurv);
  std::vector<SurvSeg> seg(nq * C + 1);
  if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess || (e = hipMemcpy(pmeta.data(), d_pmeta, R * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(pscore.data(), d_pscore, R * 8, hipMemcpyDeviceToHost)) != hipSuccess || (e = hipMemcpy(q3.data(), d_q3, 3 * nq * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(ctl.data(), d_ctl, HR_N * 4, hipMemcpyDeviceToHost)) != hipSuccess || (e = hipMemcpy(surv.data(), d_surv, nsurv * sizeof(SurvRec), hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(seg.data(), d_seg, (nq * C + 1) * sizeof(SurvSeg), hipMemcpyDeviceToHost)) != hipSuccess)
    return fail_hip(e);
  cleanup();
  {
    size_t i = 0;
    for (uint32_t r = 0; r < SCAN_REGIONS; ++r)
      for (uint32_t k = 0; k < in.fills[r]; ++k, ++i) {
        out.meta[i] = pmeta[((size_t)r << in.region_shift) + k];
        out.score[i] = pscore[((size_t)r << in.region_shift) + k];
      }
  }
  for (size_t q = 0; q < nq; ++q) {
    const uint32_t qi = b->order[q];
    if (qi >= n_input) continue;
    for (int k = 0; k < 3; ++k) out.qcount[k * n_input + qi] = q3[k * nq + q];
    if (C) memcpy(static_cast<char*>(out.seg) + (size_t)qi * C * sizeof(SurvSeg), &seg[q * C], C * sizeof(SurvSeg));
  }
  for (uint32_t r = 0; r < SCAN_REGIONS; ++r) {
    const uint32_t fill = ctl[HR_SCTR + r * RC_STRIDE];
    for (uint32_t k = 0; k < std::min(fill, in.surv_region_cap); ++k) {  // (written records: the query as its input index)
      SurvRec& s = surv[(size_t)r * in.surv_region_cap + k];
      if (s.q < nq) s.q = b->order[s.q];
    }
    out.ctr[0 * SCAN_REGIONS + r] = fill;
    for (uint32_t l = 0; l < 3; ++l) out.ctr[(1 + l) * SCAN_REGIONS + r] = ctl[HR_LCTR + (l * SCAN_REGIONS + r) * RC_STRIDE];
    out.ctr[4 * SCAN_REGIONS + r] = ctl[HR_SCTR + r * RC_STRIDE + 1];
  }
  memcpy(out.surv, surv.data(), nsurv * sizeof(SurvRec));
  *out.skipped = ctl[HR_CTR + CTR_SKIPPED];
  return ANX_OK;
}

// ---- test hook: the scan stage alone (anx_debug_scan_pairs; tests/test_gpu_scan_door.py) ------------------------------------------------
// The tiles are the encoder's own, never the caller's: the batch's (batch form) or those small_encode_launch lays on a borrowed context of the
// small path (small form, as small_find borrows one).  What is plain data in ScanArgs is the caller's and validated on the host before anything
// is launched.  The pair list, its counters and the per-query counts are the hook's own buffers: the pair list (and SCAN_GUARD slots behind
// it) starts as 0xFE bytes -- neither RAW_INVALID nor a pair -- the counters as 0.  The launch is scan_stage_launch / launch_scan_small.
constexpr uint32_t SCAN_GUARD = 4096;  // slots behind the pair list that must keep the fill
int debug_scan_pairs(const HostModel& m, const DeviceLexicon* dl, const Batch* b, const DebugScanIn& in, const DebugScanOut& out, std::string& err) {
  if (!dl) { err = "scan pairs: the model is not resident on a device"; return ANX_ENODEVICE; }
  auto refuse = [&](const std::string& msg) { err = "scan pairs: " + msg; return ANX_EINVAL; };
  const bool small = b == nullptr;
  if (in.region_shift < 10 || in.region_shift > 25) return refuse("region_shift outside 10 .. 25");
  for (uint32_t c : {in.chunk, in.chunk_fused, in.chunk_first})
    if (c < 32 || c > 1024) return refuse("a chunk size outside 32 .. 1024");
  if (in.fuse && (!in.drop_len || in.want_exact)) return refuse("fuse without drop_len or with want_exact: the fused filter takes pairs that passed the length test (as a run sets it)");
  uint32_t lens[SMALL_MAX];
  uint32_t maxbytes = 0;
  if (small) {
    if (in.n == 0 || in.n > SMALL_MAX) return refuse("the small form takes 1 .. " + std::to_string(SMALL_MAX) + " strings");
    if (in.slots != 8 && in.slots != 16 && in.slots != 32) return refuse("tile slots per query are 8, 16 or 32");
    if ((size_t)in.slots * in.n > (size_t)8 * SMALL_MAX) return refuse("more tile slots than a context of the small path holds");
    if (in.want_exact || in.count_pairs || !in.drop_len) return refuse("the small call's kernel has no instance for StopAtExactMatch, per-query counts or every pair");
    if (dl->nplanes > 42) return refuse("the small path does not take this alphabet");
    for (size_t i = 0; i < in.n; ++i) {
      const size_t l = in.utf8[i] ? strlen(in.utf8[i]) : 0;
      if (l > SMALL_MAX_BYTES) return refuse("a string of more than " + std::to_string(SMALL_MAX_BYTES) + " bytes");
      lens[i] = (uint32_t)l;
      maxbytes = std::max(maxbytes, (uint32_t)l);
    }
  } else {
    if (b->nq >= ((size_t)1 << 26)) return refuse("more than 2^26 queries");
    if (in.want_exact && (!b->params.stop_at_exact_match || !b->qexact)) return refuse("want_exact with a batch that was not encoded for StopAtExactMatch");
  }
  HIP_TRY(hipSetDevice(dl->device));
  const size_t nq = small ? in.n : b->nq;
  const uint32_t ntiles = small ? in.slots * (uint32_t)in.n : b->ntiles;
  const size_t R = (size_t)SCAN_REGIONS << in.region_shift;
  uint2* d_raw = nullptr;
  uint32_t *d_rctr = nullptr, *d_qpairs = nullptr;
  SmallCtx* c = nullptr;
  auto cleanup = [&]() {
    for (void* p : {(void*)d_raw, (void*)d_rctr, (void*)d_qpairs}) if (p) (void)hipFree(p);
    if (c) { (void)hipStreamSynchronize(c->st); small_ctx_release(c); }
  };
  auto fail_hip = [&](hipError_t e) { err = std::string("HIP: ") + hipGetErrorString(e); cleanup(); return ANX_ENODEVICE; };
  hipError_t e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return fail_hip(e);  // (the encoder's streams: the tiles and query arrays are complete)
  if ((e = hipMalloc(reinterpret_cast<void**>(&d_raw), (R + SCAN_GUARD) * sizeof(uint2))) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&d_rctr), SCAN_REGIONS * RC_STRIDE * 4)) != hipSuccess ||
      (e = hipMalloc(reinterpret_cast<void**>(&d_qpairs), std::max<size_t>(nq, 1) * 4)) != hipSuccess)
    return fail_hip(e);
  if ((e = hipMemset(d_raw, 0xFE, (R + SCAN_GUARD) * sizeof(uint2))) != hipSuccess || (e = hipMemset(d_rctr, 0, SCAN_REGIONS * RC_STRIDE * 4)) != hipSuccess ||
      (e = hipMemset(d_qpairs, 0, std::max<size_t>(nq, 1) * 4)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)
    return fail_hip(e);
  ScanStage S{};
  S.ntiles = ntiles;
  S.raw = d_raw; S.region_cap = 1u << in.region_shift; S.rctr = d_rctr;
  S.chunk = in.chunk; S.chunk_fused = in.chunk_fused; S.chunk_first = in.chunk_first;
  S.want_exact = in.want_exact ? 1 : 0; S.drop_len = in.drop_len ? 1 : 0; S.fuse = in.fuse ? 1 : 0; S.twins = in.twins ? 1 : 0;
  S.qpairs = in.count_pairs ? d_qpairs : nullptr; S.dbg = 0;
  const Tile* d_tiles = nullptr;
  const uint32_t *d_qorig = nullptr, *d_qmeta = nullptr;
  uint32_t nadj = 0, nsad = 0;
  if (small) {
    c = small_ctx_acquire(dl, err);
    if (!c) { (void)hipGetLastError(); cleanup(); return ANX_ENODEVICE; }
    uint32_t* h_off = reinterpret_cast<uint32_t*>(c->h_in + SMALL_IN_BLOB);
    size_t pos = 0;
    for (size_t i = 0; i < in.n; ++i) {  // the inputs -> pinned staging, as small_find packs them
      h_off[i] = (uint32_t)pos;
      if (lens[i]) memcpy(c->h_in + pos, in.utf8[i], lens[i]);
      c->h_in[pos + lens[i]] = '\0';
      pos += (size_t)lens[i] + 1;
    }
    h_off[in.n] = (uint32_t)pos;
    memset(c->h_in + pos, 0, 16);
    const uint32_t qw = std::max<uint32_t>(1u, (maxbytes + 15u) / 16u);
    SmallEnc enc = c->enc;
    enc.text = nullptr; enc.textoff = nullptr;
    SmallZero z{};  // (the context's counters are not this call's: nothing to clear)
    const int rc = small_encode_launch(m, dl, enc, reinterpret_cast<const uint8_t*>(c->h_in), h_off, (uint32_t)in.n, qw, *in.params, z, in.slots, true, h_off, c->st, err);
    if (rc) { cleanup(); return rc; }
    S.tiles = c->enc.tiles; S.q_bits = c->enc.q_bits; S.q_cv = c->enc.q_cv; S.q_rec = c->enc.q_rec; S.qexact = c->enc.qexact;
    launch_scan_small(dl, S, c->st);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(c->st)) != hipSuccess) return fail_hip(e);
    d_tiles = c->enc.tiles; d_qorig = c->enc.q_orig; d_qmeta = c->enc.q_meta;
  } else {
    nsad = b->n_sad_tiles; nadj = std::min(b->n_adj_tiles, ntiles - nsad);
    S.tiles = b->d_tiles; S.n_adj_tiles = b->n_adj_tiles; S.n_sad_tiles = nsad; S.q_bits = b->q_bits; S.q_cv = b->q_cv; S.q_rec = b->q_rec; S.qexact = b->qexact;
    if (ntiles) scan_stage_launch(dl, S, 0, nullptr, nullptr);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) return fail_hip(e);
    d_tiles = b->d_tiles; d_qorig = b->q_orig; d_qmeta = b->q_meta;
  }
  // ---- everything back ----------------------------------------------------------------------------------------------------------------
  static_assert(sizeof(Tile) == 15 * sizeof(uint32_t), "a tile is 15 words");
  uint32_t* tiles = static_cast<uint32_t*>(malloc(std::max<size_t>(ntiles, 1) * sizeof(Tile)));
  std::vector<uint2> guard(SCAN_GUARD);
  if (!tiles) { cleanup(); err = "out of memory"; return ANX_EINVAL; }
  if ((ntiles && (e = hipMemcpy(tiles, d_tiles, (size_t)ntiles * sizeof(Tile), hipMemcpyDeviceToHost)) != hipSuccess) ||
      (nq && ((e = hipMemcpy(out.q_orig, d_qorig, nq * 4, hipMemcpyDeviceToHost)) != hipSuccess || (e = hipMemcpy(out.q_meta, d_qmeta, nq * 4, hipMemcpyDeviceToHost)) != hipSuccess ||
              (e = hipMemcpy(out.qpairs, d_qpairs, nq * 4, hipMemcpyDeviceToHost)) != hipSuccess)) ||
      (e = hipMemcpy(out.raw, d_raw, R * sizeof(uint2), hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(guard.data(), d_raw + R, SCAN_GUARD * sizeof(uint2), hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(out.rctr, d_rctr, SCAN_REGIONS * RC_STRIDE * 4, hipMemcpyDeviceToHost)) != hipSuccess) {
    free(tiles);
    return fail_hip(e);
  }
  cleanup();
  // the kind of every query as its tile tests it (kend), 0 = count vectors; UINT32_MAX = in no tile
  for (size_t q = 0; q < nq; ++q) out.q_kind[q] = 0xFFFFFFFFu;
  for (uint32_t i = 0; i < ntiles; ++i) {
    const Tile& t = reinterpret_cast<const Tile*>(tiles)[i];
    for (uint32_t j = 0; j < t.nq && (size_t)t.q0 + j < nq; ++j)
      out.q_kind[t.q0 + j] = t.kind == 0u ? 0u : j < (t.kend & 0xFFu) ? 1u : j < ((t.kend >> 8) & 0xFFu) ? 2u : j < ((t.kend >> 16) & 0xFFu) ? 3u : 4u;
  }
  uint32_t touched = 0;
  for (const uint2& g : guard) touched += (g.x != 0xFEFEFEFEu || g.y != 0xFEFEFEFEu) ? 1u : 0u;
  out.counts[0] = ntiles; out.counts[1] = nadj; out.counts[2] = small ? 0u : ntiles - nsad - nadj; out.counts[3] = nsad; out.counts[4] = (uint32_t)nq;
  out.counts[5] = touched;
  *out.tiles = tiles;
  return ANX_OK;
}
