// engine.hip -- the HIP (gfx950 / CDNA4) variant-query pipeline of the anx engine.
//
// Replaces, for a whole batch of queries at once, the reference's
//   find_nearest_anahashes  (/root/reference/src/lib.rs:1143-1308)  -> k_scan_bits / k_scan_sad       (kernels_scan.hpp)
//   gather_instances        (src/lib.rs:1311-1402, src/distance.rs)  -> k_filter_score, k_score_fast8,
//                                                                      k_score_pairs                  (kernels_score.hpp)
//   score_and_rank          (src/lib.rs:1405-1653, src/types.rs:334-365) -> the same + k_compact, k_rank (kernels_rank.hpp)
// This file: lexicon upload, batch encoding / tiling, the launch sequence of a run and its read-back, the small call
// (small_path.hpp) and the test doors (debug_doors.hpp).  The device memory pool, the streams, the shells and the kernel timer are
// runtime.hip's; the ranked rows leave the device through results.hip.  One translation unit for every kernel of a run (the kernel
// headers are included below).  Integer work only: no MFMA.  Wave = 64 lanes everywhere.  See DESIGN.md for layout and rooflines.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>

#include "engine_internal.h"
#include "scan_twins.hpp"

namespace anx {

#include "kernels_common.hpp"
#include "kernels_swar.hpp"
#include "kernels_scan.hpp"
#include "kernels_prefix.hpp"
#include "kernels_score.hpp"
#include "kernels_rank.hpp"

// ------------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------------
// layout of a run's control block on the device (Batch::ctl) and of the pinned block it is read back into (Batch::h_read), in uint32 words
enum { HR_RCTR = 0, HR_SCTR = SCAN_REGIONS * RC_STRIDE, HR_LCTR = 2 * SCAN_REGIONS * RC_STRIDE, HR_CTR = 5 * SCAN_REGIONS * RC_STRIDE,
       HR_TOTAL_SURV = HR_CTR + CTR_N, HR_TOTAL_RESULTS = HR_TOTAL_SURV + 1, HR_CONF = HR_TOTAL_RESULTS + 1 /* 2 words */, HR_N = HR_CONF + 2 };
constexpr size_t HR_COLD_OFF = (HR_N * sizeof(uint32_t) + 63) & ~(size_t)63;  // byte offset of the FsCold staging copy in Batch::h_read
// Host staging array WITHOUT value-initialisation: the threaded fill loops write every element, so the pages are first
// touched (and faulted in) by the worker threads instead of being zero-filled by the calling thread (a million queries
// stage ~150 MB; the single-threaded zero fill of std::vector cost a quarter of the encode time).
template <typename T>
struct HostBuf {
  T* p = nullptr;
  size_t n = 0;
  explicit HostBuf(size_t count) : p(static_cast<T*>(malloc(std::max<size_t>(count, 1) * sizeof(T)))), n(count) {}
  ~HostBuf() { free(p); }
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
  T* data() { return p; }
  size_t size() const { return n; }
};

template <typename T>
static int upload(T** dst, const void* src, size_t count, std::string& err, size_t* total) {
  const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  HIP_TRY(pool_malloc(reinterpret_cast<void**>(dst), bytes));
  if (count) HIP_TRY(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
  if (total) *total += bytes;
  return ANX_OK;
}
template <typename T>
static int dalloc(T** dst, size_t count, std::string& err) {
  HIP_TRY(pool_malloc(reinterpret_cast<void**>(dst), std::max<size_t>(count * sizeof(T), 16)));
  return ANX_OK;
}

DeviceLexicon* lexicon_upload(const LexiconImage& img, const EncodeTables& et, const AdjIndex* adj, int device, std::string& err, int dev_closure, size_t dev_budget,
                              AdjIndex* dev_stats) {
  DeviceGuard guard;
  int n = device_count(err);
  if (n <= 0) {
    if (err.empty()) err = "no HIP device available";
    return nullptr;
  }
  if (device < 0 || device >= n) { err = "invalid device ordinal"; return nullptr; }
  if (hipSetDevice(device) != hipSuccess) { err = "hipSetDevice failed"; return nullptr; }
  DeviceLexicon* d = new DeviceLexicon();
  d->device = device;
  lexicon_registered(device);
  d->nplanes = img.nplanes;
  d->nsym = img.nsym;
  d->nclasses = img.nclasses;
  d->nentries = img.nentries;
  d->cstride = img.cstride;
  d->any_variants = img.any_variants ? 1 : 0;
  uint32_t maxlen = 1;
  for (uint32_t m : img.ent_meta) maxlen = std::max(maxlen, m & 0xFFu);
  d->max_len = maxlen;
  int rc = ANX_OK;
  std::vector<EntRec> rec(img.ent_vocab.size());
  for (size_t e = 0; e < rec.size(); ++e) rec[e] = EntRec{img.ent_vocab[e], img.ent_freq[e], img.ent_order[e], img.ent_meta[e]};
  std::vector<uint4> erec(2 * img.ent_vocab.size());
  for (size_t e = 0; e < img.ent_vocab.size(); ++e) {
    memcpy(&erec[2 * e], &img.rows[(size_t)img.ent_rowoff[e] * 16], 16);
    erec[2 * e + 1] = make_uint4(img.ent_meta[e], img.ent_rowoff[e], img.ent_freq[e], 0u);
  }
  std::vector<uint4> eplanes(img.ent_vocab.size());   // {meta, symbol planes of the first 16 symbols}
  for (size_t e = 0; e < img.ent_vocab.size(); ++e) {
    uint32_t pw[3];
    symbol_planes16(&img.rows[(size_t)img.ent_rowoff[e] * 16], img.ent_meta[e] & 0xFFu, pw);
    eplanes[e] = make_uint4(img.ent_meta[e], pw[0], pw[1], pw[2]);
  }
  // scan records of the bit-plane kernel: one per ENTRY (class-major, the order of the entry ids) carrying the planes of its
  // class, so that a scan hit is a (query, entry) pair -- classes with several entries (8 % of eng.aspell) are tested once per
  // entry, and the hit expansion has no entries-per-class loop (it ran as long as the largest class among 64 hits)
  std::vector<uint4> srec((size_t)img.nentries + 1, make_uint4(0u, 0u, 0u, 0u));   // {plane 1, plane 2, len, class}
  std::vector<uint2> srec34((size_t)img.nentries + 1, make_uint2(0u, 0u));         // {plane 3, plane 4}
  for (uint32_t c = 0; c < img.nclasses; ++c)
    for (uint32_t e = img.cls_off[c]; e < img.cls_off[c + 1]; ++e) {
      srec[e] = make_uint4(img.cls_bits[c], img.cls_bits[(size_t)img.cstride + c], img.cls_len[c], c);
      srec34[e] = make_uint2(img.cls_bits[2 * (size_t)img.cstride + c], img.cls_bits[3 * (size_t)img.cstride + c]);
    }
  srec[img.nentries] = make_uint4(0u, 0u, 255u, 0xFFFFFFFFu);  // the padding record
  std::vector<uint4> sig2(img.sig_lo.size());  // {signature, first class of the run, classes in the run}
  for (size_t i = 0; i < sig2.size(); ++i)
    sig2[i] = make_uint4(img.sig_lo[i], img.sig_hi[i], img.sig_cbeg[i], i + 1 < img.sig_cbeg.size() ? img.sig_cbeg[i + 1] - img.sig_cbeg[i] : 0u);
  std::vector<uint32_t> off = img.cls_off;
  if (off.empty()) off.push_back(0);
  // Signature hash table + L1 balls of signature offsets: instead of walking the whole +-k charcount window of the signature
  // table (thousands of steps on a large lexicon) a scan tile enumerates the offsets d with sum |d_g| <= k, adds each to its own
  // signature and probes the table: 377 probes for 6 groups and k = 3, whatever the size of the lexicon.
  uint32_t hmask = 64;
  while (hmask < 4 * (uint32_t)img.nsigs) hmask <<= 1;
  std::vector<uint4> shash, shash_e;  // {sig lo, sig hi, first class / first entry of the run, classes / entries}; count 0 = empty slot
  for (;; hmask <<= 1) {  // every key within 16 probes of its home slot
    shash.assign(hmask, make_uint4(0u, 0u, 0u, 0u));
    shash_e.assign(hmask, make_uint4(0u, 0u, 0u, 0u));
    bool ok = true;
    for (uint32_t i = 0; i < img.nsigs && ok; ++i) {
      uint32_t h = sig_hash(img.sig_lo[i], img.sig_hi[i]) & (hmask - 1);
      int probes = 0;
      while (shash[h].w && probes < 16) { h = (h + 1) & (hmask - 1); ++probes; }
      if (probes == 16) { ok = false; break; }
      const uint32_t c0 = img.sig_cbeg[i], c1 = img.sig_cbeg[i + 1];  // a signature's run holds at least one class, a class one entry
      shash[h] = make_uint4(img.sig_lo[i], img.sig_hi[i], c0, c1 - c0);
      shash_e[h] = make_uint4(img.sig_lo[i], img.sig_hi[i], img.cls_off[c0], img.cls_off[c1] - img.cls_off[c0]);
    }
    if (ok) break;
  }
  d->hash_mask = hmask - 1;
  std::vector<unsigned long long> ball;
  {
    int ng = 1;
    for (uint8_t g : img.sym_group) ng = std::max(ng, (int)g + 1);
    for (int k = 0; k <= 12; ++k) {
      std::vector<unsigned long long> cur;
      int8_t dv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      bool too_big = false;
      std::function<void(int, int)> rec = [&](int g, int left) {
        if (too_big) return;
        if (g == ng) {
          unsigned long long v = 0;
          for (int i = 0; i < 8; ++i) v |= (unsigned long long)(uint8_t)dv[i] << (8 * i);
          cur.push_back(v);
          if (cur.size() > BALL_MAX) too_big = true;
          return;
        }
        for (int x = -left; x <= left; ++x) { dv[g] = (int8_t)x; rec(g + 1, left - (x < 0 ? -x : x)); }
        dv[g] = 0;
      };
      rec(0, k);
      d->ball_off[k] = (uint32_t)ball.size();
      d->ball_n[k] = too_big ? 0u : (uint32_t)cur.size();
      if (!too_big) ball.insert(ball.end(), cur.begin(), cur.end());
    }
  }
  std::vector<uint32_t> btab(26);
  for (int k = 0; k <= 12; ++k) { btab[k] = d->ball_off[k]; btab[13 + k] = d->ball_n[k]; }
  std::vector<uint4> sig2e(sig2.size());  // {signature, first entry of the run, entries in the run}
  for (size_t i = 0; i < sig2.size(); ++i) {
    const uint32_t c0 = std::min(img.sig_cbeg[i], img.nclasses), c1 = std::min(i + 1 < img.sig_cbeg.size() ? img.sig_cbeg[i + 1] : img.nclasses, img.nclasses);
    sig2e[i] = make_uint4(img.sig_lo[i], img.sig_hi[i], off[c0], off[c1] - off[c0]);
  }
  if ((rc = upload(&d->cls_planes, img.cls_planes.data(), img.cls_planes.size(), err, &d->bytes)) ||
      (rc = upload(&d->cls_bits, img.cls_bits.data(), img.cls_bits.size(), err, &d->bytes)) ||
      (rc = upload(&d->cls_len, img.cls_len.data(), img.cls_len.size(), err, &d->bytes)) ||
      (rc = upload(&d->cls_off, off.data(), off.size(), err, &d->bytes)) ||
      (rc = upload(&d->scan_rec, srec.data(), srec.size(), err, &d->bytes)) ||
      (rc = upload(&d->scan_rec34, srec34.data(), srec34.size(), err, &d->bytes)) ||
      (rc = upload(&d->sig_e, sig2e.data(), sig2e.size(), err, &d->bytes)) ||
      (rc = upload(&d->sighash, shash.data(), shash.size(), err, &d->bytes)) ||
      (rc = upload(&d->sighash_e, shash_e.data(), shash_e.size(), err, &d->bytes)) ||
      (rc = upload(&d->ball, ball.data(), ball.size(), err, &d->bytes)) ||
      (rc = upload(&d->ball_tab, btab.data(), btab.size(), err, &d->bytes)) ||
      (rc = upload(&d->sig, sig2.data(), sig2.size(), err, &d->bytes)) ||
      (rc = upload(&d->sig_cbeg, img.sig_cbeg.data(), img.sig_cbeg.size(), err, &d->bytes)) ||
      (rc = upload(&d->ent_vocab, img.ent_vocab.data(), img.ent_vocab.size(), err, &d->bytes)) ||
      (rc = upload(&d->ent_freq, img.ent_freq.data(), img.ent_freq.size(), err, &d->bytes)) ||
      (rc = upload(&d->ent_meta, img.ent_meta.data(), img.ent_meta.size(), err, &d->bytes)) ||
      (rc = upload(&d->ent_rowoff, img.ent_rowoff.data(), img.ent_rowoff.size(), err, &d->bytes)) ||
      (rc = upload(&d->ent_order, img.ent_order.data(), img.ent_order.size(), err, &d->bytes)) ||
      (rc = upload(&d->ent_rec, rec.data(), rec.size(), err, &d->bytes)) ||
      (rc = upload(&d->e_rec, erec.data(), erec.size(), err, &d->bytes)) ||
      (rc = upload(&d->e_planes, eplanes.data(), eplanes.size(), err, &d->bytes)) ||
      (rc = upload(&d->ent_var_off, img.ent_var_off.data(), img.ent_var_off.size(), err, &d->bytes)) ||
      (rc = upload(&d->var_target, img.var_target.data(), img.var_target.size(), err, &d->bytes)) ||
      (rc = upload(&d->var_target_freq, img.var_target_freq.data(), img.var_target_freq.size(), err, &d->bytes)) ||
      (rc = upload(&d->var_score, img.var_score.data(), img.var_score.size(), err, &d->bytes)) ||
      (rc = upload(reinterpret_cast<uint8_t**>(&d->rows), img.rows.data(), img.rows.size(), err, &d->bytes)) ||
      // tables of the device-side query encoder (encode.hip): flattened alphabet, symbol groups, lowercase ranges
      (rc = upload(&d->alpha.fast, et.fast, 256, err, &d->bytes)) || (rc = upload(&d->alpha.coff, et.coff, 257, err, &d->bytes)) ||
      (rc = upload(reinterpret_cast<uint32_t**>(&d->alpha.cand), et.cand.data(), et.cand.size(), err, &d->bytes)) ||
      (rc = upload(&d->alpha.bytes, et.bytes.data(), et.bytes.size(), err, &d->bytes)) ||
      (rc = upload(&d->alpha.sym_group, img.sym_group.data(), img.sym_group.size(), err, &d->bytes)) ||
      (rc = upload(reinterpret_cast<uint32_t**>(&d->alpha.lower), et.lower.data(), et.lower.size(), err, &d->bytes)) ||
      (rc = upload(&d->alpha.siglen_begin, img.siglen_begin, kMaxSymbols + 2, err, &d->bytes))) {
    lexicon_free(d);
    return nullptr;
  }
  d->alpha.nlower = (uint32_t)(et.lower.size() / 2);
  {  // x / L for x, L <= 32 as the host's IEEE division computes it (ScoreArgs::quot; until round 5 uploaded again with every batch)
    std::vector<double> quot(33 * 33, 0.0);
    for (int x = 0; x <= 32; ++x)
      for (int L = 1; L <= 32; ++L) {
        volatile double num = (double)x, den = (double)L;  // a real division at run time, as the reference does
        quot[(size_t)x * 33 + L] = num / den;
      }
    if ((rc = upload(&d->quot, quot.data(), quot.size(), err, &d->bytes))) { lexicon_free(d); return nullptr; }
  }
  if (adj && !adj->hash.empty() && img.nsym <= 32) {  // signature adjacency lists (adjacency.h): streamed by the bit-plane scan
    static_assert(sizeof(AdjSlot) == sizeof(uint4) && sizeof(AdjHdr) == 32 && sizeof(AdjPlanes) == sizeof(uint2), "adjacency records");
    if ((rc = upload(reinterpret_cast<AdjSlot**>(&d->adj_hash), adj->hash.data(), adj->hash.size(), err, &d->bytes)) ||
        (rc = upload(reinterpret_cast<AdjHdr**>(&d->adj_hdr), adj->hdr.data(), adj->hdr.size(), err, &d->bytes)) ||
        (rc = upload(reinterpret_cast<AdjPlanes**>(&d->adj_planes), adj->planes, adj->rows * kAdjRow, err, &d->bytes)) ||
        (rc = upload(&d->adj_ids, adj->ids, adj->rows * kAdjRow, err, &d->bytes))) {
      lexicon_free(d);
      return nullptr;
    }
    d->adj_mask = adj->hash_mask;
    d->adj_nhdr = (uint32_t)adj->hdr.size();
    d->adj_hash_host = adj->hash;
    d->adj_hdr_host = adj->hdr;
  } else if (!adj && dev_closure >= 0 && img.nsym <= 32) {  // built here, on the device, from the tables just uploaded (adjacency.hip)
    AdjIndex local;
    if ((rc = adjacency_build_device(d, img, dev_closure, dev_budget, dev_stats ? *dev_stats : local, err))) {
      // the lists only accelerate the scan (k_scan_bits probes the ball of a tile without a list): a build that failed -- out of
      // memory on a busy device, as a rule -- leaves a working replica without lists
      fprintf(stderr, "[anx] device %d: signature adjacency lists not built (%s): the scan probes every tile's ball itself\n", device, err.c_str());
      (void)hipGetLastError();
      for (void** p : {(void**)&d->adj_hash, (void**)&d->adj_hdr, (void**)&d->adj_planes, (void**)&d->adj_ids})
        if (*p) { pool_free(*p); *p = nullptr; }
      d->adj_mask = 0;
      d->adj_nhdr = 0;
      if (dev_stats) { dev_stats->nsig_kept = 0; dev_stats->rows = 0; dev_stats->records = 0; }
      err.clear();
    }
  }
  return d;
}

void lexicon_free(DeviceLexicon* d) {
  if (!d) return;
  DeviceGuard guard;
  (void)hipSetDevice(d->device);
  for (void* p : {(void*)d->cls_planes, (void*)d->cls_bits, (void*)d->cls_len, (void*)d->cls_off, (void*)d->scan_rec, (void*)d->scan_rec34, (void*)d->sig_e, (void*)d->sighash, (void*)d->sighash_e, (void*)d->ball, (void*)d->ball_tab, (void*)d->sig, (void*)d->sig_cbeg, (void*)d->ent_vocab,
                  (void*)d->ent_freq, (void*)d->ent_meta, (void*)d->ent_rowoff, (void*)d->ent_order, (void*)d->ent_rec, (void*)d->e_rec, (void*)d->e_planes, (void*)d->ent_var_off,
                  (void*)d->var_target, (void*)d->var_target_freq, (void*)d->var_score, (void*)d->rows, (void*)d->alpha.fast, (void*)d->alpha.coff,
                  (void*)d->alpha.cand, (void*)d->alpha.bytes, (void*)d->alpha.sym_group, (void*)d->alpha.lower, (void*)d->alpha.siglen_begin,
                  (void*)d->adj_hash, (void*)d->adj_hdr, (void*)d->adj_planes, (void*)d->adj_ids, (void*)d->quot, (void*)d->vocab_ent})
    if (p) pool_free(p);
  conf_free(d->dconf);
  lm_free(d->dlm);
  lexicon_released(d->device);  // the last model of this device: its pool goes back to the driver
  delete d;
}

static int scan_mode() { return switches().scan_sad; }  // ANX_SCAN=sad forces the general count-vector kernel (A/B testing)

// The threaded HOST encoder (ANX_ENCODE=host): the A/B reference of the device-side encoder in encode.hip, same arrays.
static int encode_host(const HostModel& m, const DeviceLexicon* dl, Batch* b, const char* const* utf8, size_t n, const anx_params& p,
                       std::string& err) {
  const bool timing = switches().encode_timing != 0;
  auto tnow = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_prev = tnow();
  auto lap = [&](const char* what) { if (timing) { const double t = tnow(); fprintf(stderr, "[anx encode] %-28s %8.2f ms\n", what, (t - t_prev) * 1e3); t_prev = t; } };
  b->status.assign(n, 0);
  const int NP = dl->nplanes;
  const bool bits_ok = dl->nsym <= 32 && !scan_mode();
  // ---- host encoding, threaded: normalisation (src/anahash.rs:50-80), count vector, threshold clamps -------
  struct Enc {
    uint32_t meta;   // len | k<<8 | d<<16 | first_is_lower<<24 ; 0 = not encodable
    uint32_t key;    // (bit-plane kinds ? 256 : 0) + len : bucket for the counting sort
    uint32_t kind;   // 0 = count-vector (SAD) scan, 1..NBITPLANES = planes the bit-plane scan compares for this query
    uint32_t off;    // offset of the norm string in its thread's arena
    uint16_t thread;
    uint16_t twin;   // twin_hash of the planes (scan_twins.hpp; kind 0: 0): the last sort key, as in the device encoder
    uint64_t sig;    // per-group symbol counts (LexiconImage::sym_group)
  };
  HostBuf<Enc> enc(n);
  unsigned nthreads = std::max(1u, std::min(32u, usable_hw_threads()));
  if (n < 4096) nthreads = 1;
  std::vector<std::vector<uint8_t>> arena(nthreads);
  const int A = m.alphabet.size();
  const size_t cvbytes = (size_t)NP * 4;
  HostBuf<uint8_t> cv_all(n * cvbytes);
  auto encode_range = [&](unsigned tid, size_t lo, size_t hi) {
    std::vector<uint8_t>& ar = arena[tid];
    ar.reserve((hi - lo) * 12);
    int16_t codes[kMaxSymbols];
    for (size_t i = lo; i < hi; ++i) {
      Enc& e = enc[i];
      e.meta = 0; e.key = 0; e.kind = 0; e.off = 0; e.thread = (uint16_t)tid; e.twin = 0; e.sig = 0;
      memset(&cv_all[i * cvbytes], 0, cvbytes);
      const int len = utf8[i] ? m.alphabet.scan_into(utf8[i], strlen(utf8[i]), codes, kMaxSymbols) : -1;
      if (len < 0) { b->status[i] = ANX_ELIMIT; continue; }
      if (len == 0) { b->status[i] = ANX_EEMPTY; continue; }
      uint8_t* cv = &cv_all[i * cvbytes];
      e.off = (uint32_t)ar.size();
      uint32_t maxcount = 0;
      for (int s = 0; s < len; ++s) {
        ar.push_back((uint8_t)(codes[s] >= 0 ? codes[s] : A + 1));                     // src/anahash.rs:76
        const uint8_t c = ++cv[(size_t)(codes[s] >= 0 ? codes[s] : A)];                // src/anahash.rs:42
        maxcount = std::max<uint32_t>(maxcount, c);
      }
      const int k = clamp_threshold(p.max_anagram_distance, len, kMaxAnagramDistance);
      const int d = clamp_threshold(p.max_edit_distance, len, kMaxEditDistance);
      e.meta = (uint32_t)len | ((uint32_t)k << 8) | ((uint32_t)d << 16) |
               (first_char_is_lowercase(utf8[i]) ? 1u << 24 : 0u);
      const uint32_t kind = (bits_ok && maxcount <= (uint32_t)NBITPLANES) ? maxcount : 0;
      e.kind = kind;
      if (kind) {  // the thermometer planes fill_range builds below, here only for their hash
        uint32_t pl[NBITPLANES] = {};
        for (size_t sym = 0; sym < cvbytes && sym < 32; ++sym)
          for (uint32_t tp = 0; tp < cv[sym] && tp < (uint32_t)NBITPLANES; ++tp) pl[tp] |= 1u << sym;
        static_assert(NBITPLANES == 4, "twin_hash takes four planes");
        e.twin = (uint16_t)twin_hash(pl[0], pl[1], pl[2], pl[3]);
      }
      e.key = (kind ? 256u : 0u) + (uint32_t)len;
      e.sig = signature_of(cv, cvbytes, m.lex.sym_group);
    }
  };
  {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nthreads; ++t) {
      const size_t lo = n * t / nthreads, hi = n * (t + 1) / nthreads;
      if (nthreads == 1) encode_range(0, lo, hi);
      else th.emplace_back(encode_range, t, lo, hi);
    }
    for (auto& x : th) x.join();
  }
  lap("normalise + count vectors");
  // (scan kernel, length)-bucketed order, stable (counting sort): a bucket shares k, d and the class window
  constexpr uint32_t NKEYS = 2 * 256;
  std::vector<size_t> kstart(NKEYS + 1, 0);
  size_t maxlen = 1;
  // per-thread histograms over contiguous input ranges -> per-thread cursors: a parallel, stable counting sort
  std::vector<std::vector<size_t>> hist(nthreads, std::vector<size_t>(NKEYS, 0));
  std::vector<size_t> t_maxlen(nthreads, 1);
  std::vector<uint32_t> t_dmax(nthreads, 0);
  auto run_threads = [&](const std::function<void(unsigned, size_t, size_t)>& f, size_t count) {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nthreads; ++t) {
      const size_t lo = count * t / nthreads, hi = count * (t + 1) / nthreads;
      if (nthreads == 1) f(0, lo, hi);
      else th.emplace_back(f, t, lo, hi);
    }
    for (auto& x : th) x.join();
  };
  run_threads([&](unsigned tid, size_t lo, size_t hi) {
    std::vector<size_t>& h = hist[tid];
    size_t ml = 1;      // thread-local: neighbouring elements of t_maxlen / t_dmax share a cache line
    uint32_t dm = 0;
    for (size_t i = lo; i < hi; ++i)
      if (enc[i].meta) {
        h[enc[i].key]++;
        ml = std::max<size_t>(ml, enc[i].meta & 0xFF);
        dm = std::max<uint32_t>(dm, (enc[i].meta >> 16) & 0xFF);
      }
    t_maxlen[tid] = ml;
    t_dmax[tid] = dm;
  }, n);
  for (unsigned t = 0; t < nthreads; ++t) {
    maxlen = std::max(maxlen, t_maxlen[t]);
    b->dmax = std::max(b->dmax, t_dmax[t]);
  }
  {
    size_t run = 0;
    for (uint32_t kx = 0; kx < NKEYS; ++kx) {
      kstart[kx] = run;
      for (unsigned t = 0; t < nthreads; ++t) {  // thread t's items of this key follow those of the threads before it
        const size_t c = hist[t][kx];
        hist[t][kx] = run;
        run += c;
      }
    }
    kstart[NKEYS] = run;
  }
  const size_t nq = kstart[NKEYS];
  b->nq = nq;
  b->qw = (uint32_t)((maxlen + 15) / 16);
  HostBuf<uint32_t> h_cv(nq * (size_t)NP), h_bits(nq * (size_t)NBITPLANES), h_meta(nq), h_orig(nq), h_kind(nq);
  HostBuf<uint64_t> h_sig(nq);
  HostBuf<uint8_t> h_rows(nq * (size_t)b->qw * 16);
  HostBuf<uint4> h_qrec(2 * nq);
  b->order.resize(nq);
  run_threads([&](unsigned tid, size_t lo, size_t hi) {
    std::vector<size_t>& cursor = hist[tid];
    for (size_t i = lo; i < hi; ++i)
      if (enc[i].meta) b->order[cursor[enc[i].key]++] = (uint32_t)i;
  }, n);
  lap("counting sort");
  {  // inside a (scan kernel, length) bucket: by (signature, kind, hash of the planes), stable -- the order of the device encoder's
     // key; equal planes end up next to each other (scan_twins.hpp); buckets are independent -> threads take them
     // round-robin.  LSD radix sort (8-bit digits, digits on which the whole bucket agrees are skipped; kind and hash are the
     // least significant digit) over (signature, kind and hash, input index) records: contiguous keys instead of a comparison sort
     // through enc[] (23 -> 8 ms per million queries)
    struct SigIdx { uint64_t sig; uint32_t idx; uint32_t kind; };  // kind: kind << kTwinHashBits | hash
    auto sort_buckets = [&](unsigned tid) {
      std::vector<SigIdx> a, t2;
      std::vector<size_t> kcnts;
      for (uint32_t kx = tid; kx < NKEYS; kx += nthreads) {
        const size_t b0 = kstart[kx], cnt = kstart[kx + 1] - b0;
        if (cnt < 2) continue;
        a.resize(cnt);
        t2.resize(cnt);
        uint64_t all_or = 0, all_and = ~0ull;
        uint32_t kind_or = 0, kind_and = ~0u;
        for (size_t i = 0; i < cnt; ++i) {
          const uint32_t x = b->order[b0 + i];
          a[i] = SigIdx{enc[x].sig, x, enc[x].kind << kTwinHashBits | enc[x].twin};
          all_or |= a[i].sig;
          all_and &= a[i].sig;
          kind_or |= a[i].kind;
          kind_and &= a[i].kind;
        }
        const uint64_t varying = all_or ^ all_and;  // bits on which some keys differ
        SigIdx *src = a.data(), *dst = t2.data();
        if (kind_or != kind_and) {  // least significant digit: the kind (0..NBITPLANES) above the hash of the planes
          constexpr int NV = (NBITPLANES + 1) << kTwinHashBits;
          kcnts.assign(NV + 1, 0);
          for (size_t i = 0; i < cnt; ++i) kcnts[src[i].kind + 1]++;
          for (int v = 0; v < NV; ++v) kcnts[v + 1] += kcnts[v];
          for (size_t i = 0; i < cnt; ++i) dst[kcnts[src[i].kind]++] = src[i];
          std::swap(src, dst);
        }
        for (int byte = 0; byte < 8; ++byte) {
          if (!((varying >> (8 * byte)) & 0xFF)) continue;
          size_t cnts[257] = {0};
          for (size_t i = 0; i < cnt; ++i) cnts[((src[i].sig >> (8 * byte)) & 0xFF) + 1]++;
          for (int v = 0; v < 256; ++v) cnts[v + 1] += cnts[v];
          for (size_t i = 0; i < cnt; ++i) dst[cnts[(src[i].sig >> (8 * byte)) & 0xFF]++] = src[i];
          std::swap(src, dst);
        }
        for (size_t i = 0; i < cnt; ++i) b->order[b0 + i] = src[i].idx;
      }
    };
    std::vector<std::thread> th;
    if (nthreads == 1) sort_buckets(0);
    else
      for (unsigned t = 0; t < nthreads; ++t) th.emplace_back(sort_buckets, t);
    for (auto& x : th) x.join();
  }
  lap("signature sort");
  auto fill_range = [&](size_t lo, size_t hi) {
    for (size_t s = lo; s < hi; ++s) {
      if (s + 8 < hi) {  // the sorted order gathers enc / cv_all / arena at random: prefetch a few queries ahead
        const size_t ip = b->order[s + 8];
        __builtin_prefetch(&enc[ip]);
        __builtin_prefetch(&cv_all[ip * cvbytes]);
      }
      if (s + 4 < hi) { const Enc& ep = enc[b->order[s + 4]]; __builtin_prefetch(&arena[ep.thread][ep.off]); }
      const size_t i = b->order[s];
      const Enc& e = enc[i];
      const uint8_t* cv = &cv_all[i * cvbytes];
      memcpy(&h_cv[s * (size_t)NP], cv, cvbytes);
      for (uint32_t tp = 0; tp < (uint32_t)NBITPLANES; ++tp) h_bits[s * NBITPLANES + tp] = 0;
      for (size_t sym = 0; sym < cvbytes && sym < 32; ++sym) {
        const uint32_t c = cv[sym];  // thermometer code: plane tp has the bit iff count > tp
        for (uint32_t tp = 0; tp < c && tp < (uint32_t)NBITPLANES; ++tp) h_bits[s * NBITPLANES + tp] |= 1u << sym;
      }
      uint8_t* row = &h_rows[s * (size_t)b->qw * 16];
      memset(row, 0xFE, (size_t)b->qw * 16);  // padding that equals nothing (kernels_score.hpp)
      memcpy(row, &arena[e.thread][e.off], e.meta & 0xFF);
      memcpy(&h_qrec[2 * s], row, 16);  // 32-B query record: first 16 symbols + meta
      {
        uint32_t pw[3];
        symbol_planes16(reinterpret_cast<const uint8_t*>(row), e.meta & 0xFFu, pw);
        h_qrec[2 * s + 1] = make_uint4(e.meta, pw[0], pw[1], pw[2]);
      }
      h_meta[s] = e.meta;
      h_orig[s] = (uint32_t)i;
      h_kind[s] = e.kind;
      h_sig[s] = e.sig;
    }
  };
  {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nthreads; ++t) {
      const size_t lo = nq * t / nthreads, hi = nq * (t + 1) / nthreads;
      if (nthreads == 1) fill_range(lo, hi);
      else th.emplace_back(fill_range, lo, hi);
    }
    for (auto& x : th) x.join();
  }
  lap("fill device images");
  // tiles: <= SCAN_TQ queries of one scan kernel, length and signature (sorted by kind inside); one wave of k_scan each
  for (size_t i = 0; i < nq;) {
    size_t j = i;
    const bool sad = h_kind[i] == 0;
    while (j < nq && (h_kind[j] == 0) == sad && (h_meta[j] & 0xFF) == (h_meta[i] & 0xFF) && h_sig[j] == h_sig[i]) ++j;
    const uint32_t lq = h_meta[i] & 0xFF, k = (h_meta[i] >> 8) & 0xFF;
    const int lo = std::max<int>(1, (int)lq - (int)k), hi = std::min<int>(kMaxSymbols, (int)lq + (int)k);
    // aligned to whole 64-signature blocks (the neighbours inside the edge blocks belong to charcounts outside the window)
    const uint32_t s0 = m.lex.siglen_begin[lo] & ~63u, s1 = (m.lex.siglen_begin[hi + 1] + 63u) & ~63u;
    const uint32_t tq = scan_tq_of(sig_group_count(m.lex.sym_group));
    // The count-vector (SAD) tiles are rare (queries with a symbol more than NBITPLANES times) and run as a launch of
    // their own: a handful of waves whose time is the latency of ONE wave walking the whole signature window.  Their
    // windows are therefore split over several waves (disjoint signature ranges = disjoint classes: same pairs).
    // probe the signature hash table with the L1 ball of offsets when that is cheaper than walking the window (engine: lexicon_upload)
    uint32_t ball0 = 0, balln = 0;
    if (probe_enabled() && k <= 12 && tile_probes(dl->ball_n[k], s1 - s0, h_sig[i])) { ball0 = dl->ball_off[k]; balln = dl->ball_n[k]; }
    const uint32_t nsplit = (sad && !balln) ? 8u : 1u;
    const uint32_t step = (((s1 - s0) + nsplit - 1) / nsplit + 63u) & ~63u;
    uint32_t adj = 0;  // the signature's adjacency list (adjacency.h), as the device encoder's adj_lookup finds it
    if (!sad && k <= (uint32_t)kAdjRadius && switches().scan_adj && dl->adj_mask && dl->adj_hash_host.empty()) {
      const int rca = adjacency_host_copies(dl, err);  // (lists built on the device: the table comes down once)
      if (rca) return rca;
    }
    if (!sad && k <= (uint32_t)kAdjRadius && switches().scan_adj && !dl->adj_hash_host.empty()) {
      uint32_t h = sig_hash((uint32_t)h_sig[i], (uint32_t)(h_sig[i] >> 32)) & dl->adj_mask;
      for (int pr = 0; pr < 17; ++pr) {
        const AdjSlot& e = dl->adj_hash_host[h];
        if (!e.hdr1) break;
        if (e.lo == (uint32_t)h_sig[i] && e.hi == (uint32_t)(h_sig[i] >> 32)) { adj = e.hdr1; break; }
        h = (h + 1u) & dl->adj_mask;
      }
    }
    for (size_t s = i; s < j; s += tq) {
      const uint32_t tn = (uint32_t)std::min<size_t>(tq, j - s);
      uint32_t ke[3] = {0, 0, 0};  // end of the kind-1 / kind-2 / kind-3 queries inside the tile
      for (uint32_t x = 0; x < tn; ++x)
        for (uint32_t kd = h_kind[s + x]; kd >= 1 && kd <= 3; ++kd) ke[kd - 1]++;
      const uint32_t kend = sad ? 0u : (ke[0] | ke[1] << 8 | ke[2] << 16);
      for (uint32_t part = 0; part < nsplit; ++part) {
        const uint32_t a0 = s0 + part * step, a1 = std::min(s1, a0 + step);
        if (a0 >= a1 && part) break;
        b->tiles.push_back(Tile{(uint32_t)s, tn, a0, a1, k, lq, (uint32_t)h_sig[i], (uint32_t)(h_sig[i] >> 32), sad ? 0u : 1u,
                                (h_meta[i] >> 16) & 0xFFu, kend, ball0, balln, adj, (s == i && part == 0u) ? 1u : 0u});
      }
    }
    i = j;
  }
  // longest-processing-time-first: cost ~ queries (the compatible classes per query vary little inside a length)
  // bit-plane tiles first, the SAD tiles (kind 0) after them: two launches
  auto tile_cost = [&](const Tile& x) {
    return x.adj ? (uint64_t)dl->adj_hdr_host[x.adj - 1].cum[kAdjSections - 1] * (8u + x.nq) + 16u : (uint64_t)x.nq * (x.s1 - x.s0 + 64);
  };
  std::stable_sort(b->tiles.begin(), b->tiles.end(), [&](const Tile& x, const Tile& y) {
    if ((x.kind == 0) != (y.kind == 0)) return y.kind == 0;
    if ((x.adj == 0) != (y.adj == 0)) return y.adj == 0;   // the tiles of k_scan_adj first
    return tile_cost(x) > tile_cost(y);
  });
  b->n_adj_tiles = 0;
  for (const Tile& t : b->tiles) { b->n_sad_tiles += t.kind == 0; b->n_adj_tiles += t.adj != 0; }
  lap("tiles + LPT order");
  std::vector<uint32_t> h_xcls(nq, 0xFFFFFFFFu);
  if (p.stop_at_exact_match) {  // the exact anagram class of every query (the index lookup of src/lib.rs:1164-1173)
    auto lookup_range = [&](size_t lo, size_t hi) {
      std::string key(cvbytes, '\0');
      for (size_t s = lo; s < hi; ++s) {
        memcpy(&key[0], &cv_all[(size_t)b->order[s] * cvbytes], cvbytes);
        auto it = m.class_of_cv.find(key);
        if (it != m.class_of_cv.end()) h_xcls[s] = it->second;
      }
    };
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nthreads; ++t) {
      const size_t lo = nq * t / nthreads, hi = nq * (t + 1) / nthreads;
      if (nthreads == 1) lookup_range(lo, hi);
      else th.emplace_back(lookup_range, lo, hi);
    }
    for (auto& x : th) x.join();
  }
  int rc;
  if ((rc = upload(&b->q_rec, h_qrec.data(), h_qrec.size(), err, nullptr)) ||
      (rc = upload(&b->qexact, h_xcls.data(), nq, err, nullptr)) ||
      (rc = upload(&b->q_cv, h_cv.data(), h_cv.size(), err, nullptr)) ||
      (rc = upload(&b->q_bits, h_bits.data(), h_bits.size(), err, nullptr)) ||
      (rc = upload(reinterpret_cast<uint8_t**>(&b->q_rows), h_rows.data(), h_rows.size(), err, nullptr)) ||
      (rc = upload(&b->q_meta, h_meta.data(), nq, err, nullptr)) || (rc = upload(&b->q_orig, h_orig.data(), nq, err, nullptr)) ||
      (rc = upload(&b->d_tiles, b->tiles.data(), b->tiles.size(), err, nullptr)))
    return rc;
  b->ntiles = (uint32_t)b->tiles.size();
  std::vector<Tile>().swap(b->tiles);
  lap("uploads");
  return ANX_OK;
}

// what every batch needs besides its query arrays: counters, per-query accumulators, events
static int encode_tail(Batch* b, std::string& err) {
  const size_t nq = b->nq;
  int rc;
  const size_t nblk = (nq + SCAN_TILE - 1) / SCAN_TILE + 2;
  if ((rc = dalloc(&b->ctl, HR_N, err)) || (rc = dalloc(&b->qsurv, 3 * nq, err)) ||
      (rc = dalloc(&b->soff, nq + 1, err)) || (rc = dalloc(&b->qcur, nq, err)) ||
      (rc = dalloc(&b->scan_tmp, nblk, err)) || (rc = dalloc(&b->r_count, nq, err)))
    return rc;
  b->rctr = b->ctl + HR_RCTR; b->sctr = b->ctl + HR_SCTR; b->lctr = b->ctl + HR_LCTR; b->counters = b->ctl + HR_CTR;
  b->qmaxfreq = b->qsurv + nq; b->qexpand = b->qsurv + 2 * nq;  // (qexpand last: only models with variant lists clear and use it)
  return shell_acquire(b->device, *b, HR_COLD_OFF + sizeof(FsCold), err);  // events + pinned read-back block (runtime.hip)
}

Batch* batch_encode_spans(const HostModel& m, const DeviceLexicon* dl, const char* blob, size_t blob_bytes, const uint32_t* off, size_t n,
                          const anx_params& p, std::string& err, int* code, bool keep_text, bool blob_on_device, bool after_stream, void* src_stream) {
  *code = ANX_OK;
  if (blob_on_device && (off || switches().encode_host)) { err = "inputs in device memory need the device-side encoder and no host offsets"; *code = ANX_EINVAL; return nullptr; }
  if (!dl) { err = "model is not resident on a device (no HIP device / anx_model_to_device not called)"; *code = ANX_ENODEVICE; return nullptr; }
  if (hipSetDevice(dl->device) != hipSuccess) { err = "hipSetDevice failed"; *code = ANX_ENODEVICE; return nullptr; }
  if (n >= (1u << 27)) { err = "more than 2^27 inputs per batch"; *code = ANX_ELIMIT; return nullptr; }
  Batch* b = new Batch();
  b->device = dl->device;
  b->params = p;
  b->n_input = n;
  b->keep_text = keep_text;
  int rc;
  if (switches().encode_host) {  // ANX_ENCODE=host: the threaded host encoder (A/B reference)
    std::vector<uint32_t> hoff;
    if (!off) {
      if (!packed_offsets(blob, blob_bytes, n, hoff)) { err = "packed inputs hold fewer strings than announced"; *code = ANX_EINVAL; batch_free(b); return nullptr; }
      off = hoff.data();
    }
    std::vector<const char*> ptrs(n);
    for (size_t i = 0; i < n; ++i) ptrs[i] = blob + off[i];  // every span is followed by a NUL byte
    rc = encode_host(m, dl, b, ptrs.data(), n, p, err);
    if (!rc && keep_text) {  // the host encoder does not upload the inputs: the device-side confusable weighting reads them
      const size_t bytes = n ? (size_t)off[n] : 0;
      std::vector<uint32_t> o(off, off + n + 1);
      if (!n) o.assign(1, 0u);
      if ((rc = upload(&b->d_text, blob, bytes, err, nullptr)) == 0) rc = upload(&b->d_textoff, o.data(), o.size(), err, nullptr);
      b->text_bytes = bytes;
    }
  } else {
    rc = batch_encode_device(m, dl, b, blob, blob_bytes, off, n, p, err, blob_on_device, after_stream, src_stream);
  }
  if (!rc) rc = encode_tail(b, err);
  if (rc) { *code = rc; batch_free(b); return nullptr; }
  return b;
}

// n NUL-terminated strings -> one buffer + offsets (threaded), then batch_encode_spans
Batch* batch_encode(const HostModel& m, const DeviceLexicon* dl, const char* const* utf8, size_t n, const anx_params& p,
                    std::string& err, int* code, bool keep_text) {
  std::vector<uint32_t> off(n + 1, 0);
  unsigned nthreads = std::max(1u, std::min(16u, usable_hw_threads()));
  if (n < 16384) nthreads = 1;
  std::vector<size_t> part(nthreads + 1, 0);
  auto run_threads = [&](const std::function<void(unsigned, size_t, size_t)>& f) {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nthreads; ++t) {
      const size_t lo = n * t / nthreads, hi = n * (t + 1) / nthreads;
      if (nthreads == 1) f(0, lo, hi);
      else th.emplace_back(f, t, lo, hi);
    }
    for (auto& x : th) x.join();
  };
  std::vector<uint32_t> lens(n);
  std::atomic<bool> too_big{false};
  run_threads([&](unsigned t, size_t lo, size_t hi) {
    size_t sum = 0;
    for (size_t i = lo; i < hi; ++i) {
      const size_t l = utf8[i] ? strlen(utf8[i]) : 0;  // a NULL input encodes like an empty one: no results
      if (l >= (1u << 28)) too_big.store(true, std::memory_order_relaxed);
      lens[i] = (uint32_t)l;
      sum += l + 1;
    }
    part[t + 1] = sum;
  });
  for (unsigned t = 0; t < nthreads; ++t) part[t + 1] += part[t];
  if (too_big.load() || part[nthreads] >= ((size_t)1 << 32)) { err = "inputs exceed 4 GB per batch: split the batch"; *code = ANX_ELIMIT; return nullptr; }
  HostBuf<char> blob(part[nthreads] + 1);
  if (!blob.data()) { err = "out of memory"; *code = ANX_ELIMIT; return nullptr; }
  run_threads([&](unsigned t, size_t lo, size_t hi) {
    size_t pos = part[t];
    for (size_t i = lo; i < hi; ++i) {
      off[i] = (uint32_t)pos;
      if (lens[i]) memcpy(&blob[pos], utf8[i], lens[i]);
      blob[pos + lens[i]] = '\0';
      pos += (size_t)lens[i] + 1;
    }
  });
  off[n] = (uint32_t)part[nthreads];
  return batch_encode_spans(m, dl, blob.data(), blob.size(), off.data(), n, p, err, code, keep_text);
}

// tmp: nb + 2 words.  Up to SCAN_FUSED_BLOCKS blocks (2 M elements) k_scan_add adds up the block totals in front of it itself: two launches
static int exclusive_scan(const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* tmp, hipStream_t st, uint32_t* copy = nullptr) {
  const uint32_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
  if (nb == 0) return hipMemsetAsync(out, 0, sizeof(uint32_t), st) == hipSuccess ? 0 : -1;
  const int fused = nb <= SCAN_FUSED_BLOCKS ? 1 : 0;
  hipLaunchKernelGGL(k_scan_local, dim3(nb), dim3(SCAN_THREADS), 0, st, in, n, out, tmp);
  if (!fused) hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_THREADS), 0, st, tmp, nb);
  hipLaunchKernelGGL(k_scan_add, dim3(nb), dim3(SCAN_THREADS), 0, st, out, n, tmp, nb, copy, fused);
  return 0;
}

#include "launch_plan.hpp"

// ---- the scan stage: what Run::scan and the test hook debug_scan_pairs (below) both launch ------------------------------------------------
template <int NP>
static void launch_scan(ScanArgs A, uint32_t nadj, uint32_t nbits, uint32_t nsad, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  // tiles: [bit-plane tiles with an adjacency list | other bit-plane tiles | SAD kind]
  const int kt = ktimer_begin("k_scan", st);  // (off unless anx_debug_kernel_timer(1); its launch count = the runs of a batch, repeats after an overflow included)
  if (e0) (void)hipEventRecord(e0, st);  // e0 .. e1 = k_scan_adj + k_scan_bits (anx_batch_stats.ms_scan_kernel)
  const bool gen = A.want_exact || A.qpairs || !A.drop_len;
  if (nadj) {
    A.ntiles = nadj;
    if (gen) hipLaunchKernelGGL((k_scan_adj<true>), dim3((nadj + 3) / 4), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((k_scan_adj<false>), dim3((nadj + 3) / 4), dim3(256), 0, st, A);
    A.tiles += nadj;
    nbits -= nadj;
  }
  if (nbits) {
    A.ntiles = nbits;
    // the general instance for StopAtExactMatch, per-query pair counts and runs that keep every pair; production runs take the lean one
    if (A.want_exact || A.qpairs || !A.drop_len) hipLaunchKernelGGL((k_scan_bits<true>), dim3((nbits + 3) / 4), dim3(256), 0, st, A);
    else hipLaunchKernelGGL((k_scan_bits<false>), dim3((nbits + 3) / 4), dim3(256), 0, st, A);
  }
  if (e1) (void)hipEventRecord(e1, st);
  if (nsad) {
    A.tiles += nbits;
    A.ntiles = nsad;
    hipLaunchKernelGGL((k_scan_sad<NP>), dim3((nsad + 3) / 4), dim3(256), 0, st, A);
  }
  ktimer_end(kt, st);
}
// the three launches [adj | bits | sad] of a stage with at least one tile (launch_plan.hpp ScanStage); e0 .. e1 (or nullptr) around the bit-plane kernels
static void scan_stage_launch(const DeviceLexicon* dl, const ScanStage& S, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  const ScanArgs A = scan_args_of(dl, S);
  const uint32_t nsad = S.n_sad_tiles, nbits = S.ntiles - nsad, nadj = std::min(S.n_adj_tiles, nbits);
  with_nplanes(dl->nplanes, [&](auto np) { launch_scan<decltype(np)::value>(A, nadj, nbits, nsad, st, e0, e1); });
}

static int ensure_raw(Batch* b, size_t slots_per_region, std::string& err) {
  uint32_t shift = 10;
  while (((size_t)1 << shift) < slots_per_region) ++shift;
  if (shift > 25) { err = "pair list exceeds 2^31 slots: split the batch"; return ANX_ELIMIT; }
  const size_t cap = (size_t)SCAN_REGIONS << shift;
  if (cap <= b->raw_cap) return ANX_OK;
  for (void* p : {(void*)b->raw, (void*)b->p_score, (void*)b->p_meta})
    if (p) pool_free(p);
  b->raw = nullptr; b->p_score = nullptr; b->p_meta = nullptr; b->raw_cap = 0;
  int rc;
  if ((rc = dalloc(&b->raw, cap, err))) return rc;
  b->raw_cap = cap;
  b->region_shift = shift;
  return ANX_OK;
}
// per-slot outputs of the scoring kernels (12 B per slot): only the debug view of every pair needs them
static int ensure_pair_outputs(Batch* b, std::string& err) {
  if (b->p_meta) return ANX_OK;  // ensure_raw drops them whenever the pair list is regrown
  int rc;
  if ((rc = dalloc(&b->p_score, b->raw_cap, err)) || (rc = dalloc(&b->p_meta, b->raw_cap, err))) return rc;
  return ANX_OK;
}

static int ensure_surv(Batch* b, size_t cap, std::string& err) {
  if (cap <= b->surv_cap) return ANX_OK;
  for (void* p : {(void*)b->c_rows, (void*)b->r_rows, (void*)b->t_key})
    if (p) pool_free(p);
  b->c_rows = nullptr;
  b->r_rows = nullptr;
  b->t_key = nullptr;
  b->surv_cap = 0;
  int rc;
  if ((rc = dalloc(&b->c_rows, cap, err)) || (rc = dalloc(&b->r_rows, cap, err)) || (rc = dalloc(&b->t_key, cap, err))) return rc;
  b->surv_cap = cap;
  return ANX_OK;
}
// survivor records of the scoring kernels, `need` per region
static int ensure_surv_records(Batch* b, size_t need, std::string& err) {
  if (need <= b->surv_region_cap) return ANX_OK;
  if (b->surv) pool_free(b->surv);
  b->surv = nullptr;
  b->surv_region_cap = 0;
  int rc;
  if ((rc = dalloc(&b->surv, need * SCAN_REGIONS, err))) return rc;
  b->surv_region_cap = need;
  return ANX_OK;
}
// the three slot lists (SlotLists, launch_plan.hpp), `need` entries per region each
static int ensure_slot_lists(Batch* b, size_t need, std::string& err) {
  if (need <= b->list_cap) return ANX_OK;
  for (void* p : {(void*)b->list8, (void*)b->listg, (void*)b->listw})
    if (p) pool_free(p);
  b->list8 = b->listg = b->listw = nullptr;
  b->list_cap = 0;
  int rc;
  if ((rc = dalloc(&b->list8, need * SCAN_REGIONS, err)) || (rc = dalloc(&b->listg, need * SCAN_REGIONS, err)) || (rc = dalloc(&b->listw, need * SCAN_REGIONS, err))) return rc;
  b->list_cap = need;
  return ANX_OK;
}

// ---- one run of the pipeline = batch_launch (everything enqueued on the stream, NO host round trip in between) + batch_finish
// (wait for the read-back, check the capacities the launch assumed, statistics).  The launch sizes its grids and buffers from the
// previous run of the batch (first run: estimates); every kernel bounds-checks its appends, the fills come back with the one
// read-back at the end, and a run whose assumptions did not hold is repeated with the measured sizes.

// ANX_CAP_DIV=n (tests): the first-run capacity ESTIMATES are divided by n, so that the overflow -> regrow -> repeat path runs
static size_t cap_div() { return (size_t)switches().cap_div; }

// Per-query survivor segments (SurvOut::seg): C = ANX_SURV_SEG survivors per query go from the scoring kernels straight to sseg[q * C ..],
// where k_rank reads them; only the surplus (a query's survivors beyond C) takes the region lists and k_compact_grouped.  The path of
// models without variant lists at freq_weight == 0 (k_rank<true>), without early device confusables (they re-weight c_rows before
// ranking) and without StopAtExactMatch.  Returns C, or 0: the batch takes the region lists alone (switch off, another path, the
// segments beyond kSegBudget or not allocatable).
constexpr size_t kSegBudget = (size_t)4 << 30;  // bytes of segments per batch (1 M queries at C = 32: 512 MB)
static uint32_t seg_wanted(const Batch* b) {  // (without the lexicon's variant lists, the budget and the allocation)
  const uint32_t C = (uint32_t)switches().surv_seg;
  return (b->conf_mode == 2 || b->params.stop_at_exact_match || b->params.freq_weight != 0.0f) ? 0u : C;
}
static uint32_t seg_capacity(const DeviceLexicon* dl, Batch* b) {
  const uint32_t C = seg_wanted(b);
  if (!C || dl->any_variants) return 0;
  const size_t need = b->nq * (size_t)C;
  if (need * sizeof(SurvSeg) > kSegBudget) return 0;
  if (need > b->sseg_cap) {
    if (b->sseg) pool_free(b->sseg);
    b->sseg = nullptr;
    b->sseg_cap = 0;
    std::string e;
    if (dalloc(&b->sseg, need, e)) { (void)hipGetLastError(); return 0; }  // (clears the failed allocation's error)
    b->sseg_cap = need;
  }
  return C;
}
// ---- sizes carried from batch to batch (RunHints, kernels_common.hpp) ----------------------------------------------------------------
static bool same_threshold(const anx_threshold& a, const anx_threshold& b) { return a.kind == b.kind && a.value == b.value && a.ratio == b.ratio; }
// (the survivor-list fill of a run with segments is only its surplus: no hint for a run without them, and the other way round)
static bool hints_match(const RunHints& h, const Batch* b) {
  return h.valid && same_threshold(h.kth, b->params.max_anagram_distance) && same_threshold(h.dth, b->params.max_edit_distance) &&
         h.score_threshold == b->params.score_threshold && h.stop == (b->params.stop_at_exact_match ? 1 : 0) && h.seg == seg_wanted(b);
}
// first launch of a batch: fills per region / rows per query of the last finished batch of the same parameters, scaled to this batch's
// queries, + 25 %.  Only ever SHRINKS what the worst-case estimates would take.
static void hints_apply(const DeviceLexicon* dl, Batch* b) {
  if (b->runs_finished || b->hinted || b->prev_maxfill || !switches().hints || switches().cap_div != 1 || b->nq < 4096) return;
  RunHints& h = dl->hints;
  std::lock_guard<std::mutex> g(h.mu);
  if (!hints_match(h, b)) return;
  const double nq = (double)b->nq, m = 1.25;
  const double worst_fill = (nq * 140.0 + (double)b->ntiles * SCAN_CHUNK) / SCAN_REGIONS + 4096.0;
  const double fill = h.maxfill * nq * m + 8192.0;
  if (fill >= worst_fill) return;
  b->prev_maxfill = (uint32_t)fill;
  b->prev_surv_fill = (uint32_t)(h.surv_fill * nq * m + 1024.0);
  b->prev_list_fill = h.list_fill > 0 ? (uint32_t)(h.list_fill * nq * m + 1024.0) : 0u;
  b->hint_rows = (size_t)std::min(nq * 16.0 + 1024.0, h.total_surv * nq * m + 4096.0);
  b->hinted = true;
}
// a first run that stood: what it measured, per query (a running maximum that decays: alternating kinds of batches -- search mode's
// unigram and higher-order batches -- keep the larger one's sizes)
static void hints_record(const DeviceLexicon* dl, const Batch* b, uint32_t maxfill, uint32_t surv_fill, uint32_t list_fill, uint32_t total_surv) {
  if (b->nq < 4096 || !switches().hints) return;
  RunHints& h = dl->hints;
  std::lock_guard<std::mutex> g(h.mu);
  const double nq = (double)b->nq, decay = hints_match(h, b) ? 0.9 : 0.0;
  h.maxfill = std::max(maxfill / nq, h.maxfill * decay);
  h.surv_fill = std::max(surv_fill / nq, h.surv_fill * decay);
  h.list_fill = std::max(list_fill / nq, h.list_fill * decay);
  h.total_surv = std::max(total_surv / nq, h.total_surv * decay);
  h.kth = b->params.max_anagram_distance; h.dth = b->params.max_edit_distance; h.score_threshold = b->params.score_threshold;
  h.stop = b->params.stop_at_exact_match ? 1 : 0;
  h.seg = seg_wanted(b);
  h.nq = nq;
  h.valid = true;
}

// ---- the stages of batch_launch: each enqueues its part of the run on the stream ------------------------------------------------------
namespace {
struct Run {  // one batch_launch: what its stages share
  const HostModel& m;
  const DeviceLexicon* dl;
  Batch* b;
  hipStream_t st;
  std::string& err;
  uint32_t nq;
  int stop;                               // StopAtExactMatch
  uint32_t region_cap = 0, fill_cap = 0;  // setup: slots per region of the pair list / of them the scoring grid covers
  SurvOut so{};                           // score: the survivor lists and segments k_rank reads
  int setup(), scan(), score(), compact_rank(), readback();
};
}  // namespace

// sizes from the previous run of the batch or from the hints of the last batch (first run: estimates), the pair list
int Run::setup() {
  int rc;
  hints_apply(dl, b);
  if (b->raw_cap == 0 && b->hinted && (rc = ensure_raw(b, (size_t)b->prev_maxfill + (b->prev_maxfill >> 3) + 4096, err))) return rc;
  if (b->raw_cap == 0 && (rc = ensure_raw(b, (nq * (size_t)140 + (size_t)b->ntiles * SCAN_CHUNK) / SCAN_REGIONS / cap_div() + 4096, err)))
    return rc;
  region_cap = 1u << b->region_shift;
  // slots per region the scoring grid covers: the previous fill + 1/8 (first run: the whole region; blocks beyond a region's
  // fill return at once)
  fill_cap = b->prev_maxfill ? (uint32_t)std::min<size_t>(region_cap, (size_t)b->prev_maxfill + (b->prev_maxfill >> 3) + FS_BLK) : region_cap;
  b->fill_cap_launched = fill_cap;
  HIP_TRY(hipEventRecord(b->ev[0], st));
  return ANX_OK;
}

int Run::scan() {
  int rc;
  // the whole control block: the scan's counters, and already those of the later stages (nothing touches them before Run::score)
  HIP_TRY(hipMemsetAsync(b->ctl, 0, HR_N * sizeof(uint32_t), st));
  if (b->ntiles == 0) { HIP_TRY(hipEventRecord(b->ev_scan0, st)); HIP_TRY(hipEventRecord(b->ev[5], st)); }
  if (b->ntiles) {
    ScanStage S{};
    S.tiles = b->d_tiles; S.ntiles = b->ntiles; S.n_adj_tiles = b->n_adj_tiles; S.n_sad_tiles = b->n_sad_tiles; S.q_bits = b->q_bits; S.q_cv = b->q_cv;
    S.chunk = SCAN_CHUNK;  // (the small call: 64 / 32)
    S.chunk_fused = switches().scan_chunk_fused ? (uint32_t)switches().scan_chunk_fused : SCAN_CHUNK_FUSED;
    S.chunk_first = switches().scan_chunk_first ? (uint32_t)switches().scan_chunk_first : SCAN_CHUNK_FIRST;  // (the kernel caps it at the tile's chunk)
#ifdef ANX_DEBUG_SWITCHES
    { const char* e = getenv("ANX_SCAN_CHUNK"); const int v = e ? atoi(e) : 0; if (v >= 32 && v <= 1024) S.chunk = (uint32_t)v; }
#endif
    S.raw = b->raw; S.region_cap = region_cap; S.rctr = b->rctr; S.qexact = b->qexact; S.want_exact = stop;
    S.drop_len = (!stop && !b->keep_all_pairs) ? 1 : 0;
    S.q_rec = b->q_rec;
    // the band-match bound where the pair is born (not in the run that materialises every pair for the debug view, and not with
    // StopAtExactMatch, whose dropped pairs are counted by the scoring kernel from the materialised list)
    S.fuse = (switches().fuse_prefilter && switches().prefilter && S.drop_len) ? 1 : 0;
    S.twins = switches().scan_twins;
    S.qpairs = nullptr;
    if (b->count_pairs) {
      if (!b->qpairs && (rc = dalloc(&b->qpairs, nq, err))) return rc;
      HIP_TRY(hipMemsetAsync(b->qpairs, 0, nq * sizeof(uint32_t), st));
      S.qpairs = b->qpairs;
    }
    S.dbg = 0;
#ifdef ANX_DEBUG_SWITCHES
    { const char* e = getenv("ANX_SCAN_DBG"); S.dbg = e ? atoi(e) : 0; }  // read per run: tools/scan_probe.py switches it between runs
#endif
    scan_stage_launch(dl, S, st, b->ev_scan0, b->ev[5]);
  }
  HIP_TRY(hipEventRecord(b->ev[1], st));
  b->n_raw = (uint32_t)(SCAN_REGIONS << b->region_shift);  // slot space (regions are sparse)
  return ANX_OK;
}

// ---- the scoring stage: what Run::score and the test hook debug_score_slots (below) both launch ------------------------------------------
// The plan of a stage (launch_plan.hpp) with the caller's debug choices; refuses a per-lane state beyond the LDS budget.
static int score_stage_plan(const HostModel& m, const DeviceLexicon* dl, double score_threshold, uint32_t qw, uint32_t dmax, bool store_pairs, ScorePlan& plan, std::string& err) {
  plan = score_plan_of(m, dl, score_threshold, qw, dmax);
  ScoreArgs& sa = plan.sa;
#ifdef ANX_DEBUG_SWITCHES
  { const char* e = getenv("ANX_SCORE_DBG"); sa.dbg = e ? atoi(e) : 0; }
#endif
  sa.store_pairs = store_pairs ? 1 : 0;
  if (!plan.fits()) { err = "per-lane scoring state exceeds the LDS budget"; return ANX_ELIMIT; }  // (the small call hands such a call to this path)
  return ANX_OK;
}
// slot lists for the pairs the fused kernel cannot score inline: strings of 17..32 symbols (8-word kernel) and everything
// else (longer strings, d > 3).  Only a batch that can have such pairs allocates and walks them (the small call: fixed buffers, always)
static bool score_stage_needs_lists(const ScorePlan& plan, const DeviceLexicon* dl) { return !plan.fastD || plan.have_long_q || dl->max_len > 16; }
struct ScoreStage {   // the arrays and sizes of one scoring stage (the caller owns and has sized all of them)
  uint32_t nq;
  int stop;                          // StopAtExactMatch
  uint32_t region_shift, fill_cap;   // the pair list: log2(slots per region), slots per region the grid covers
  uint32_t blk;                      // slots per block of k_filter_score (FilterArgs::blk)
  bool one_launch;                   // the slot-list kernels as the small call's single launch, k_small_lists (plan.threads == 256), else the batch path's separate launches
  const uint2* raw;
  const uint32_t* q_meta;
  const uint4 *q_rows, *q_rec;
  const uint32_t* qexact;
  double* p_score;                   // per-slot outputs, or nullptr (store_pairs == 0)
  uint32_t* p_meta;
  uint32_t* qsurv;                   // [3][nq]: qsurv, qmaxfreq, qexpand
  uint32_t *rctr, *sctr, *lctr, *counters;
  SurvOut so;
  bool need_lists;
  uint32_t *list8, *listg, *listw;
  uint32_t list_cap;
  FsCold* h_cold;                    // pinned staging copy of k_filter_score's rarely used arguments, and where they go on the device
  void* d_cold;
  hipEvent_t ev_fs0, ev_fs1;         // around k_filter_score alone (nullptr: not recorded)
};
static int score_stage_launch(const DeviceLexicon* dl, const ScorePlan& plan, const ScoreStage& S, hipStream_t st, std::string& err) {
  const uint32_t nq = S.nq;
  HIP_TRY(hipMemsetAsync(S.qsurv, 0, (dl->any_variants ? 3 : 2) * (size_t)nq * sizeof(uint32_t), st));  // qsurv, qmaxfreq (, qexpand)
  const ScoreArgs& sa = plan.sa;
  const int fastD = plan.fastD;
  const SurvOut& so = S.so;
  const SlotLists sl = slot_lists_of(S.list8, S.listg, S.listw, S.lctr, S.list_cap);
  const PairArgs pa = pair_args_of(dl, S.raw, S.q_meta, S.q_rows, S.q_rec, S.p_score, S.p_meta, S.qsurv + nq, S.qsurv, S.qsurv + 2 * (size_t)nq);
  FilterArgs fa;
  fa.region_shift = S.region_shift; fa.rctr = S.rctr; fa.qexact = S.qexact; fa.stop = S.stop; fa.enable = plan.enable_filter;
  // pairs with a string of 17..32 symbols go to the 8-word register DL also when no QUERY is that long (the few 17..19-symbol candidates
  // of a short-query batch): until round 6 those went to the general LDS kernel, whose one round cost 0.05 ms (scoring stage of BASELINE
  // configs[1] 0.555 -> 0.53 ms; the three slot-list kernels as ONE launch, k_small_lists, on top of that: 0.527, not kept)
  // (the small call: only when k_small_lists runs, threads == 256)
  fa.use_nw8 = (plan.have_long_q || fastD > 0) ? 1 : 0; fa.counters = S.counters; fa.stat_ctr = S.sctr; fa.fill_cap = S.fill_cap; fa.blk = S.blk;
  const dim3 fgrid(((S.fill_cap + S.blk - 1) / S.blk) * SCAN_REGIONS);
  // k_filter_score's rarely used arguments: uploaded with every run (the small call keeps them on the device until they change)
  *S.h_cold = FsCold{sa, so, sl.l8, sl.lg, sl.lw};
  HIP_TRY(hipMemcpyAsync(S.d_cold, S.h_cold, sizeof(FsCold), hipMemcpyHostToDevice, st));
  if (S.ev_fs0) HIP_TRY(hipEventRecord(S.ev_fs0, st));  // ev_fs0 .. ev_fs1 = k_filter_score alone (anx_batch_stats.ms_filter_score_kernel)
  // (split_wide, round 6: for batches with long queries as well -- BASELINE configs[2]: 9.68 -> 9.52 ms per pass, configs[3]'s share:
  // 6.73 -> 6.42 ms per 1 M queries)
  launch_filter_score(plan, fgrid, st, fa, pa, static_cast<const FsCold*>(S.d_cold));
  if (S.ev_fs1) HIP_TRY(hipEventRecord(S.ev_fs1, st));
  const int do_wide = (plan.split_wide && plan.enable_filter) ? 1 : 0;
  if (S.need_lists && S.one_launch) {  // as small_find launches them (small_path.hpp), a block per region
    launch_small_lists_of(plan, st, sl, fa, pa, so);
  } else if (S.need_lists) {  // the list fills are only known on the device: fixed grids walk the lists in strides
    const dim3 lgrid(LIST_P * SCAN_REGIONS);
    if (do_wide) hipLaunchKernelGGL(k_filter_wide, lgrid, dim3(256), 0, st, sl.lw, fa, pa, sa, fastD, sl.l8, sl.lg);
    if (fastD) launch_score_fast8(fastD, lgrid, st, sl.l8, pa, sa, so);  // (the small call's separate launches: only with long queries)
    hipLaunchKernelGGL(k_score_pairs, lgrid, dim3(plan.threads), plan.lds_bytes(), st, sl.lg, pa, sa, so);
  }
  return ANX_OK;
}

int Run::score() {
  int rc;
  ScorePlan plan;
  if ((rc = score_stage_plan(m, dl, b->params.score_threshold, b->qw, b->dmax, b->keep_all_pairs, plan, err))) return rc;
  if (plan.sa.store_pairs && (rc = ensure_pair_outputs(b, err))) return rc;
  // survivor records: region r of the survivor list takes the survivors of region r of the pair list.  Sized from the
  // previous run (first run: half the slots the grid covers -- ~10 % of the slots survive on config 2); an overflow is
  // detected by batch_finish and the run repeated with the measured size
  if ((rc = ensure_surv_records(b, b->prev_surv_fill ? (size_t)b->prev_surv_fill + (b->prev_surv_fill >> 3) + 256 : (size_t)fill_cap / 2 / cap_div() + 256, err))) return rc;
  so = SurvOut{b->surv, b->sctr, (uint32_t)b->surv_region_cap, nullptr, seg_capacity(dl, b)};
  so.seg = so.seg_cap ? b->sseg : nullptr;
  const bool need_lists = score_stage_needs_lists(plan, dl);
  // without the inline DL (d > 3) every length-compatible pair goes to the general list; else the prefilter passes ~1/3
  if (need_lists && (rc = ensure_slot_lists(b, b->prev_list_fill ? (size_t)b->prev_list_fill + (b->prev_list_fill >> 3) + 256 : (plan.fastD ? (size_t)fill_cap / 2 : (size_t)fill_cap) / cap_div() + 256, err)))
    return rc;
  if (!b->d_cold && (rc = dalloc(reinterpret_cast<char**>(&b->d_cold), sizeof(FsCold), err))) return rc;
  ScoreStage S{};
  S.nq = nq; S.stop = stop; S.region_shift = b->region_shift; S.fill_cap = fill_cap; S.blk = FS_BLK; S.one_launch = false;
  S.raw = b->raw; S.q_meta = b->q_meta; S.q_rows = b->q_rows; S.q_rec = b->q_rec; S.qexact = b->qexact; S.p_score = b->p_score; S.p_meta = b->p_meta;
  S.qsurv = b->qsurv; S.rctr = b->rctr; S.sctr = b->sctr; S.lctr = b->lctr; S.counters = b->counters; S.so = so;
  S.need_lists = need_lists; S.list8 = b->list8; S.listg = b->listg; S.listw = b->listw; S.list_cap = (uint32_t)b->list_cap;
  S.h_cold = reinterpret_cast<FsCold*>(reinterpret_cast<char*>(b->h_read) + HR_COLD_OFF);  // pinned: a truly asynchronous copy
  S.d_cold = b->d_cold; S.ev_fs0 = b->ev_fs0; S.ev_fs1 = b->ev_fs1;
  if ((rc = score_stage_launch(dl, plan, S, st, err))) return rc;
  HIP_TRY(hipEventRecord(b->ev[2], st));
  return ANX_OK;
}

int Run::compact_rank() {
  int rc;
  // confusables weighted on the device, late mode: k_rank crops without the cutoff, conf.hip re-ranks and cuts off afterwards
  // (the small call takes no confusables: always the caller's cutoff)
  const RankArgs ra = rank_args_of(m, dl, b->params, b->conf_mode == 1 ? 0.0 : b->params.cutoff_threshold);
  exclusive_scan(b->qsurv, nq, b->soff, b->scan_tmp, st, b->qcur);  // + qcur = soff: the cursors of the compaction
  if (dl->any_variants) {
    // variant lists: a survivor expands to several rows; the row buffer and the grid of k_compact come from the survivor
    // counts, so this (rare) configuration keeps one host round trip in the middle of the run
    uint32_t total_surv = 0;
    HIP_TRY(hipMemcpyAsync(&total_surv, b->soff + nq, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(b->h_read + HR_SCTR, b->sctr, SCAN_REGIONS * RC_STRIDE * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint32_t surv_fill = 0;
    for (uint32_t r = 0; r < SCAN_REGIONS; ++r) surv_fill = std::max(surv_fill, b->h_read[HR_SCTR + r * RC_STRIDE]);
    if ((size_t)surv_fill > b->surv_region_cap) {  // survivor records were dropped: nothing of this run is used (batch_finish repeats it)
      surv_fill = 0;
      HIP_TRY(hipMemsetAsync(b->counters + CTR_OVERFLOW, 0xFF, sizeof(uint32_t), st));
    }
    if ((rc = ensure_surv(b, (size_t)total_surv + (total_surv >> 2) + 1024, err))) return rc;
    if (surv_fill) {
      CompactArgs ca{m.have_freq ? 1 : 0, dl->any_variants};
      hipLaunchKernelGGL(k_compact, dim3(((surv_fill + 255) / 256) * SCAN_REGIONS), dim3(256), 0, st, b->surv, b->sctr,
                         (uint32_t)b->surv_region_cap, ca, b->qcur, dl->ent_rec, dl->ent_var_off, dl->var_target,
                         dl->var_target_freq, dl->var_score, b->c_rows);
    }
  } else if (b->surv_cap == 0 && (rc = ensure_surv(b, b->hint_rows ? b->hint_rows : (size_t)nq * 16 / cap_div() + 1024, err))) return rc;
  const uint32_t row_cap = (uint32_t)std::min<size_t>(b->surv_cap, 0xFFFFFFFFu);
  // No host round trip between scoring and ranking: the row buffers keep the size of the previous run (first run:
  // an estimate), the kernels check the total on the device, and batch_finish repeats the run if it did not fit.
  // With segments the region lists hold only the surplus: row j of it for query q goes to c_rows[soff[q] + j].
  if (!dl->any_variants)
    hipLaunchKernelGGL(k_compact_grouped, dim3(COMPACT_P * SCAN_REGIONS), dim3(COMPACT_B), 0, st, b->surv, b->sctr,
                       (uint32_t)b->surv_region_cap, m.have_freq ? 1 : 0, b->qcur, dl->ent_rec, b->c_rows, b->soff + nq, row_cap,
                       b->counters + CTR_OVERFLOW);
  HIP_TRY(hipEventRecord(b->ev[3], st));
  if (b->conf_mode == 2 && (rc = conf_launch(m, dl, b, st, true, row_cap, err))) return rc;
  // (k_compact's rows were sized from the survivor counts on the host: k_rank has no total to check; and no segments with variant lists)
  launch_rank(ra, st, nq, b->soff, b->c_rows, b->qmaxfreq, b->qexpand, b->t_key, b->r_rows, b->r_count, dl->any_variants ? 0xFFFFFFFFu : row_cap, b->counters + CTR_OVERFLOW,
              dl->any_variants ? SegRows{nullptr, 0u, nullptr} : SegRows{so.seg, so.seg_cap, dl->ent_rec});
  if (b->conf_mode == 1 && (rc = conf_launch(m, dl, b, st, false, row_cap, err))) return rc;
  // what batch_finish wants of the ranked lists (their total and the longest), and the words of other buffers the read-back takes along
  // (after an overflow k_rank has returned early and r_count is stale: batch_finish repeats the run and uses none of this)
  hipLaunchKernelGGL(k_run_summary, dim3((nq + SCAN_THREADS * SUMMARY_ITEMS - 1) / (SCAN_THREADS * SUMMARY_ITEMS)), dim3(SCAN_THREADS), 0, st, b->r_count, nq, b->ctl,
                     (uint32_t)HR_TOTAL_RESULTS, (uint32_t)(HR_CTR + CTR_MAXROWS), b->soff + nq, (uint32_t)HR_TOTAL_SURV,
                     (b->conf_mode && b->cf_ctr) ? b->cf_ctr : nullptr, (uint32_t)HR_CONF);
  HIP_TRY(hipEventRecord(b->ev[4], st));
  return ANX_OK;
}

// the fills and totals batch_finish reads, behind everything else of the run
int Run::readback() {
  HIP_TRY(hipMemcpyAsync(b->h_read, b->ctl, HR_N * sizeof(uint32_t), hipMemcpyDeviceToHost, st));  // (HR_CONF: zero unless k_run_summary copied cf_ctr)
  HIP_TRY(hipEventRecord(b->ev_done, st));
  HIP_TRY(hipGetLastError());
  return ANX_OK;
}

static int batch_launch(const HostModel& m, const DeviceLexicon* dl, Batch* b, void* stream, std::string& err) {
  if (!dl) { err = "model is not resident on a device"; return ANX_ENODEVICE; }
  if (b->nq >= (1u << 27) || dl->nentries >= (1u << 26)) { err = "more than 2^27 queries per batch or 2^26 lexicon entries (32-bit record offsets, packed pair records)"; return ANX_ELIMIT; }
  HIP_TRY(hipSetDevice(dl->device));
  if (b->launched) {  // a run enqueued with anx_batch_run_async and never waited for: its events and read-back buffer are reused
    HIP_TRY(hipEventSynchronize(b->ev_done));
    b->launched = false;
  }
  b->last_stream = stream;
  b->ran = false;
  b->ran_keep_all = b->keep_all_pairs;  // the run that also stores the per-slot outputs the debug fetch of every pair reads
  b->n_pairs = b->n_results = b->n_surv = 0;
  b->n_raw = 0;
  if (b->nq == 0) { b->ran = true; return ANX_OK; }
  Run r{m, dl, b, reinterpret_cast<hipStream_t>(stream), err, (uint32_t)b->nq, b->params.stop_at_exact_match ? 1 : 0};
  int rc;
  if ((rc = r.setup()) || (rc = r.scan()) || (rc = r.score()) || (rc = r.compact_rank()) || (rc = r.readback())) return rc;
  b->launched = true;
  return ANX_OK;
}

// Waits for the launched run.  Returns ANX_OK with *retry = false when the run stands; *retry = true when a capacity the launch
// assumed was exceeded (the buffers have been regrown: launch again).
static int batch_finish(const HostModel& m, const DeviceLexicon* dl, Batch* b, bool* retry, std::string& err) {
  (void)m;
  *retry = false;
  if (!b->launched) return ANX_OK;  // empty batch
  HIP_TRY(hipSetDevice(dl->device));
  HIP_TRY(hipEventSynchronize(b->ev_done));
  b->launched = false;
  const uint32_t nq = (uint32_t)b->nq;
  const uint32_t* h = b->h_read;
  uint32_t maxfill = 0, surv_fill = 0, list_fill = 0;
  uint64_t n_valid = 0, n_slots = 0, nsel = 0, n_fused = 0, n_adj_rows = 0, n_adj_rows_first = 0;
  b->n_class_tests = 0;
  for (int i = 0; i <= NBITPLANES; ++i) b->n_tests_kind[i] = 0;
  for (uint32_t r = 0; r < SCAN_REGIONS; ++r) {
    const uint32_t* c = h + HR_RCTR + r * RC_STRIDE;
    maxfill = std::max(maxfill, c[RC_RAW]);
    b->region_fill[r] = c[RC_RAW];
    n_slots += c[RC_RAW];
    n_valid += c[RC_VALID];
    n_fused += c[RC_FUSED];
    n_adj_rows += c[RC_ADJ];
    n_adj_rows_first += c[RC_ADJ_FIRST];
    for (int i = 0; i <= NBITPLANES; ++i) {
      uint64_t v;
      memcpy(&v, c + RC_TESTS + 2 * i, sizeof v);
      b->n_tests_kind[i] += v;
      b->n_class_tests += v;
    }
    surv_fill = std::max(surv_fill, h[HR_SCTR + r * RC_STRIDE]);
    nsel += h[HR_SCTR + r * RC_STRIDE + 1];
    for (int l = 0; l < 3; ++l) list_fill = std::max(list_fill, h[HR_LCTR + (l * SCAN_REGIONS + r) * RC_STRIDE]);
  }
  const uint32_t total_surv = h[HR_TOTAL_SURV], total_results = h[HR_TOTAL_RESULTS];
  b->conf_fallback = b->conf_mode != 0 && (h[HR_CONF + 1] != 0 || b->conf_skipped);
  b->stats.n_conf_scripts = b->conf_mode ? h[HR_CONF] : 0;
  b->stats.n_adj_tiles = std::min(b->n_adj_tiles, b->ntiles - b->n_sad_tiles);
  // ---- did the run fit what the launch assumed? ------------------------------------------------------------
  int rc;
  bool again = false;
  size_t surv_need = total_surv;
  {
    // a pair list that overflowed, or reached beyond the scoring grid, gave the later stages only the slots that fit: what they
    // measured is scaled up to the whole list, so that the repeated run does not overflow their buffers in turn (a second repeat)
    const uint32_t covered = std::min(1u << b->region_shift, b->fill_cap_launched);
    if (maxfill > covered && covered) {
      const double f = (double)maxfill / covered;
      surv_fill = (uint32_t)std::min(surv_fill * f, 4.0e9);
      list_fill = (uint32_t)std::min(list_fill * f, 4.0e9);
      surv_need = (size_t)(total_surv * f);
    }
  }
  if (maxfill > (1u << b->region_shift)) {  // pair list
    if ((rc = ensure_raw(b, (size_t)maxfill + (maxfill >> 3) + 4096, err))) return rc;
    again = true;
  }
  if (maxfill > b->fill_cap_launched) again = true;  // slots the scoring grid did not cover
  if ((size_t)surv_fill > b->surv_region_cap) again = true;
  if (list_fill && (size_t)list_fill > b->list_cap) again = true;
  if (!dl->any_variants && surv_need > b->surv_cap) {
    if ((rc = ensure_surv(b, surv_need + (surv_need >> 2) + 1024, err))) return rc;
    again = true;
  }
  b->prev_maxfill = std::max(b->prev_maxfill, maxfill);
  b->prev_surv_fill = std::max(b->prev_surv_fill, surv_fill);
  b->prev_list_fill = std::max(b->prev_list_fill, list_fill);
  if (again) { *retry = true; b->runs_finished++; return ANX_OK; }
  if (b->runs_finished++ == 0) hints_record(dl, b, maxfill, surv_fill, list_fill, total_surv);
  if (maxfill == 0) b->n_raw = 0;
  b->n_pairs = n_valid - h[HR_CTR + CTR_SKIPPED];
  b->n_surv = total_surv;
  b->n_sel = nsel;
  b->n_results = total_results;
  b->max_rows = h[HR_CTR + CTR_MAXROWS];
  b->ran = true;
  anx_batch_stats& s = b->stats;
  s.n_queries = nq;
  s.n_pairs = b->n_pairs;
  s.n_class_tests = b->n_class_tests;
  s.n_results = total_results;
  s.n_scan_blocks = b->ntiles;
  for (int i = 0; i <= NBITPLANES; ++i) s.n_tests_kind[i] = b->n_tests_kind[i];
  s.n_pair_slots = n_slots;
  s.n_survivors = total_surv;
  s.n_selected = b->n_sel;
  s.n_prefiltered_in_scan = n_fused;
  s.n_adj_records = n_adj_rows * kAdjRow;
  s.n_adj_records_first = n_adj_rows_first * kAdjRow;
  (void)hipEventElapsedTime(&s.ms_scan, b->ev[0], b->ev[1]);
  (void)hipEventElapsedTime(&s.ms_score, b->ev[1], b->ev[2]);
  (void)hipEventElapsedTime(&s.ms_group, b->ev[2], b->ev[3]);
  (void)hipEventElapsedTime(&s.ms_rank, b->ev[3], b->ev[4]);
  (void)hipEventElapsedTime(&s.ms_total, b->ev[0], b->ev[4]);
  (void)hipEventElapsedTime(&s.ms_scan_kernel, b->ev_scan0, b->ev[5]);
  (void)hipEventElapsedTime(&s.ms_filter_score_kernel, b->ev_fs0, b->ev_fs1);
  return ANX_OK;
}

// asynchronous form: enqueue the run on `stream` and return; batch_wait completes it (repeating it synchronously in the rare
// case a capacity estimate did not hold).  Several batches in flight on different streams overlap the latency-bound tail of
// one run (compaction, ranking) with the scan of the next.
// own_streams (single-replica models, ANX_RUN_OVERLAP != 0): the run goes to one of two streams of the library's own, alternately,
// ordered behind what the caller's stream holds at this point (an event) -- so that consecutive asynchronous runs of DIFFERENT
// batches overlap (the scan of one under the scoring tail, compaction and ranking of the other) although the caller uses one
// stream: 3.11 -> 2.7-2.8 ms per step on BASELINE configs[1], what two caller streams gave before.  Everything that reads a batch's
// results requires a finished run (batch_wait has synchronised with it), so the caller's stream needs no event back.
int batch_run_async(const HostModel& m, const DeviceLexicon* dl, Batch* b, void* stream, bool own_streams, std::string& err) {
  void* use = stream;
  if (own_streams && dl && switches().run_overlap) {
    HIP_TRY(hipSetDevice(dl->device));
    hipStream_t s = run_stream_next(dl->device);
    if (s) {
      HIP_TRY(hipEventRecord(b->ev_in, reinterpret_cast<hipStream_t>(stream)));
      HIP_TRY(hipStreamWaitEvent(s, b->ev_in, 0));
      use = s;
    }
  }
  const int rc = batch_launch(m, dl, b, use, err);
  // what follows a finished run (fetches, exports, a repeated launch) goes to the CALLER's stream: on the library's shared run stream a
  // fetch would queue behind the whole run of another batch in flight there
  if (rc == ANX_OK && use != stream) b->last_stream = stream;
  return rc;
}
int batch_wait(const HostModel& m, const DeviceLexicon* dl, Batch* b, std::string& err) {
  for (int attempt = 0;; ++attempt) {
    bool retry = false;
    int rc = batch_finish(m, dl, b, &retry, err);
    if (rc || !retry) return rc;
    if (attempt == 3) { err = "the run did not fit its buffers after three regrows"; return ANX_ENODEVICE; }
    if ((rc = batch_launch(m, dl, b, b->last_stream, err))) return rc;
  }
}
int batch_run(const HostModel& m, const DeviceLexicon* dl, Batch* b, void* stream, std::string& err) {
  const int rc = batch_launch(m, dl, b, stream, err);
  return rc ? rc : batch_wait(m, dl, b, err);
}

void batch_set_last_stream(Batch* b, void* stream) { if (b && !b->launched) b->last_stream = stream; }
size_t batch_n_results(const Batch* b) { return b->ran ? (size_t)b->n_results : 0; }
size_t batch_n_input(const Batch* b) { return b->n_input; }

// ---- what results.hip and reweigh.hip ask of this translation unit: the prefix sum and k_rank -----------------------------------------------
static size_t scan_tmp_bytes(size_t n) { return ((n + SCAN_TILE - 1) / SCAN_TILE + 2) * sizeof(uint32_t); }  // exclusive_scan's tmp
size_t prefix_scan_tmp_bytes(size_t n) { return scan_tmp_bytes(n); }
int prefix_scan_enqueue(const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* tmp, hipStream_t st, uint32_t* copy) { return exclusive_scan(in, n, out, tmp, st, copy); }
void rank_rows_enqueue(const RankPlain& r, hipStream_t st, uint32_t nq, const uint32_t* soff, const SurvRow* c_rows, const uint32_t* qmaxfreq, double* t_key, DevRow* r_rows,
                       uint32_t* r_count, uint32_t row_cap, const uint32_t* overflow) {
  RankArgs ra{};
  ra.cutoff_threshold = r.cutoff_threshold;
  ra.max_matches = r.max_matches;
  ra.freq_weight = r.freq_weight;
  ra.have_freq = r.have_freq;
  ra.any_variants = 0;
  launch_rank(ra, st, nq, soff, c_rows, qmaxfreq, nullptr, t_key, r_rows, r_count, row_cap, overflow, SegRows{nullptr, 0u, nullptr});
}

// sorted position -> input index on the host (the device-side encoder only leaves it in q_orig): downloaded on first use
static int ensure_order(const Batch* cb, std::string& err) {
  Batch* b = const_cast<Batch*>(cb);
  if (b->order.size() == b->nq) return ANX_OK;
  b->order.resize(b->nq);
  if (b->nq) HIP_TRY(hipMemcpy(b->order.data(), b->q_orig, b->nq * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return ANX_OK;
}

int batch_fetch_pairs(const HostModel& m, const DeviceLexicon* dl, const Batch* cb, anx_pair** out, size_t* n,
                      std::string& err) {
  if (!cb->ran) { err = "batch has not been run"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(cb->device));
  if (!cb->ran_keep_all) {
    // the production run only counts the pairs that fail the DL's length test; this debug view lists every pair, so the
    // batch is run once more with all of them materialised (same results, same statistics)
    Batch* mb = const_cast<Batch*>(cb);
    mb->keep_all_pairs = true;
    const int rc = batch_run(m, dl, mb, nullptr, err);
    if (rc) return rc;
  }
  const Batch* b = cb;
  { const int rc = ensure_order(b, err); if (rc) return rc; }
  const size_t R = b->n_raw;
  anx_pair* res = static_cast<anx_pair*>(malloc(std::max<size_t>(1, (size_t)b->n_pairs) * sizeof(anx_pair)));
  if (!res) { err = "out of memory"; return ANX_EINVAL; }
  size_t w = 0;
  if (R) {
    std::vector<uint2> pr(R);
    std::vector<uint32_t> pm(R), ev(dl->nentries);
    std::vector<double> ps(R);
    HIP_TRY(hipMemcpy(pr.data(), b->raw, R * sizeof(uint2), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pm.data(), b->p_meta, R * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ps.data(), b->p_score, R * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ev.data(), dl->ent_vocab, (size_t)dl->nentries * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < R; ++i) {
      if ((i & (((size_t)1 << b->region_shift) - 1)) >= b->region_fill[i >> b->region_shift]) continue;  // beyond the region's fill
      if (pm[i] == META_SKIPPED || w >= b->n_pairs) continue;
      anx_pair& r = res[w++];
      r.query = b->order[pr[i].x];
      r.vocab_id = ev[pr[i].y & RAW_ENTRY_MASK];
      const uint32_t ld = pm[i] & 0x7F;
      r.ld = ld == PAIR_NONE ? (int16_t)-1 : (int16_t)ld;
      r.samecase = (pm[i] >> 7) & 1;
      r.lcs = (pm[i] >> 8) & 0xFF;
      r.prefixlen = (pm[i] >> 16) & 0xFF;
      r.suffixlen = (pm[i] >> 24) & 0xFF;
      r._pad = 0;
      r.score = ld == PAIR_NONE ? 0.0 : ps[i];
    }
  }
  *out = res;
  *n = w;
  return ANX_OK;
}

// Scored pairs per input query, counted by the scan of a PRODUCTION run (pairs that fail the DL's length test are only
// counted there, never materialised): the batch is run once more with the per-query counters switched on.
int batch_pair_counts(const HostModel& m, const DeviceLexicon* dl, Batch* b, uint32_t** out, std::string& err) {
  if (!b->ran) { err = "batch has not been run"; return ANX_EINVAL; }
  HIP_TRY(hipSetDevice(b->device));
  const bool keep = b->keep_all_pairs;
  b->keep_all_pairs = false;
  b->count_pairs = true;
  const int rc = batch_run(m, dl, b, b->last_stream, err);
  b->count_pairs = false;
  b->keep_all_pairs = keep;
  if (rc) return rc;
  { const int rc2 = ensure_order(b, err); if (rc2) return rc2; }
  uint32_t* res = static_cast<uint32_t*>(calloc(std::max<size_t>(1, b->n_input), sizeof(uint32_t)));
  if (!res) { err = "out of memory"; return ANX_EINVAL; }
  if (b->nq) {
    std::vector<uint32_t> h(b->nq);
    if (hipMemcpy(h.data(), b->qpairs, b->nq * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) { free(res); err = "hipMemcpy failed"; return ANX_ENODEVICE; }
    for (size_t s = 0; s < b->nq; ++s) res[b->order[s]] = h[s];
  }
  *out = res;
  return ANX_OK;
}

void batch_set_run_mode(Batch* b, const anx_params& p, int conf_mode) {
  b->params = p;
  b->conf_mode = conf_mode;
}
void batch_free(Batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  // the export kernels are asynchronous on the caller's stream and read this batch's buffers: they must have finished
  // before the blocks go back to the pool, where another batch / thread / stream may take them at once
  if (b->async_pending) (void)hipStreamSynchronize(reinterpret_cast<hipStream_t>(b->async_stream));
  if (b->launched) (void)hipEventSynchronize(b->ev_done);  // a run enqueued with batch_run_async and never waited for
  for (void* p : {(void*)b->q_cv, (void*)b->q_bits, (void*)b->q_rows, (void*)b->q_rec, (void*)b->q_meta, (void*)b->q_orig, (void*)b->d_tiles, (void*)b->ctl, (void*)b->surv,
                  (void*)b->qexact, (void*)b->qsurv, (void*)b->soff, (void*)b->qcur,
                  (void*)b->d_cold, (void*)b->qpairs, (void*)b->x_cnt, (void*)b->x_tmp, (void*)b->scan_tmp, (void*)b->raw, (void*)b->p_score, (void*)b->p_meta, (void*)b->list8, (void*)b->listg, (void*)b->listw,
                  (void*)b->c_rows, (void*)b->sseg, (void*)b->r_rows, (void*)b->t_key, (void*)b->r_count,
                  (void*)b->d_text, (void*)b->d_textoff, (void*)b->cf_weight, (void*)b->cf_need, (void*)b->cf_ctr, b->cf_work, (void*)b->cf_sort, b->cf_sort_tmp})
    if (p) pool_free(p);
  shell_release(b->device, *b);  // events + pinned read-back block: to the device's shells (runtime.hip) (hipHostFree / hipEventDestroy here would wait for the device)
  delete b;
}

#include "small_path.hpp"
#include "debug_doors.hpp"


}  // namespace anx
