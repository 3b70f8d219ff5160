// gold_host.hpp -- the host steps eval.hip, sweep.hip and reweigh.hip share around the kernels of kernels_gold.hpp.
// Included inside namespace anx after kernels_gold.hpp.
#pragma once

inline unsigned gold_grid(size_t n) { return (unsigned)std::max<size_t>(1, (n + GOLD_BLOCK - 1) / GOLD_BLOCK); }

// The compact export sections of a chunk of n pairs (secs, with sec_rows[s] rows each) as the kernels read them: checks every section
// against the chunk, fills hs and enqueues the upload of the index lists on st, into blocks of `blocks`; with d_table also the upload
// of hs itself.  hs is the host source of that upload and the lists are the caller's: both live until the stream has been waited for.
// who: the caller's name in the messages.
inline int gold_sections_upload(const char* who, const std::vector<LearnSection>& secs, const std::vector<size_t>& sec_rows, size_t n, PoolBlocks& blocks, hipStream_t st,
                                std::vector<GoldSection>& hs, GoldSection** d_table, std::string& err) {
  if (secs.size() != sec_rows.size()) { err = std::string(who) + ": sections and row counts differ"; return ANX_EINVAL; }
  for (size_t s = 0; s < secs.size(); ++s)
    if (sec_rows[s] >= 0x7FFFFFFFull || secs[s].n > n || (!secs[s].idx && secs[s].lo + secs[s].n > n)) { err = std::string(who) + ": a section beyond the chunk"; return ANX_EINVAL; }
  hs.assign(secs.size(), GoldSection{});
  for (size_t s = 0; s < secs.size(); ++s) {
    const LearnSection& L = secs[s];
    const size_t off_bytes = ((L.n + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
    hs[s].off = static_cast<const uint32_t*>(L.base);
    hs[s].rec = reinterpret_cast<const anx_topk_record*>(static_cast<const char*>(L.base) + off_bytes);
    hs[s].n = (uint32_t)L.n;
    hs[s].lo = (uint32_t)L.lo;
    hs[s].rows = (uint32_t)sec_rows[s];
    if (L.idx && L.n) {
      uint32_t* d_idx = nullptr;
      if (int rc = blocks.get(&d_idx, L.n, err)) return rc;
      HIP_TRY(hipMemcpyAsync(d_idx, L.idx, L.n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      hs[s].idx = d_idx;
    }
  }
  if (d_table) {
    if (int rc = blocks.get(d_table, hs.size(), err)) return rc;
    if (!hs.empty()) HIP_TRY(hipMemcpyAsync(*d_table, hs.data(), hs.size() * sizeof(GoldSection), hipMemcpyHostToDevice, st));
  }
  return ANX_OK;
}

// the ANX_VOCAB_* bits per vocabulary item (never empty: the upload has a source)
inline void gold_vflags(const HostModel& m, std::vector<uint8_t>& out) {
  out.assign(std::max<size_t>(m.decoder.size(), 1), 0);
  for (size_t v = 0; v < m.decoder.size(); ++v) out[v] = m.decoder[v].vocabtype;
}

// The end of a set: the summary (and, with out, the n records) from the device into the pinned block h, the wait, the counters ADDED
// to *sum.  -> the bytes downloaded in *bytes.
inline int gold_set_download(char* h, const unsigned long long* d_sum, const uint4* d_out, size_t n, hipStream_t st, anx_gold_summary* sum, anx_gold_eval* out,
                             size_t* bytes, std::string& err) {
  static_assert(sizeof(anx_gold_summary) == GOLD_COUNTERS * sizeof(unsigned long long), "the summary is its counters");
  HIP_TRY(hipMemcpyAsync(h, d_sum, sizeof(anx_gold_summary), hipMemcpyDeviceToHost, st));
  if (out) HIP_TRY(hipMemcpyAsync(h + sizeof(anx_gold_summary), d_out, n * sizeof(anx_gold_eval), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint64_t* got = reinterpret_cast<const uint64_t*>(h);
  uint64_t* acc = reinterpret_cast<uint64_t*>(sum);
  for (uint32_t j = 0; j < GOLD_COUNTERS; ++j) acc[j] += got[j];
  if (out) memcpy(out, h + sizeof(anx_gold_summary), n * sizeof(anx_gold_eval));
  *bytes = sizeof(anx_gold_summary) + (out ? n * sizeof(anx_gold_eval) : 0);
  return ANX_OK;
}
