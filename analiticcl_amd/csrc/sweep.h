// sweep.h -- anx_evaluate_sweep: what sweep_capi.cpp (host: argument checks, chunking, the batch runs of every parameter set) asks of
// sweep.hip (device: the pair side of a chunk once, then per set the rank search, the classification and the reduction to a summary).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "engine.h"

namespace anx {

// One chunk of at most PAIRS_CHUNK (input, gold) pairs on dl's device.  begin: one upload of the 2 n strings, the encoder, the pair
// kernels, the vocabulary lookup of the gold strings and the upload of the vocabulary flags -- everything that does not depend on a
// parameter set; it stays resident until end.  *vocab: the model's learn table (the caller holds the learn lock).
// want_records: the chunk keeps a record buffer, so that set() can hand the anx_gold_eval records out.
struct SweepChunk;
int sweep_chunk_begin(const HostModel& m, const DeviceLexicon* dl, LearnVocab** vocab, const PairSpan* a, const PairSpan* gold, size_t n, bool want_records,
                      SweepChunk** out, std::string& err);
// One parameter set over the chunk: the ranked rows of its inputs under `p` lie in compact export sections on the chunk's device
// (evaluate_chunk's layout).  The chunk's counts are ADDED to *sum; out (may be nullptr, needs want_records): the n records
// evaluate_chunk writes under `p`.  baseline: this is sets[0], whose "gold at rank 0" byte per pair the later sets compare with.
// Waits for the device: the sections may be freed when it returns.
int sweep_chunk_set(SweepChunk* c, const anx_params& p, bool baseline, const std::vector<LearnSection>& secs, const std::vector<size_t>& sec_rows,
                    anx_gold_summary* sum, anx_gold_eval* out, std::string& err);
// what score_pairs_chunk writes for the chunk's pairs
int sweep_chunk_pairs(SweepChunk* c, anx_pair_score* pairs, std::string& err);
void sweep_chunk_end(SweepChunk* c);
// What anx_evaluate_sweep_weights (reweigh.hip) reads of a chunk: what begin left on the chunk's device, and the chunk's stream.
struct SweepChunkView {
  const HostModel* m;
  const DeviceLexicon* dl;
  size_t n;
  void* stream;
  const uint32_t *meta, *kind, *cv, *bits;  // k_enc_strings over the 2 n strings (SweepKArgs, sweep.hip)
  const unsigned long long* sig;
  const anx_pair_score* pair;               // [n]
  const uint32_t* gid;                      // [n] gold id or 0xFFFFFFFF
  const uint8_t* vflags;                    // [V]
  uint8_t* at1;                             // [n] gold at rank 0 under set 0
  const uint8_t* blob;                      // the chunk's 2 n strings as uploaded: input i = blob[off[i] .. off[i + 1] - 1)
  const uint32_t* off;                      // [2 n + 1]
};
void sweep_chunk_view(const SweepChunk* c, SweepChunkView* v);

// anx_debug_sweep_stats: running totals since process start
enum { SWEEP_CALLS = 0, SWEEP_CHUNKS, SWEEP_SETS, SWEEP_PAIR_PASSES, SWEEP_LOOKUPS, SWEEP_BATCH_RUNS, SWEEP_BYTES_DOWN, SWEEP_NSTATS };
void sweep_stats_add(int which, uint64_t v);
void sweep_stats(uint64_t out[SWEEP_NSTATS]);

}  // namespace anx
