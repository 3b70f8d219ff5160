// engine.h -- device side of the anx engine (gfx950 only).  See DESIGN.md for the data layout.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "host_model.h"
#include "adjacency.h"

namespace anx {

struct DeviceLexicon;  // HBM-resident SoA lexicon
struct Batch;          // encoded queries + pipeline buffers + results, HBM-resident

int device_count(std::string& err);
// adj: the signature adjacency lists of the image (adjacency.h; nullptr = none: every scan tile probes its ball itself)
// dev_closure >= 0 (and adj == nullptr): the lists are built ON THE DEVICE (adjacency.hip) for that closure within dev_budget bytes;
// *dev_stats (may be nullptr) receives what the host builder reports (counts and the statistics of the length split)
DeviceLexicon* lexicon_upload(const LexiconImage& img, const EncodeTables& et, const AdjIndex* adj, int device, std::string& err, int dev_closure = -1,
                              size_t dev_budget = 0, AdjIndex* dev_stats = nullptr);
void lexicon_free(DeviceLexicon*);
// test hook: the band-match bound of the scan / scoring kernels on n (query row, candidate row) pairs (engine.hip k_debug_band_bound)
int debug_band_bound(int device, const uint8_t* q_rows, const uint8_t* c_rows, const uint8_t* lq, const uint8_t* lc, size_t n, int d, int form,
                     uint8_t* out, std::string& err);
// test hook: the run's exclusive prefix sum (engine.hip exclusive_scan) on n host values: out[0 .. n], copy[0 .. n) (may be nullptr)
int debug_exclusive_scan(int device, const uint32_t* in, size_t n, uint32_t* out, uint32_t* copy, std::string& err);
// test hook: k_rank alone (engine.hip debug_rank_rows) on the caller's candidate rows, no model: nq queries of counts[q] rows, back to back
// in the physical order the caller chose.  via may be nullptr (no row has one).  seg_cap = C > 0: rows i < C of a query as SurvSeg
// records + hook-made ent_rec, the surplus in c_rows (only any_variants == 0, position 0, no via).  out_count[nq] and out_rows (the whole
// r_rows buffer: one 24-byte DevRow per candidate row, query q's ranked rows from the exclusive sum of counts) start as 0xFF bytes.
struct DebugRankIn {
  size_t nq;
  const uint32_t *counts, *maxfreq, *qexpand;
  const double* score;
  const uint32_t *order, *position, *vocab, *freq, *via;
  double cutoff_threshold;
  uint64_t max_matches;
  float freq_weight;
  int have_freq, any_variants;
  uint32_t seg_cap, row_cap, overflow;
};
int debug_rank_rows(int device, const DebugRankIn& in, uint32_t* out_count, void* out_rows, std::string& err);
// test hook: the scoring stage alone (engine.hip debug_score_slots: k_filter_score and the slot-list kernels, launched by the function a
// run launches them with) on an encoded batch and a pair list the caller laid out.  fills[SCAN_REGIONS = 64] slots per region, back to
// back in `slots` as (query input index, entry id | flags) or (0xFFFFFFFF, -) = an unused slot.  Every check of the slots runs on the host
// before the first launch (ANX_EINVAL).  The outputs (sizes in include/anx.h) are the hook's device buffers, which start as 0xFF bytes.
struct DebugScoreIn {
  uint32_t region_shift;           // log2(slots per region), 10 .. 16
  const uint32_t* fills;
  const uint32_t* slots;
  uint32_t seg_cap;                // 0, or C: per-query segments
  uint32_t surv_region_cap, list_cap, blk;
  int one_launch;                  // the slot-list kernels as k_small_lists
};
struct DebugScoreOut {
  uint32_t* meta;                  // [slots]
  double* score;                   // [slots]
  uint32_t* qcount;                // [3][inputs]: qsurv, qmaxfreq, qexpand
  void* surv;                      // [64][surv_region_cap] {u32 input, u32 entry, f64 score}
  uint32_t* ctr;                   // [5][64]: fills of the survivor list, list8, listg, listw; selected pairs
  void* seg;                       // [inputs][seg_cap] {f64 score, u32 entry, u32 0}
  uint32_t* skipped;
};
int debug_score_slots(const HostModel& m, const DeviceLexicon* dl, const Batch* b, const DebugScoreIn& in, const DebugScoreOut& out, std::string& err);
// test hook: the scan stage alone (engine.hip debug_scan_pairs: k_scan_adj / k_scan_bits / k_scan_sad launched by the function a run launches
// them with, or k_scan_small by the small call's) on tiles the product's own encoders made.  b != nullptr: the batch's tiles and queries (the
// batch is left as it is); b == nullptr: the n strings are encoded by the small path's encoder with `slots` tile slots per query.  Everything
// is validated on the host before the first launch (ANX_EINVAL).  Outputs: sizes in include/anx.h; *tiles is malloc'd.
struct DebugScanIn {
  uint32_t region_shift;           // log2(slots per region), 10 .. 25
  uint32_t chunk, chunk_fused, chunk_first;  // 32 .. 1024
  int fuse, twins, drop_len, want_exact, count_pairs;
  const char* const* utf8;         // small form
  size_t n;
  const anx_params* params;
  uint32_t slots;                  // 8, 16 or 32
};
struct DebugScanOut {
  uint32_t* counts;                // [6]: tiles, of them in the adjacency / bit-plane / count-vector launch, queries, guard slots written
  uint32_t** tiles;                // [tiles][15]
  uint32_t *q_orig, *q_kind, *q_meta, *qpairs;  // [queries] in the sorted order the tiles refer to
  uint32_t* raw;                   // [64 << region_shift][2]
  uint32_t* rctr;                  // [64][32]
};
int debug_scan_pairs(const HostModel& m, const DeviceLexicon* dl, const Batch* b, const DebugScanIn& in, const DebugScanOut& out, std::string& err);
void kernel_timer_enable(bool on);  // also clears the totals
bool kernel_timer_read(const char* name, double* total_ms, uint64_t* launches);  // waits for the recorded launches
void device_pool_trim(int device);  // hands the cached scratch blocks of the device (and the pinned result buffers) back to the driver
// result rows of batch_fetch live in cached pinned host buffers: release them with host_result_free (falls back to free())
// a non-blocking stream on `device` for a replica of a multi-device model (hipStream_t behind void*)
void* stream_create(int device, std::string& err, bool high_priority = false);  // high_priority: see engine.hip make_stream
void stream_destroy(int device, void* stream);
void* host_result_alloc(size_t bytes);
bool host_result_is_pinned(void* p);  // a block of host_result_alloc that is pinned (device-visible) host memory
void host_result_free(void* p);
void* thread_stream_begin(int device);            // see engine.hip; nullptr = nothing to end
void thread_stream_end(int device, void* stream);
void encoder_stream_set_override(void* stream);  // this thread's encodes (and lattice decodes) use `stream` (nullptr: the pool's streams again)
void host_result_cache_stats(uint64_t* hits, uint64_t* misses, uint64_t* miss_bytes);  // since the library was loaded (diagnosis)

// keep_text: the inputs' bytes stay on the device with the batch (confusable weighting on the device reads them)
Batch* batch_encode(const HostModel& m, const DeviceLexicon* dl, const char* const* utf8, size_t n,
                    const anx_params& p, std::string& err, int* code, bool keep_text = false);
// the same with the inputs in one buffer: input i = blob[off[i] .. off[i+1] - 1), followed by one NUL byte.  off == nullptr: the
// inputs are the first n NUL-terminated spans of blob[0, blob_bytes) and the device finds their offsets itself
// blob_on_device: `blob` is device memory of the replica's device (off must be nullptr then): the encoder copies it device to device
Batch* batch_encode_spans(const HostModel& m, const DeviceLexicon* dl, const char* blob, size_t blob_bytes, const uint32_t* off, size_t n,
                          const anx_params& p, std::string& err, int* code, bool keep_text = false, bool blob_on_device = false,
                          bool after_stream = false, void* src_stream = nullptr);  // after_stream: the encoder's stream first waits for what src_stream holds now
// how the following runs treat confusables: conf_mode 0 = not on the device (the caller rescored / has none), 1 = late, 2 = early
// (src/lib.rs:1591-1595 / :1505-1508); `p` = the parameters those runs use
void batch_set_run_mode(Batch* b, const anx_params& p, int conf_mode);
bool batch_conf_fallback(const Batch* b);  // the last run met a row the device could not weight: repeat it with host-side weighting
// the inputs as the batch holds them on the device (keep_text): bytes and n + 1 offsets
int batch_download_text(const Batch* b, std::string& text, std::vector<uint32_t>& off, std::string& err);

int batch_run(const HostModel& m, const DeviceLexicon* dl, Batch* b, void* stream, std::string& err);
// the same in two halves: enqueue on `stream` and return / wait for it (statistics, results usable afterwards)
int batch_run_async(const HostModel& m, const DeviceLexicon* dl, Batch* b, void* stream, bool own_streams, std::string& err);
int batch_wait(const HostModel& m, const DeviceLexicon* dl, Batch* b, std::string& err);
void batch_set_last_stream(Batch* b, void* stream);  // where the fetches / exports of a FINISHED run are enqueued from now on
int batch_fetch(const HostModel& m, const DeviceLexicon* dl, const Batch* b, anx_result** rows, size_t** offs,
                std::string& err);
// The small call (small_path.hpp): find_variants for at most 4096 inputs of at most 64 bytes in nine launches and one host wait,
// no allocation.  0: done (*rows: a block of the pinned result cache, *offs: malloc'd, as batch_fetch returns them); 1: not taken
// (too many / too long inputs, StopAtExactMatch, host-side confusable weighting, a fixed capacity exceeded): use the batch path;
// negative: device error.  Models with variant lists are taken too (k_compact_expand expands the survivors within the fixed row
// capacity), and models with confusables: `p` is the caller's own parameter set, late / early weighting follows from the model
// (four launches more, conf_launch_small; a row the device cannot weight hands the call over like a capacity).
int small_find(const HostModel& m, const DeviceLexicon* dl, const char* const* utf8, size_t n, const anx_params& p, anx_result** rows, size_t** offs, std::string& err);
void small_stats(uint64_t* out);  // out[0] = calls the small path answered, out[1] = calls it handed to the batch path after a capacity overflow
size_t batch_n_results(const Batch* b);
size_t batch_n_input(const Batch* b);
// batch_fetch into caller-provided storage: rows[0 .. batch_n_results) and offs[0 .. batch_n_input] = base + CSR offsets (a shard
// of a multi-device batch fills its slice of the whole call's arrays)
int batch_fetch_into(const Batch* b, anx_result* rows, size_t* offs, size_t base, std::string& err);
// the same as 16-byte records with u32 offsets.  via (may be null): via[0 .. batch_n_results), the vocabulary id of the variant a
// row was reached through, 0xFFFFFFFF = none; plain: a model without variant lists -- the words are written on the host, nothing
// more crosses PCIe
int batch_fetch_compact_into(const Batch* b, anx_topk_record* rows, uint32_t* offs, uint32_t* via, uint32_t base, bool plain, std::string& err);
// the measures behind the same rows (anx_batch_fetch_measures, kernels_explain.hpp): rows[r] describes row r of batch_fetch_compact_into
// with `via` -- edit distance, common substring / prefix / suffix, case flag, anagram distance and the unweighted score of (input,
// scored entry), the scored entry being the `via` item where the row has one.  The model and the replica supply the weights and the tables
int batch_fetch_measures_into(const HostModel& m, const DeviceLexicon* dl, const Batch* b, anx_row_measures* rows, uint32_t* offs, uint32_t base, std::string& err);
int batch_fetch_pairs(const HostModel& m, const DeviceLexicon* dl, const Batch* b, anx_pair** out, size_t* n,
                      std::string& err);
int batch_pair_counts(const HostModel& m, const DeviceLexicon* dl, Batch* b, uint32_t** out, std::string& err);
int batch_export_topk(const DeviceLexicon* dl, const Batch* b, void* dst, uint32_t stride, void* stream,
                      std::string& err);
int batch_export_compact(const DeviceLexicon* dl, const Batch* b, void* dst, size_t capacity, void* stream,
                         size_t* used, std::string& err);
// the top-k gather behind the C ABI: the compact export of a batch (as batch_export_compact) placed at dst on device dst_device --
// exported in place when the batch lives there, else exported on its own device and copied over (hipMemcpyPeerAsync: xGMI where the
// devices see each other, staged through the host otherwise); returns when the bytes are at their destination
size_t batch_compact_bytes(const Batch* b);
int batch_gather_compact(const DeviceLexicon* dl, const Batch* b, int dst_device, void* dst, size_t capacity, void* stream, std::string& err);
// The exports with `via` (the vocabulary id of the variant a row was reached through, 0xFFFFFFFF = none), for every model: the compact form
// followed by u32 via[n_results] (batch_compact_via_bytes in all; offsets and records byte-equal to batch_export_compact's), the gather of
// that section, and the fixed-stride form with a parallel array via[n_input * stride] (0xFFFFFFFF also in every unused slot)
size_t batch_compact_via_bytes(const Batch* b);
int batch_export_compact_via(const DeviceLexicon* dl, const Batch* b, void* dst, size_t capacity, void* stream, size_t* used, std::string& err);
int batch_gather_compact_via(const DeviceLexicon* dl, const Batch* b, int dst_device, void* dst, size_t capacity, void* stream, std::string& err);
int batch_export_topk_via(const DeviceLexicon* dl, const Batch* b, void* dst, void* via, uint32_t stride, void* stream, std::string& err);
// test hook (adjacency.hip): the adjacency lists of the given signatures as the replica holds them
int adjacency_debug_lists(const DeviceLexicon* d, const uint64_t* sigs, size_t n, uint32_t* out_cum, uint32_t** out_ids, std::string& err);
void batch_stats(const Batch* b, anx_batch_stats* s);

// ---- search mode's lattice decoding on the device (lattice.hip) ------------------------------------------------------------------
// One lattice per stretch of text between hard boundaries (src/lib.rs:2088-2276): states = boundaries + start, arcs = the variants
// of the segments (+ out-of-vocabulary and fail-safe epsilon arcs), listed per DESTINATION state in (source state, arc number)
// order; state nstates is a virtual end state behind the final states (zero-cost epsilon arcs).  Indices inside a stretch are local.
struct LatStretch {
  uint32_t nstates;          // without the virtual end state
  uint32_t in_off0;          // first of its nstates + 2 entries of LatInput::in_off
  uint32_t arc0, sym0;       // first arc / symbol
  uint32_t btok_off0, btok0; // first of its nb + 1 entries of btok_off / first boundary token
  uint32_t out0;             // first slot of its chosen symbols in the output
  float best_cost_init;      // (nb - 1) * 2 (src/lib.rs:2319)
  uint32_t ring;             // 1 + the most states an arc of the stretch spans (virtual end arcs included): the cost lists a merge reads
  uint64_t node0;            // set by the driver: first node of the stretch in the launch's node pool
};
struct LatArc { float cost; uint32_t src; uint32_t sym; };   // sym: local symbol id, 0xFFFFFFFF = epsilon
struct LatSym { uint32_t vocab_id; uint32_t boundary; };     // OutputSymbol (src/search.rs:133-150): vocab id 0 = out of vocabulary
struct LatInput {
  std::vector<LatStretch> st;
  std::vector<uint32_t> in_off;
  std::vector<LatArc> arcs;
  std::vector<LatSym> syms;
  std::vector<uint32_t> btok_off;
  std::vector<int32_t> btok;   // LM tokens of the boundary texts (-1 = not in the vocabulary)
  size_t out_total = 0;
};
// the whole call's lattices as plain arrays (search.cpp lays them out in pinned host memory: host_result_alloc)
struct LatView {
  const LatStretch* st; size_t nst;
  const uint32_t* in_off; size_t nin;
  const LatArc* arcs; size_t narcs;
  const LatSym* syms; size_t nsyms;
  const uint32_t* btok_off; size_t nboff;
  const int32_t* btok; size_t nbtok;
  size_t out_total;
  // models with context rules: beside out_syms, what covers each chosen symbol (rule << 8 | position in the rule, 0xFFFFFFFF =
  // uncovered), [out_total], written by lattice_decode; nullptr: such a model's lattices are handed back
  uint32_t* out_cover = nullptr;
};
// out_n[i] = symbols on the chosen path of stretch i (0xFFFFFFFF: not decoded here -> the host decoder), out_syms[st[i].out0 ..]
// decodes the lattices [first, first + count) of the view on the replica `dl` (a multi-device model gives every replica a share)
// The test record of anx_debug_lattice_decode (nullptr in production: nothing below happens).  budget_nodes replaces the driver's node
// budget of a launch; the device pools start as 0xFF bytes and, per launch and before they are reused or freed, come back to the
// caller's arrays.  Stretch j (relative to the decoded sub-range) owns the states [state_off(j), state_off(j) + nstates + 1) of those
// arrays, state_off = the running sum of nstates + 1; a state owns K nodes / (K + 3 & ~3) mark bytes / one count; a stretch K ctxval.
struct LatDebug {
  uint64_t budget_nodes = 0;       // in: nodes per launch, 0 = the driver's own
  uint32_t* launch_of = nullptr;   // [count]: the launch that took stretch j
  uint32_t* width_of = nullptr;    // [count]: lanes per stretch of its kernels (32 | 64)
  uint32_t* lds_of = nullptr;      // [count]: dynamic LDS bytes per block of its k_lattice launch
  uint32_t* nodes = nullptr;       // [states * K * 3]: (cost bits, parent, symbol)
  uint32_t* lm = nullptr;          // [states * K * 3]: (lp bits, n, prev), written with an LM only
  uint8_t* marks = nullptr;        // [states * (K + 3 & ~3)], written with an LM only
  uint16_t* cnts = nullptr;        // [states]
  double* ctxval = nullptr;        // [count * K], written with rules only
  uint32_t lds_limit = 0;          // out: the device's dynamic LDS limit per block the routing used
  uint32_t n_launches = 0;         // out
};
int lattice_decode(const HostModel& m, const DeviceLexicon* dl, const LatView& in, size_t first, size_t count, const anx_search_params& p,
                   uint32_t* out_n, uint32_t* out_syms, std::string& err);
// the same with the test record (lattice.hip only: anx_debug_lattice_decode lives there, so the host-only build needs no stub of it)
int lattice_decode_dbg(const HostModel& m, const DeviceLexicon* dl, const LatView& in, size_t first, size_t count, const anx_search_params& p,
                       uint32_t* out_n, uint32_t* out_syms, std::string& err, LatDebug* dbg);
void batch_free(Batch*);

// ---- caller-chosen string pairs (pairs.hip): anx_score_pairs ------------------------------------------------------------------------
// One chunk of at most PAIRS_CHUNK pairs: pair i = (a[i], b[i]), byte spans without their terminators.  out[i] receives the measures
// of pair i (unrestricted Damerau-Levenshtein, longest common substring, common prefix / suffix, case flag) and the distance score
// under the model's weights.  One upload, the encoder, at most one launch per tier (both sides <= PAIRS_SHORT_BYTES bytes: a pair per
// lane; everything else: a pair per wave), one download.
constexpr size_t PAIRS_CHUNK = (size_t)1 << 20;
constexpr uint32_t PAIRS_SHORT_BYTES = 16;
struct PairSpan { const char* p; size_t len; };
// weight != nullptr (anx_score_pairs_weighted): weight[i] = the product of the weights of the model's confusables found in the edit
// script of (a[i] -> b[i]) (src/lib.rs:1733-1756), 1.0 for a pair with a status or a model without confusables; `out` is what the
// unweighted call writes.  Screen and edit script run on the device behind the pair kernels (conf.hip); a pair beyond the device's
// fixed capacities, and every pair under ANX_CONFUSABLES=host, is weighted by HostModel::confusable_weight_text.
int score_pairs_chunk(const HostModel& m, const DeviceLexicon* dl, const PairSpan* a, const PairSpan* b, size_t n, anx_pair_score* out, std::string& err,
                      double* weight = nullptr);
// running totals of the weighted calls: pairs seen, pairs the screen gave 1.0 without a script, scripts run on the device, pairs weighted on the host
void pairs_conf_stats(uint64_t out[4]);

// ---- learn mode's fold on the device (learn.hip) ------------------------------------------------------------------------------------
struct LearnVocab;  // vocabulary hash table of one device (text hash -> id): built on first use, rebuilt when the vocabulary size or ANX_LEARN_HASH_BITS changes
void learn_vocab_free(LearnVocab*);
// one compact export section (anx_batch_gather_compact layout) on the fold's device: u32 offsets[n + 1] padded to 16 bytes, then the
// records; its inputs are the call's inputs lo + j, or idx[j] (host array) when idx is set
void* learn_device_alloc(int device, size_t bytes);  // the gather buffers of a learn call (nullptr: out of memory / HIP error)
void learn_device_free(int device, void* p);
bool learn_device_upload(int device, void* dst, const void* src, size_t bytes);  // host -> gather buffer (anx_debug_learn_fold_rows)
struct LearnSection { const void* base; size_t n; size_t lo; const uint32_t* idx; };
// the fold of n inputs (blob[soff[i] .. soff[i+1] - 1) + NUL, host memory) over the n_rows rows of the sections, on `device`
int learn_fold_device(const HostModel& m, int device, LearnVocab** vocab, const char* blob, const uint32_t* soff, size_t n,
                      const std::vector<LearnSection>& secs, size_t n_rows, LearnFold& out, std::string& err);

// ---- gold evaluation (eval.hip): anx_evaluate_gold -----------------------------------------------------------------------------------
// One chunk of at most PAIRS_CHUNK (input, gold) pairs whose ranked rows lie in compact export sections on replica 0's device (the
// layout learn mode gathers: LearnSection, inputs relative to the chunk; sec_rows[s] = the records of section s).  out[i] = the
// anx_gold_eval record of pair i; pairs (may be nullptr): what score_pairs_chunk writes for the same pairs.  One upload of the 2 n
// strings, the encoder with `p`'s thresholds, the pair kernels, the vocabulary lookup of the gold strings, k_eval_rows over the
// gathered rows, k_eval_classify, one download.  *vocab: the model's learn table (the caller holds the learn lock).
void* eval_device_alloc(int device, size_t bytes);  // a gather buffer from the device's scratch pool (nullptr: out of memory / HIP error)
void eval_device_free(int device, void* p);
int evaluate_chunk(const HostModel& m, const DeviceLexicon* dl, LearnVocab** vocab, const PairSpan* a, const PairSpan* gold, size_t n, const anx_params& p,
                   const std::vector<LearnSection>& secs, const std::vector<size_t>& sec_rows, anx_gold_eval* out, anx_pair_score* pairs, std::string& err);

// ---- search mode in one device pass (lattice.hip): the lattices are built on the device from the rows of the part's batches --------------
// What the host knows without any result: the segments ("matches") of every stretch, in the order of the stretch's match list
// (order-major), the states they connect, and the layout of the arcs ("groups", listed per destination state in (source state,
// insertion) order: a segment's variants | the epsilon arc of a state | an arc into the virtual end state).
struct OnePassIn {
  size_t nmatch = 0, ngroup = 0, nin = 0, nst = 0;
  const uint32_t* m_q = nullptr;     // [nmatch] input index of the segment in its batch (order 1: the unigram batch, else the higher-order batch); 0xFFFFFFFF: none
  const uint32_t* m_u0 = nullptr;    // [nmatch] order > 1: the unigram matches [u0, u1) (part-wide match indices) that lie inside the segment (redundant_match)
  const uint32_t* m_u1 = nullptr;
  const uint32_t* m_pack = nullptr;  // [nmatch] source state | destination state << 12 | order << 24 | (ends at no boundary) << 31
  const uint32_t* m_lat = nullptr;   // [nmatch] lattice of its stretch (index into st), 0xFFFFFFFF: the stretch has no lattice
  const uint32_t* g_ref = nullptr;   // [ngroup] kind << 30 | value: 0 match index, 1 epsilon arc (value = source state), 2 arc into the end state (value = source state)
  const uint32_t* e_g0 = nullptr;    // [nin] first group of every (lattice, state) entry of in_off: nstates + 2 per lattice
  const uint32_t* e_lat = nullptr;   // [nin] its lattice
  const uint32_t* st_m0 = nullptr;   // [nst] first match of the lattice's stretch
  const uint32_t* st_e0 = nullptr;   // [nst] first in_off entry of the lattice (= LatStretch::in_off0)
  LatStretch* st = nullptr;          // [nst] nstates, in_off0, btok_off0, btok0, out0, best_cost_init, ring set; arc0 / sym0 are the device's
  const uint32_t* maxdeg = nullptr;  // [nst] upper bound of the incoming arcs of a state
  const uint32_t* btok_off = nullptr; size_t nboff = 0;
  const int32_t* btok = nullptr; size_t nbtok = 0;
  size_t out_total = 0;              // out slots (LatStretch::out0: nstates per lattice)
};
struct OnePassOut {   // host_result_alloc'd (block, rows): release with host_result_free
  char* block = nullptr;
  uint32_t* out_n = nullptr;    // [nst] symbols on the chosen path
  uint32_t* e_match = nullptr;  // [out_total] per out slot: match index within its stretch
  uint32_t* e_sel = nullptr;    // ... chosen variant, 0xFFFFFFFF = none (out of vocabulary)
  uint32_t* e_row0 = nullptr;   // [out_total + 1] ... first of the match's rows in `rows`
  uint32_t* cover = nullptr;    // [out_total] models with context rules (else nullptr): rule << 8 | position in the rule that covers the symbol, 0xFFFFFFFF = uncovered
  anx_result* rows = nullptr;
  size_t n_rows = 0;
  bool handed_back = false;     // some lattice is beyond the device decoder's limits: nothing above is valid, take the classic path
};
struct OnePassState;
int search_onepass_prepare(const DeviceLexicon* dl, const Batch* bu, Batch* bh, const OnePassIn& in, const anx_search_params& p, OnePassState** out, std::string& err);
int search_onepass_finish(const HostModel& m, const DeviceLexicon* dl, OnePassState* s, const Batch* bu, const Batch* bh, OnePassIn& in, const anx_search_params& p,
                          OnePassOut& out, std::string& err);
int search_onepass_rows_wait(OnePassState* s, std::string& err);  // the row array of search_onepass_finish is complete
void search_onepass_free(OnePassState*);

}  // namespace anx
