/* anx.h -- C ABI of the MI355X-native variant-scoring engine ("anx") for analiticcl.
 *
 * This header is the drop-in boundary for analiticcl's variant-query hot path.  The reference
 * (proycon/analiticcl, Rust) has no FFI of its own; the functions below are what a Rust `extern "C"`
 * block (or cgo / ctypes / N-API) binds in place of the reference's Rust methods.  Each entry point cites
 * the reference interface it replaces (paths relative to the reference tree).  INTEGRATION.md shows the
 * Rust-side binding.
 *
 * Conventions: plain pointers and sizes only; UTF-8, NUL-terminated strings borrowed for the call;
 * every function returning int returns 0 on success and a negative ANX_E* code on failure, with a
 * thread-local message available from anx_last_error(); nothing aborts across the ABI.
 * The compute path is HIP-only (gfx950): there is no CPU fallback -- calls that need the device fail
 * with ANX_ENODEVICE when no GPU is present.
 */
#ifndef ANX_H
#define ANX_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 1: rounds 1-3.
 * 2: anx_batch_stats grew (n_prefiltered_in_scan, ...) and anx_batch_get_stats(batch, out, struct_size) takes the caller's struct
 *    size as its third argument (the struct only grows at its end; a size below the version-2 struct's first 152 bytes is refused
 *    with ANX_EINVAL: a caller built against ABI 1 passes no size at all), anx_shutdown, asynchronous fetch, length-partitioned
 *    sharding.  A binding compares anx_abi_version() with the ANX_ABI_VERSION it was compiled against before it calls anything else.
 * 3: anx_pipeline_submit_packed NEVER blocks: with `depth` jobs in flight it returns ANX_ELIMIT and submits nothing (until the middle
 *    of ABI 2's life it waited instead -- a binding written against the blocking contract sees failing submits, hence the new
 *    version); anx_batch_encode_packed_device_on (the caller's stream orders the encoder behind the producer of the buffer);
 *    anx_debug_search_stats, anx_debug_small_stats (anx_find_variants_batch's path for small calls); ANX_ADJ_CLOSURE is 0..2 for every builder.  Nothing was removed; every struct of version 2 is unchanged.
 *    Added later within version 3 (additive, no struct changed): learn mode (anx_learn_*, anx_model_variants, anx_model_vocab_type,
 *    anx_format_variant_list, anx_debug_learn_stats / _times); the test hook anx_debug_learn_fold_rows and the test switch
 *    ANX_LEARN_HASH_BITS; compact records with `via` for models with variant lists (anx_batch_fetch_compact_via,
 *    anx_compact_to_results_via, anx_pipeline_next_via: additive, anx_topk_record and every existing call unchanged);
 *    anx_debug_search_lattice_stats and the test hook anx_debug_contextrule_match (models with context rules are decoded on the
 *    device: additive, results unchanged); the device-side exports with `via` (anx_batch_export_compact_via,
 *    anx_batch_gather_compact_via, anx_batch_export_topk_via: additive, the via-less exports unchanged) and the small call on
 *    multi-device models (anx_debug_small_replica_stats; results unchanged); anx_score_pairs / anx_score_pairs_packed and the
 *    struct anx_pair_score: the measures and the score of caller-chosen string pairs (additive, nothing else changed);
 *    anx_score_pairs_weighted / _packed, anx_model_confusable_weight_text and anx_debug_pairs_conf_stats: the confusable weight of
 *    such pairs (additive); the test hooks anx_debug_exclusive_scan and anx_debug_rank_rows (additive); anx_evaluate_gold /
 *    anx_evaluate_gold_packed, the struct anx_gold_eval, the ANX_GOLD_* reasons and the test hook anx_debug_evaluate_gold_chunk
 *    (additive, nothing else changed); the test hook anx_debug_score_slots (additive); anx_batch_fetch_measures, anx_measures_free and
 *    the struct anx_row_measures: the measures behind every ranked row of a batch (additive, nothing else changed);
 *    anx_mine_confusables / _packed, anx_mine_result_free, anx_default_mine_params, anx_format_confusable_list, the structs
 *    anx_mine_params / anx_mine_site / anx_mine_result and the hooks anx_debug_mine_stats / anx_debug_mine_chunk: confusable patterns
 *    mined from string pairs (additive, nothing else changed); anx_evaluate_sweep / _packed, the struct anx_gold_summary and the hooks
 *    anx_debug_evaluate_sweep_chunk / anx_debug_sweep_stats: several parameter sets over the same gold pairs (additive); the test hooks
 *    anx_debug_lattice_decode (with the struct anx_lattice_debug) and anx_debug_portable_log (additive); the test hook
 *    anx_debug_scan_pairs and its options struct anx_debug_scan_opts: additive; anx_evaluate_sweep_weights / _packed and the hooks
 *    anx_debug_evaluate_sweep_weights_chunk / anx_debug_weight_sweep_stats: sets that also differ in the score weights (additive);
 *    anx_evaluate_sweep_confusables / _packed and the hooks anx_debug_evaluate_sweep_confusables_chunk / anx_debug_sweep_conf_masks /
 *    anx_debug_conf_mask_text / anx_debug_conf_sweep_stats: candidate confusable patterns with a weight per set (additive);
 *    anx_fit_confusable_weights / _packed, the structs anx_fit_* and the hooks anx_debug_fit_confusable_weights_chunk /
 *    anx_debug_fit_select / anx_debug_fit_stats: the weights of candidate patterns fitted on the device (additive). */
#define ANX_ABI_VERSION 3

enum {
  ANX_OK = 0,
  ANX_EINVAL = -1,    /* bad argument */
  ANX_EIO = -2,       /* file could not be read (reference: io::Result from the readers) */
  ANX_ENOTBUILT = -3, /* find_variants before build() (reference prints an error and returns [], src/lib.rs:973-976) */
  ANX_ENODEVICE = -4, /* no HIP device / HIP runtime error */
  ANX_ELIMIT = -5,    /* input exceeds a documented limit (255 symbols per string, 166 alphabet classes) */
  ANX_EEMPTY = -6     /* empty query (reference panics: assert!(input_length > 0), src/lib.rs:1420) */
};

typedef struct anx_model anx_model; /* VariantModel, src/lib.rs:50-100 */
typedef struct anx_batch anx_batch; /* a batch of encoded queries + its results, resident in HBM */

/* Weights, src/types.rs:40-73 (defaults .5/.125/.125/.125/.125) */
typedef struct anx_weights {
  double ld, lcs, prefix, suffix, casew;
} anx_weights;

/* DistanceThreshold, src/types.rs:76-83 */
enum { ANX_ABSOLUTE = 0, ANX_RATIO = 1, ANX_RATIO_WITH_LIMIT = 2 };
typedef struct anx_threshold {
  uint8_t kind;
  uint8_t value; /* Absolute(value) or the limit of RatioWithLimit(ratio, value) */
  float ratio;
} anx_threshold;

/* SearchParameters, src/types.rs:112-192 (fields used by find_variants) */
typedef struct anx_params {
  anx_threshold max_anagram_distance; /* default Absolute(3) */
  anx_threshold max_edit_distance;    /* default Absolute(3) */
  uint64_t max_matches;               /* default 20; 0 = unlimited */
  double score_threshold;             /* default 0.25 */
  double cutoff_threshold;            /* default 2.0 */
  int32_t stop_at_exact_match;        /* StopCriterion::StopAtExactMatch, src/types.rs:308-313 */
  float freq_weight;                  /* default 0.0 */
} anx_params;

/* VocabParams, src/vocab.rs:108-131 */
enum { ANX_FREQ_SUM = 0, ANX_FREQ_MAX = 1, ANX_FREQ_MIN = 2, ANX_FREQ_REPLACE = 3 };
enum { ANX_VOCAB_NONE = 0, ANX_VOCAB_INDEXED = 1, ANX_VOCAB_LM = 2, ANX_VOCAB_TRANSPARENT = 4 };
typedef struct anx_vocab_params {
  uint8_t text_column;   /* default 0 */
  int16_t freq_column;   /* default 1; -1 = None */
  uint8_t freq_handling; /* default ANX_FREQ_MAX */
  uint8_t vocab_type;    /* default ANX_VOCAB_INDEXED */
} anx_vocab_params;

/* VariantResult, src/types.rs:326-332 */
#define ANX_NO_VIA UINT64_MAX
typedef struct anx_result {
  uint64_t vocab_id;
  double dist_score;
  double freq_score;
  uint64_t via; /* Option<VocabId>; ANX_NO_VIA = None */
} anx_result;

/* One scored (query, candidate) pair -- the reference's Distance (src/types.rs:289-305) for every instance
 * on which damerau_levenshtein is invoked (src/lib.rs:1343); ld = -1 where it returned None.
 * Exposed for parity tests and the "scored pairs" metric. */
typedef struct anx_pair {
  uint32_t query;    /* index into the batch */
  uint32_t vocab_id;
  int16_t ld;
  uint16_t lcs, prefixlen, suffixlen;
  uint8_t samecase;
  uint8_t _pad;
  double score;      /* dist score (src/lib.rs:1443-1452); 0 when ld < 0 */
} anx_pair;

/* Fixed-stride ranked record for device-to-device export / RCCL gather (16 B). */
typedef struct anx_topk_record {
  uint32_t vocab_id; /* UINT32_MAX = empty slot */
  float freq_score;
  double dist_score;
} anx_topk_record;

void anx_default_weights(anx_weights *);           /* Weights::default() */
void anx_default_params(anx_params *);             /* SearchParameters::default() */
void anx_default_vocab_params(anx_vocab_params *); /* VocabParams::default() */
const char *anx_last_error(void);
int anx_last_error_code(void); /* the ANX_E* code that goes with anx_last_error() (entry points that return a pointer set it too) */
int anx_abi_version(void);

/* ---- model construction (host) ------------------------------------------------------------------ */
/* VariantModel::new(alphabet_file, weights, debug), src/lib.rs:104 (+ read_alphabet :369) */
anx_model *anx_model_new(const char *alphabet_path, const anx_weights *weights, int debug);
/* VariantModel::new_with_alphabet, src/lib.rs:132; the alphabet is passed as the TSV text */
anx_model *anx_model_new_with_alphabet(const char *alphabet_tsv, const anx_weights *weights, int debug);
void anx_model_free(anx_model *);
/* read_vocabulary(filename, &VocabParams), src/lib.rs:519 */
int anx_model_read_vocabulary(anx_model *, const char *path, const anx_vocab_params *);
/* add_to_vocabulary(text, Option<u32>, &VocabParams) -> VocabId, src/lib.rs:900. Returns UINT64_MAX on error. */
uint64_t anx_model_add_to_vocabulary(anx_model *, const char *utf8, int has_frequency, uint32_t frequency,
                                     const anx_vocab_params *);
/* add_variant(ref_id, variant, score, Option<u32>, &VocabParams) -> bool, src/lib.rs:460 (+ add_variant_by_id :478).
 * Returns 1 if linked, 0 if variant == reference, negative on error. */
int anx_model_add_variant(anx_model *, uint64_t ref_id, const char *variant_utf8, double score, int has_frequency,
                          uint32_t frequency, const anx_vocab_params *);
/* read_variants(filename, Some(&VocabParams), transparent), src/lib.rs:772: weighted variant / error lists */
int anx_model_read_variants(anx_model *, const char *path, const anx_vocab_params *, int transparent);
/* build(), src/lib.rs:192: anagram classes, sorted secondary index, then the device-resident SoA lexicon.
 * `device` = HIP device ordinal to upload to; -1 = build the host index only (queries then fail with
 * ANX_ENODEVICE until anx_model_to_device succeeds). */
int anx_model_build(anx_model *, int device);
/* On-disk image of a built model: save after anx_model_build; a later run creates the
 * model with the same alphabet and calls anx_model_load_index INSTEAD of read_vocabulary / read_variants / build
 * (device >= 0 also makes it resident, like anx_model_build).  The reference has no counterpart: it rebuilds its index
 * on every start (src/lib.rs:192-245).  Confusables are not part of the image. */
int anx_model_save_index(const anx_model *, const char *path);
int anx_model_load_index(anx_model *, const char *path, int device);
/* The image stores a caller-chosen tag (any UTF-8 string; default empty) describing what it was built from -- e.g. the list of
 * resource files with sizes and content hashes -- so that a front end can tell a stale image from a current one before loading
 * it (`analiticcl_amd` CLI: --index-cache rebuilds when the tag differs).  set: before anx_model_save_index; read: the tag of
 * an image file without loading it, as a malloc'd string (anx_string_free), or NULL + anx_last_error(). */
int anx_model_set_index_tag(anx_model *, const char *tag_utf8);
char *anx_index_read_tag(const char *path);
/* names of the lexicons read so far (VariantModel::lexicons, src/lib.rs:84): bit i of a vocab item's lexindex */
uint64_t anx_model_num_lexicons(const anx_model *);
const char *anx_model_lexicon_name(const anx_model *, uint64_t i);
int anx_model_to_device(anx_model *, int device);
/* Multi-GPU, one host process (the reference's fan-out over inputs inside one process: rayon par_iter,
 * src/bin/analiticcl.rs:445-448, src/lib.rs:1883): replicate the built lexicon on the n listed HIP devices (normally every GPU of
 * the node once; an ordinal may be listed more than once = several replicas on one GPU).  Every batch call below then splits its
 * inputs over the replicas (by length, see anx_batch_shard_info), each part driven by the replica's own host thread on the replica's
 * own stream, and returns the rows in input order -- there is no collective on this path, the rows are consumed on the host.  Calls
 * with fewer than ANX_SHARD_MIN (8192) inputs per replica use fewer replicas.  Replaces the model's previous replicas.
 * anx_model_to_device(m, d) == anx_model_to_devices(m, &d, 1). */
int anx_model_to_devices(anx_model *, const int *devices, int n);
int anx_model_num_replicas(const anx_model *);
int anx_model_replica_device(const anx_model *, int replica); /* -1 when out of range */
/* has(text), src/lib.rs:331; get_vocab(id), src/lib.rs:341 */
int anx_model_has(const anx_model *, const char *utf8);
uint64_t anx_model_vocab_size(const anx_model *);
const char *anx_model_vocab_text(const anx_model *, uint64_t vocab_id);
uint32_t anx_model_vocab_frequency(const anx_model *, uint64_t vocab_id);
uint32_t anx_model_vocab_lexindex(const anx_model *, uint64_t vocab_id);
/* index statistics ("Found N instances / N anagrams / N anagrams of length L", src/lib.rs:211,220,244) */
uint64_t anx_model_num_instances(const anx_model *);
uint64_t anx_model_num_classes(const anx_model *);
uint64_t anx_model_bucket_size(const anx_model *, int charcount);
int anx_model_alphabet_size(const anx_model *); /* alphabet_size(), src/lib.rs:163 (includes UNK) */
/* normalize_to_alphabet, src/anahash.rs:50; returns length or a negative error */
int anx_model_normalize(const anx_model *, const char *utf8, uint8_t *out, int cap);
/* anahash, src/anahash.rs:16, as a decimal string; returns length or a negative error */
int anx_model_anahash(const anx_model *, const char *utf8, char *out, int cap);

/* ---- the hot path: find_variants --------------------------------------------------------------- */
/* VariantModel::find_variants(&self, &str, &SearchParameters) -> Vec<VariantResult>, src/lib.rs:972,
 * for n inputs at once (the reference's callers fan out one call per input: rayon par_iter in
 * src/bin/analiticcl.rs:445-448, src/lib.rs:1883, bindings/python/src/lib.rs:727).
 * Results are CSR: rows of query i are (*out_rows)[(*out_offsets)[i] .. (*out_offsets)[i+1]).
 * Both arrays are allocated by the library; release with anx_results_free. Thread-safe for concurrent
 * read-only use of the model. */
int anx_find_variants_batch(const anx_model *, const char *const *utf8, size_t n, const anx_params *,
                            anx_result **out_rows, size_t **out_offsets);
void anx_results_free(anx_result *rows, size_t *offsets);

/* ---- staged form of the same call (inputs/results resident in HBM between stages) --------------------
 * encode : upload of the input bytes, then ON THE DEVICE: normalisation to the alphabet (src/anahash.rs:16-80), count
 *          vectors / signatures, threshold clamps (src/lib.rs:982-1012), sort by (length, signature), tiles.
 * run    : the device pipeline (candidate scan -> pair list -> scoring -> rank [-> confusable weighting]).
 * fetch  : download + convert.  anx_find_variants_batch == encode + run + fetch + free. */
anx_batch *anx_batch_encode(const anx_model *, const char *const *utf8, size_t n, const anx_params *);
/* the same with the n inputs packed into one buffer, each terminated by a NUL byte (saves building a pointer array
 * in bindings: 1 M Python strings take 0.27 s to marshal one by one, 0.03 s packed).  The buffer goes to the device as it
 * is and the strings are found there (the first n NUL-terminated spans; anything behind them is ignored; fewer than n spans or
 * a buffer that does not end with a NUL byte: ANX_EINVAL).  An input may not contain a NUL byte itself (as in the char** form). */
anx_batch *anx_batch_encode_packed(const anx_model *, const char *blob, size_t blob_len, size_t n, const anx_params *);
/* the same for inputs that already sit in HBM: device_blob is memory of the model's (one) device, laid out like the packed buffer above
 * (every input followed by a NUL byte).  Nothing crosses PCIe; the bytes are copied device to device, so the caller's buffer is free
 * again when the call returns.  Models with several replicas and the host-side rescoring path (ANX_CONFUSABLES=host): ANX_EINVAL.
 * A trailing NUL byte is the caller's responsibility (the host cannot look).
 * Ordering: the encoder reads the buffer on a stream of its own.  anx_batch_encode_packed_device takes no stream, so the buffer must
 * be COMPLETE and visible to the device when the call is made (the work that produced it -- a kernel, an asynchronous copy -- has been
 * waited for: hipStreamSynchronize / hipDeviceSynchronize).  anx_batch_encode_packed_device_on(..., stream) instead orders the
 * encoder behind everything `stream` (a hipStream_t; NULL = the default stream) holds at the time of the call (an event recorded on it
 * that the encoder's stream waits for): the producer needs no host synchronisation. */
anx_batch *anx_batch_encode_packed_device(const anx_model *, const void *device_blob, size_t blob_len, size_t n, const anx_params *);
anx_batch *anx_batch_encode_packed_device_on(const anx_model *, const void *device_blob, size_t blob_len, size_t n, const anx_params *, void *stream);
/* `stream` is a hipStream_t (NULL = the default stream).  A model with several replicas runs every shard of the batch on its
 * replica's own stream: `stream` must then be NULL. */
int anx_batch_run(const anx_model *, anx_batch *, void *stream);
/* The same in two halves.  run_async enqueues the whole pipeline on `stream` and returns (no host round trip inside a run: grids
 * and buffers are sized from the batch's previous run or from estimates, every kernel bounds-checks, one read-back at the end);
 * wait completes it -- in the rare case an estimate did not hold it regrows the buffers and repeats the run synchronously.
 * Batches in flight overlap: the latency-bound tail of one run (compaction, ranking) runs under the scan of the next.  For a
 * single-replica model run_async therefore enqueues on one of two streams of the library's own, alternately, ordered behind what
 * `stream` holds at the time of the call (so one caller stream is enough to get the overlap; ANX_RUN_OVERLAP=0: on `stream` itself);
 * results are read through the calls below after anx_batch_wait.  anx_batch_run == launch on `stream` + wait.  (The reference's counterpart is the rayon fan-out over inputs,
 * src/bin/analiticcl.rs:445-448: independent calls in flight at once.) */
int anx_batch_run_async(const anx_model *, anx_batch *, void *stream);
int anx_batch_wait(const anx_model *, anx_batch *);
int anx_batch_fetch(const anx_batch *, anx_result **out_rows, size_t **out_offsets);
/* The same ranked rows as 16-byte anx_topk_record {vocab_id u32, freq_score f32, dist_score f64} with uint32 offsets[n + 1]: half
 * the bytes of anx_batch_fetch over PCIe (BASELINE configs[1]: 70 MB instead of 141 MB per million queries).  A record has no
 * `via`, so models with variant lists are refused (ANX_EINVAL; so are models with confusables when their lists are rescored on the
 * host -- the ANX_CONFUSABLES=host A/B path, or after a batch fell back to it --: the device-side weighting is served): use
 * anx_batch_fetch.  Rows and offsets live in one cached pinned block: release both with anx_compact_free.
 * anx_compact_to_results writes the anx_result view (via = ANX_NO_VIA) of n_rows records into caller storage. */
int anx_batch_fetch_compact(const anx_batch *, anx_topk_record **out_rows, uint32_t **out_offsets);
void anx_compact_free(anx_topk_record *rows, uint32_t *offsets);
void anx_compact_to_results(const anx_topk_record *rows, size_t n_rows, anx_result *out);
/* Compact records for EVERY model: the records of anx_batch_fetch_compact plus a parallel array out_via[n_rows], one word per row:
 * the vocabulary id of the variant the row was reached through (anx_result::via), UINT32_MAX = none.  The 16-byte record keeps its
 * layout.  A model without variant lists gets rows and offsets byte-equal to anx_batch_fetch_compact's and every word UINT32_MAX
 * (written on the host: nothing more crosses PCIe).  Rows, `via` and offsets live in one cached pinned block: release it with
 * anx_compact_free(rows, offsets).  Host-rescored confusable batches are refused as by anx_batch_fetch_compact.
 * anx_compact_to_results_via writes the anx_result view (via = ANX_NO_VIA for UINT32_MAX) of n_rows records into caller storage. */
int anx_batch_fetch_compact_via(const anx_batch *, anx_topk_record **out_rows, uint32_t **out_offsets, uint32_t **out_via);
void anx_compact_to_results_via(const anx_topk_record *rows, const uint32_t *via, size_t n_rows, anx_result *out);
/* Why a ranked row got its score ("explain"): one 16-byte record per ranked row of a batch that has run, computed on the device from
 * what is resident there.  Record r describes row r of anx_batch_fetch_compact_via on the same batch: the same rows, order and
 * offsets, for every shard layout.  The scored entry is the lexicon entry of the row's vocab_id or, when the row has a `via`, the
 * entry of `via` (the item that was matched before its variant list was expanded).  The measures are what anx_score_pairs returns for
 * (input text, text of the scored item): unrestricted Damerau-Levenshtein, longest common substring, common prefix and suffix, the
 * equality of the first-character case flags -- every one computed whatever its weight.  score is the distance score of
 * src/lib.rs:1433-1452 under the model's weights WITHOUT the confusable weight and the variant score: on a plain model it equals
 * the row's dist_score bit for bit; with confusables score * anx_model_confusable_weight(input, vocab_id) == dist_score.
 * ANX_EINVAL: NULL arguments, a batch that has not run, a batch whose confusables were rescored on the host (as
 * anx_batch_fetch_compact); ANX_ENODEVICE without a device.  A batch without rows returns ANX_OK and offsets that are all 0.
 * Rows and offsets live in one cached pinned block: release both with anx_measures_free. */
typedef struct anx_row_measures {
  double score;                          /* unweighted: no confusable weight, no variant score */
  uint8_t ld, lcs, prefixlen, suffixlen;
  uint8_t len_input, len_entry;          /* symbols */
  uint8_t anagram_distance;              /* L1 of the two count vectors: what the scan holds against k */
  uint8_t flags;                         /* bit 0 samecase, bit 1 the row has a via (the scored entry is the via item, not vocab_id) */
} anx_row_measures;                      /* 16 bytes */
#ifdef __cplusplus
static_assert(sizeof(anx_row_measures) == 16, "anx_row_measures is 16 bytes");
#else
_Static_assert(sizeof(anx_row_measures) == 16, "anx_row_measures is 16 bytes");
#endif
int anx_batch_fetch_measures(const anx_batch *, anx_row_measures **out_rows, uint32_t **out_offsets);
void anx_measures_free(anx_row_measures *rows, uint32_t *offsets);
/* The staged calls as an asynchronous pipeline for ONE caller thread (the reference's counterpart: independent find_variants calls in
 * flight on rayon's pool, src/bin/analiticcl.rs:445-448): submit hands over a packed buffer (as anx_batch_encode_packed; it must stay
 * valid until that job's results were returned) and returns at once -- ANX_ELIMIT, nothing submitted, when `depth` jobs are in flight
 * already: a job counts until anx_pipeline_next has returned its results, so the caller takes a result first; three library
 * threads encode, run and download the jobs on separate HIP streams, so the upload + encoding of batch i + 2, the device pipeline of
 * batch i + 1 and the download of batch i overlap; anx_pipeline_next returns the oldest job's ranked rows (compact records, as
 * anx_batch_fetch_compact; release with anx_compact_free) in submission order, or that job's error.  Host-side confusable rescoring
 * is refused by the fetch stage (use the staged calls).  A model with variant lists is served by anx_pipeline_next_via, which also
 * returns the job's `via` array (as anx_batch_fetch_compact_via; it works for every model); anx_pipeline_next has nowhere to put
 * `via` and answers ANX_EINVAL for every job of such a model (the job is taken off the queue).  anx_pipeline_free waits for the jobs
 * in flight and drops their results. */
typedef struct anx_pipeline anx_pipeline;
anx_pipeline *anx_pipeline_new(const anx_model *, int depth /* jobs in flight; <= 0: 6 (three stages, each working on one job with one queued) */);
int anx_pipeline_submit_packed(anx_pipeline *, const char *blob, size_t blob_len, size_t n, const anx_params *);
int anx_pipeline_pending(const anx_pipeline *); /* jobs submitted and not yet returned */
int anx_pipeline_next(anx_pipeline *, anx_topk_record **out_rows, uint32_t **out_offsets, size_t *out_n);
int anx_pipeline_next_via(anx_pipeline *, anx_topk_record **out_rows, uint32_t **out_offsets, uint32_t **out_via, size_t *out_n);
void anx_pipeline_free(anx_pipeline *);
/* every scored pair of the batch (order unspecified within a query) */
int anx_batch_fetch_pairs(const anx_batch *, anx_pair **out_pairs, size_t *out_n);
void anx_pairs_free(anx_pair *);
/* The model's measures for caller-chosen string pairs, computed on the device: for pair i the two strings go through
 * normalize_to_alphabet (src/anahash.rs:50-80) and out[i] receives what the reference's public distance functions return for the
 * two code sequences -- damerau_levenshtein(a, b, 255) (src/distance.rs:101-179: unrestricted, no distance bound),
 * longest_common_substring_length (:181-205), common_prefix_length (:207-218), common_suffix_length (:220-231) -- the
 * equality of char::is_lowercase of the two first characters (src/lib.rs:1367-1377) and the distance score of
 * src/lib.rs:1433-1452 under the model's weights with input_length = the symbols of a.  Every measure is computed whatever its
 * weight (the reference skips those of weight 0, src/lib.rs:1352-1377; their terms are 0 either way), so for a pair that
 * find_variants ranks, `score` is bit for bit the dist_score of that row.  No lexicon entry is involved: the strings need not be in
 * the vocabulary, and nothing limits their anagram or edit distance.
 * out[i] belongs to pair i.  Per-pair status: ANX_EEMPTY when a side is empty, ANX_ELIMIT when a side has more than 255 symbols;
 * the measures and the score of such a pair are 0.  The call itself returns ANX_OK then.
 * Returns ANX_OK for n == 0; ANX_EINVAL for a NULL argument (or a NULL string); ANX_ENOTBUILT before anx_model_build;
 * ANX_ENODEVICE for a model that is not resident on a device; ANX_ELIMIT for more than 4 GB of text (a packed blob, or a chunk
 * of 2^20 pairs).  Calls of any size: the work is done in chunks of at most 2^20 pairs.  Thread-safe like the query entry points;
 * a multi-device model runs the call on its first replica.
 * _packed: a = the first n NUL-terminated spans of blob_a[0, len_a), b likewise; a blob holding fewer strings than n: ANX_EINVAL. */
typedef struct anx_pair_score {
  double score;                          /* src/lib.rs:1443-1452, input_length = symbols of a; 0 when status != ANX_OK */
  uint16_t ld, lcs, prefixlen, suffixlen;
  uint8_t len_a, len_b;                  /* symbols after normalize_to_alphabet */
  uint8_t samecase;
  int8_t status;                         /* ANX_OK, ANX_EEMPTY or ANX_ELIMIT */
  uint32_t _pad;
} anx_pair_score;                        /* 24 bytes */
int anx_score_pairs(const anx_model *, const char *const *a, const char *const *b, size_t n, anx_pair_score *out);
int anx_score_pairs_packed(const anx_model *, const char *blob_a, size_t len_a, const char *blob_b, size_t len_b, size_t n,
                           anx_pair_score *out);
/* The same call with the confusable weight of every pair.  On a model with a confusable list the reference multiplies every ranked
 * row's dist_score by compute_confusable_weight(input, candidate) (src/lib.rs:1656-1663, 1733-1756; early mode :1505-1508, late
 * :1591-1595), so `score` alone is NOT the dist_score of a ranked row there: score * weight[i] (one double multiply) is, in late
 * and in early mode.  weight[i] = the product, in list order, of the weights of the model's confusables that are found_in
 * (src/confusables.rs:47-127) shortest_edit_script(a_i, b_i); both RAW strings are decoded as Unicode scalar values (a byte that
 * starts no complete sequence decodes to itself), nothing is normalised to the alphabet.  It is 1.0 on a model without confusables
 * and for a pair whose record has a status.  out[] is byte for byte what anx_score_pairs writes for the same pairs: `score` stays
 * unweighted.  Screen and edit script run on the device behind the pair kernels, on the text the call uploaded anyway; a pair the
 * device's fixed capacities cannot hold (a side above 64 code points, a very long script) is weighted on the host, that pair alone.
 * Device memory of a weighted call on a model with a list, per caller and chunk, on top of anx_score_pairs': 24 bytes per pair and
 * the script kernel's working set of 371 KB per 64 pairs of the chunk, at most 760 MB (a chunk of 2^17 pairs or more).  A call
 * that finds no room for the working set weights its chunk on the host (same weights; anx_debug_pairs_conf_stats out[3] counts them).
 * Argument checks, chunking, statuses, thread-safety and the choice of replica are those of anx_score_pairs; weight == NULL:
 * ANX_EINVAL. */
int anx_score_pairs_weighted(const anx_model *, const char *const *a, const char *const *b, size_t n, anx_pair_score *out,
                             double *weight);
int anx_score_pairs_weighted_packed(const anx_model *, const char *blob_a, size_t len_a, const char *blob_b, size_t len_b, size_t n,
                                    anx_pair_score *out, double *weight);
/* compute_confusable_weight (src/lib.rs:1733-1756) of two strings on the host: anx_model_confusable_weight with the candidate taken
 * from text instead of the vocabulary.  Needs no device and no anx_model_build.  1.0 on a model without confusables. */
int anx_model_confusable_weight_text(const anx_model *, const char *a_utf8, const char *b_utf8, double *out_weight);
/* Running totals of the weighted calls: out[0] = pairs seen, out[1] = pairs the device screen gave weight 1 without an edit script,
 * out[2] = edit scripts run on the device, out[3] = pairs weighted on the host (beyond the device's capacities, or every scorable
 * pair under ANX_CONFUSABLES=host). */
int anx_debug_pairs_conf_stats(uint64_t out[4]);
/* Scored pairs per input (counts[n], malloc'd, release with anx_counts_free): the number of damerau_levenshtein calls the
 * reference's gather_instances makes for that input (src/lib.rs:1311-1402, one per instance of every anagram class
 * find_nearest_anahashes returned; StopAtExactMatch: of the exact class only when it exists, src/lib.rs:1164-1173).
 * Counted by the scan kernel of a PRODUCTION run -- pairs that fail the DL's length test are only counted there, never
 * materialised -- so this is the per-query check of the production pair list (anx_batch_fetch_pairs re-runs with every
 * pair materialised).  Re-runs the batch. */
int anx_batch_pair_counts(anx_batch *, uint32_t **out_counts);
void anx_counts_free(uint32_t *);
/* write fixed-stride ranked records (stride records per query, batch order) into a DEVICE buffer of
 * n*stride*sizeof(anx_topk_record) bytes (e.g. a torch tensor) -- the payload of the multi-GPU gather */
int anx_batch_export_topk(const anx_batch *, void *device_dst, uint32_t stride, void *stream);
/* the same records without padding, into a DEVICE buffer of `capacity` bytes: uint32 offsets[n+1] in input order
 * (padded to a multiple of 16 bytes), then the records of all inputs back to back.  *used = bytes written (known on
 * the host without a device round trip), also set when the call fails with ANX_ELIMIT because capacity is too small;
 * the multi-GPU gather then moves the used bytes only. */
int anx_batch_export_compact(const anx_batch *, void *device_dst, size_t capacity, void *stream, size_t *used);
/* The final top-k gather of a query-sharded job behind the C ABI (what analiticcl_amd/shard.py does for one rank per GPU with RCCL):
 * the compact export (as anx_batch_export_compact) of EVERY shard of a batch of a multi-device model, in ONE buffer on device
 * dst_device.  Shard g's records start at shard_offsets[g] (shard_offsets[0 .. shards], 256-byte aligned sections; may be NULL);
 * a section = u32 offsets[n_g + 1] padded to 16 bytes, then the 16-byte anx_topk_record rows of the shard's inputs IN THE SHARD'S
 * ORDER (anx_batch_shard_info / anx_batch_shard_inputs map them to the call's input indices).  A shard that lives on dst_device is
 * exported in place; the others are exported on their own device and copied device to device (hipMemcpyPeerAsync: over xGMI where
 * the devices see each other, staged by the runtime otherwise), every shard from its replica's own host thread and stream.  Returns
 * when all sections are in place; *used = bytes needed (also when ANX_ELIMIT says capacity is too small).  The reference's
 * counterpart is the collect() of its rayon fan-out (src/bin/analiticcl.rs:445-448). */
int anx_batch_gather_compact(const anx_batch *, int dst_device, void *device_dst, size_t capacity, size_t *shard_offsets, size_t *used);
/* The three exports with `via`, for EVERY model (the 16-byte anx_topk_record has no room for it, so the via-less exports above lose the
 * `via` of every row of a model with variant lists): one uint32 per row beside the records, the vocabulary id of the variant the row
 * was reached through (anx_result::via), UINT32_MAX = none -- every word of a model without variant lists.  Arguments are checked as by
 * the via-less calls (batch not run / rows rescored on the host: ANX_EINVAL; several shards on export_*: ANX_EINVAL; capacity or stride
 * too small: ANX_ELIMIT), and the offsets and records are byte-equal to what those write for the same batch.
 * anx_batch_export_compact_via: as anx_batch_export_compact, followed by uint32 via[n_rows]:
 *   [u32 offsets[n + 1] padded to 16 bytes][anx_topk_record rows[n_rows]][u32 via[n_rows]], n_rows = offsets[n]; *used counts all three.
 * anx_batch_gather_compact_via: as anx_batch_gather_compact, every 256-byte-aligned shard section in that layout.
 * anx_batch_export_topk_via: as anx_batch_export_topk, plus device_via[n * stride] words: slot (i, k) holds the `via` of record (i, k),
 *   UINT32_MAX for rows without one and for every unused slot (also those of inputs that have no record written at all). */
int anx_batch_export_compact_via(const anx_batch *, void *device_dst, size_t capacity, void *stream, size_t *used);
int anx_batch_gather_compact_via(const anx_batch *, int dst_device, void *device_dst, size_t capacity, size_t *shard_offsets, size_t *used);
int anx_batch_export_topk_via(const anx_batch *, void *device_dst, void *device_via, uint32_t stride, void *stream);
typedef struct anx_batch_stats {
  uint64_t n_queries;
  uint64_t n_pairs;          /* scored (query,candidate) pairs = DL invocations of the reference */
  uint64_t n_class_tests;    /* (query,class) count-vector tests executed by the scan kernel */
  uint64_t n_results;        /* ranked results returned */
  uint64_t n_scan_blocks;    /* query tiles (= waves) of the scan kernels */
  uint64_t n_tests_kind[5];  /* class tests by scan body: [0] v_sad_u8 count vectors, [T] T thermometer bit planes */
  uint64_t n_pair_slots;     /* pair-list slots written (scored pairs + unused chunk tails) */
  uint64_t n_survivors;      /* pairs with score >= score_threshold */
  float ms_scan, ms_group, ms_score, ms_rank, ms_total; /* HIP-event times of the last run (stages incl. read-backs) */
  float ms_scan_kernel;      /* HIP events directly around the k_scan_bits launch (the dominant kernel) */
  uint64_t n_selected;       /* pairs that passed the prefilter and went through the DL kernels */
  float ms_filter_score_kernel; /* HIP events directly around the k_filter_score launch */
  uint64_t n_prefiltered_in_scan; /* scored pairs the scan's fused expansion tested against the band-match bound itself (their
                                   * survivors are the pair-list slots; the others of n_pairs failed the DL's length test or were
                                   * left to k_filter_score) */
  uint64_t n_conf_scripts;   /* ABI 2: ranked rows whose edit script the device-side confusable weighting computed (the other rows
                              * were screened out: no pattern can match them) */
  uint64_t n_adj_tiles;      /* scan tiles that streamed a signature adjacency list (k_scan_adj) instead of probing their ball themselves */
  uint64_t n_adj_records;    /* records (12 bytes each, padding included) those tiles streamed ... */
  uint64_t n_adj_records_first; /* ... and the share of the first tile of every (length, signature) group: what the batch reads at least once */
} anx_batch_stats;
/* counts summed over the shards of the batch, times of the slowest replica.  struct_size = sizeof(anx_batch_stats) as the CALLER
 * was compiled: the library writes at most that many bytes, so a caller built against an older, shorter struct stays in bounds
 * (the struct only ever grows at its end). */
int anx_batch_get_stats(const anx_batch *, anx_batch_stats *, size_t struct_size);
/* The replicas a batch is spread over.  Default split of a multi-replica call (ANX_SHARD_POLICY=length): the inputs are ordered by
 * (byte length, a cheap function of the signature) and cut into cost-balanced pieces, one per replica, so that a replica owns whole
 * (length, signature) groups: full scan tiles on every device (BASELINE configs[3]); a shard then holds n_inputs scattered inputs,
 * *first_input is its smallest index and anx_batch_shard_inputs returns all of them (ascending; valid until the batch is freed).
 * ANX_SHARD_POLICY=range (and calls whose rows are rescored on the host): shard i holds the consecutive inputs [first_input,
 * first_input + n_inputs) and anx_batch_shard_inputs returns NULL.  Either way every fetch returns rows in the call's input order.
 * Any out pointer may be NULL.  anx_batch_export_topk / _compact need a batch with exactly one shard. */
int anx_batch_num_shards(const anx_batch *);
int anx_batch_shard_info(const anx_batch *, int shard, int *device, size_t *first_input, size_t *n_inputs);
int anx_batch_shard_inputs(const anx_batch *, int shard, const uint32_t **indices);
/* Waits for asynchronous exports of the batch (anx_batch_export_topk / _compact on the caller's stream), then releases it. */
void anx_batch_free(anx_batch *);
/* Device scratch (pair lists, survivor rows: several GB per million queries) comes from a per-device pool that keeps freed
 * blocks for the next batch (up to 96 GB, ANX_POOL_CACHE_MB overrides; the reference has no counterpart: its scratch is
 * Vec storage inside find_variants, src/lib.rs:1311-1402).  This hands the cached blocks back to the driver, e.g. before
 * another library needs the memory. */
void anx_device_pool_trim(int device);
/* Joins the host threads the library keeps between calls (the pool search mode's parallel loops run on; a model's replica threads
 * end with anx_model_free) and releases the output blocks anx_matches_free keeps for the next search call (at most
 * ANX_SEARCH_OUT_CACHE_MB, default 1024).  Call it with no library call in flight -- before dlclose() or at the end of main(); the library also
 * does it from a destructor function when it is unloaded.  The next call that needs the pool starts a fresh one.  After fork() the
 * child starts with no pool (a pthread_atfork handler forgets the parent's), so forked workers may use the library independently;
 * device state (models, batches) is NOT usable across fork(): create models in the child. */
void anx_shutdown(void);

/* A/B, test and tuning switches (DESIGN.md section 8 "Switches").  The library reads them ONCE from the environment when it is first
 * used; a variable set later has no effect.  This sets one at run time: name = the variable's name ("ANX_ENCODE", "ANX_SHARD_MIN",
 * ...), value = what the variable would hold (NULL = unset).  None of them changes results.  ANX_EINVAL: unknown name. */
int anx_debug_set_switch(const char *name, const char *value);
/* Measurement hook (bench.py: live kernel times of the configurations that are not the headline one): while enabled, the launches of
 * "k_conf_script" (confusable weighting) and "k_lattice" (search mode's lattice decoding) are bracketed by HIP events on their launch
 * stream.  anx_debug_kernel_timer(1) clears the totals and starts, (0) stops; anx_debug_kernel_time waits for the recorded launches
 * and returns their summed duration and count (ANX_EINVAL: none recorded).  k_scan_bits / k_filter_score are always timed: anx_batch_stats. */
void anx_debug_kernel_timer(int enable);
int anx_debug_kernel_time(const char *name, double *total_ms, uint64_t *launches);
/* Diagnosis of search mode's output path since the library was loaded: out[0] = calls that ran as several parts, out[1] = of those, the
 * calls whose output arrays were written while later parts were still on the device, out[2] = calls that were eligible for that but
 * had to write at the end (an upper bound did not hold), out[3] = 0 (reserved). */
int anx_debug_search_stats(uint64_t out[4]);
/* Where search mode's lattices were decoded since the library was loaded: out[0] = lattices decoded on the device, out[1] = lattices
 * decoded by the host decoder (ANX_LATTICE=host, lattices beyond the device decoder's limits, rule sets outside its flat form),
 * out[2] = of out[0], those of models with context rules (the device scored the rules of every final path), out[3] = parts of calls
 * that completed as one device pass. */
int anx_debug_search_lattice_stats(uint64_t out[4]);
/* Test hook: element `position` of context rule `rule` of the model on (vocab_id, lexindex) -- flat = 0: as the parsed pattern
 * (PatternMatch::matches, what the host decoder evaluates), flat = 1: as the flattened element the device decoder evaluates.  *out = 0 / 1.
 * Host code only.  ANX_EINVAL: no such element; ANX_ELIMIT (flat = 1): the model's rule set is not in the flat form. */
int anx_debug_contextrule_match(const anx_model *model, size_t rule, size_t position, uint64_t vocab_id, uint32_t lexindex, int flat, int *out);
/* The small call: anx_find_variants_batch answers calls of at most 4096 inputs of at most 64 bytes each (models on one or several
 * devices -- a multi-device model runs the whole call on ONE replica, the one with the fewest small calls in flight, so concurrent and
 * consecutive callers spread over the devices; anx_debug_small_replica_stats --, with or without variant lists and confusables -- the latter when they are weighted on the device, i.e. not under ANX_CONFUSABLES=host --
 * and without StopAtExactMatch) through a path of nine launches (thirteen with confusables) and one host wait with preallocated buffers
 * (the reference's own granularity: one string per call, src/lib.rs:972; 1 000 per batch, src/bin/analiticcl.rs:416) instead of the batch
 * pipeline; results are identical.  ANX_SMALL=0 switches it off (A/B).  out[0] = calls it answered since the library was loaded,
 * out[1] = calls it handed to the batch pipeline because a fixed capacity did not hold. */
int anx_debug_small_stats(uint64_t out[2]);
/* Of those, the calls on models with confusables: out[0] = calls the small path answered with the weighting on the device, out[1] = edit
 * scripts run for them, out[2] = calls discarded (counted in anx_debug_small_stats out[1] too) because a row was beyond the fixed
 * working memory of the device weighting (a string of more than 64 code points): the batch pipeline answered with the host weighting. */
int anx_debug_small_conf_stats(uint64_t out[3]);
/* Per replica of the model (anx_model_to_devices order): the calls the small path answered THERE since the model went to its devices.
 * Writes min(cap, replicas) words and returns the number of replicas (negative: error). */
int anx_debug_small_replica_stats(const anx_model *model, uint64_t *out, size_t cap);
/* The length-partitioned split by itself (no device needed): which of n_shards replicas each of the n inputs
 * would go to (out_shard[i] in 0 .. n_shards - 1; see anx_batch_shard_info).  bench.py and the tests use it to build one GPU's share of
 * a larger job (BASELINE configs[3]) on a one-GPU box.  learn_ms (may be NULL): the device times of THOSE shares, measured by the caller
 * one after the other -- fed to the split's per-length cost corrections exactly as a multi-replica run feeds its own shard times, so
 * that the next split is the one a real N-GPU job would see after this call. */
int anx_debug_length_split(const anx_model *, const char *const *utf8, size_t n, const anx_params *, int n_shards, uint8_t *out_shard,
                           const double *learn_ms);
/* Test hooks of the signature adjacency lists (analiticcl_amd/csrc/adjacency.h; no device needed).  anx_debug_signature: the group-sum
 * signature the scan prunes with (one byte per symbol group) of a string.  anx_debug_adjacency builds the lists of the model's lexicon
 * (closure 0..2, budget in bytes) and returns, for each of the n signatures, out_cum[i][8] = {first row of its list in *out_ids, rows
 * of the length sections L-3 .. L+3 cumulated} (all 0xFFFFFFFF: no list) and the lists' entry ids in rows of 64 (padding = number of
 * entries); *out_ids is released with free().  out_stats (may be NULL): uint64[7] {lexicon signatures, closure, lists kept, records, rows, ms, rows an
 * unlimited budget would keep}.
 * tests/test_adjacency_cpu.py compares them with find_nearest_anahashes' candidate set (src/lib.rs:1143-1308) by brute force. */
int anx_debug_signature(const anx_model *, const char *utf8, uint64_t *out_sig);
/* the index's entries (class-major order = the entry ids of the pair list and of the adjacency lists) as vocabulary ids; free() */
int anx_debug_entries(const anx_model *, uint32_t **out_vocab_ids, size_t *n);
int anx_debug_adjacency(const anx_model *, int closure, uint64_t budget_bytes, const uint64_t *sigs, size_t n, uint32_t *out_cum,
                        uint32_t **out_ids, uint64_t *out_stats);
/* The same lists as the model's first replica HOLDS them (built on the device by default, analiticcl_amd/csrc/adjacency.hip): out_cum /
 * out_ids as anx_debug_adjacency (the order of the ids inside a section is the builder's own). */
int anx_debug_adjacency_device(const anx_model *, const uint64_t *sigs, size_t n, uint32_t *out_cum, uint32_t **out_ids);
/* Test hook: the band-match bound the scan's fused filter and k_filter_score apply before damerau_levenshtein (src/distance.rs:101-179)
 * on n (query, candidate) pairs of <= 16 symbols: rows of 16 bytes (alphabet-indexed symbols, the query padded with 0xFE, the
 * candidate with 0xFF), lengths, d <= 3.  form: 0 the scan's (7-bit symbols, wave-uniform d), 1 k_filter_score's (7-bit symbols),
 * 2 the general one.  out_reject[i] = 1: the bound claims damerau_levenshtein(q, c) > d -- tests/test_gpu_switches.py checks that claim
 * against the oracle's DL.  Runs on HIP device `device`. */
int anx_debug_band_bound(int device, const uint8_t *q_rows, const uint8_t *c_rows, const uint8_t *lq, const uint8_t *lc, size_t n,
                         int d, int form, uint8_t *out_reject);
/* Test hook: the exclusive prefix sum (u32) the run and the fetch / export paths use, on HIP device `device`: out[0 .. n] = the prefix
 * sums of in[0 .. n) (out[n] = the total), copy (may be NULL) receives out[0 .. n) through the kernel's second output.
 * tests/test_gpu_prefix_sum.py compares it with numpy.cumsum on both sides of the point where the two-kernel form ends. */
int anx_debug_exclusive_scan(int device, const uint32_t *in, size_t n, uint32_t *out, uint32_t *copy);
/* Test hook: the ranking kernel (k_rank: sort, duplicate removal, crop with its tie rule, cutoff) alone, on HIP device `device`, without
 * a model.  nq queries of counts[q] candidate rows, all rows back to back in the physical order the caller chose: score, entry order,
 * expansion position (< 2^20), vocab, freq (1 everywhere without have_freq), via (NULL: no row has one; UINT32_MAX = none).  maxfreq[q] /
 * qexpand[q]: the query's largest frequency and whether one of its candidates had a variant list (read with any_variants only).
 * seg_cap = 0: every row lies in the candidate row buffer.  seg_cap = C > 0 (only any_variants == 0, positions 0, no via): rows i < C
 * of a query as the per-query segment records plus entry records the hook makes up, rows i >= C in the row buffer, as a run lays them
 * out.  row_cap and overflow are the kernel's early-return inputs (it does nothing when the total exceeds row_cap or overflow != 0); the
 * hook's buffers hold the total whatever row_cap says.  out_count[nq] and out_rows start as 0xFF bytes; out_rows is the whole ranked
 * row buffer, one 24-byte record {uint32 vocab_id, uint32 via, double dist_score, double freq_score} per candidate row: query q's
 * out_count[q] ranked rows start at record counts[0] + .. + counts[q - 1].  The launch is the run's own (same kernel instance choice).
 * tests/test_gpu_rank_rows.py compares them exactly with the tail of the twin's score_and_rank (oracle/twin.py rank_tail). */
int anx_debug_rank_rows(int device, size_t nq, const uint32_t *counts, const uint32_t *maxfreq, const uint32_t *qexpand,
                        const double *score, const uint32_t *order, const uint32_t *position, const uint32_t *vocab,
                        const uint32_t *freq, const uint32_t *via, double cutoff_threshold, uint64_t max_matches, float freq_weight,
                        int have_freq, int any_variants, uint32_t seg_cap, uint32_t row_cap, uint32_t overflow, uint32_t *out_count,
                        void *out_rows);
/* Test hook: the scoring stage (k_filter_score, k_filter_wide, k_score_fast8, k_score_pairs / k_small_lists) alone, on a pair list the
 * caller laid out.  `batch` = anx_batch_encode[_packed] on a resident single-device model (one shard); it need not have run and is left
 * as it is: the stage's buffers are the hook's own.  The pair list has 64 regions of 2^region_shift slots (10 <= region_shift <= 16):
 * fills[64] = the slots of every region, `slots` = those slots back to back, region after region, two words each: (query, entry word) or
 * (UINT32_MAX, anything) = an unused slot of a chunk tail.  The query is the INPUT index (the hook translates to the batch's sorted
 * order); the entry word is the entry id in anx_debug_entries' order, | 1 << 30 = "the scan applied its prefilter" (RAW_PREFILTERED),
 * | 1 << 31 = "exact anagram class" (StopAtExactMatch batches only).
 * seg_cap: 0, or C > 0 = per-query survivor segments of C records (refused where a run of this model and batch would not use them:
 * variant lists, StopAtExactMatch, freq_weight != 0, ANX_SURV_SEG=0).  surv_region_cap / list_cap (1 .. 65536): records per region of the
 * survivor list / entries per region of the three slot lists.  blk: slots per block of k_filter_score, a multiple of 256 up to 4096 (a
 * run: 4096, the small call: 512).  one_launch != 0: the slot-list kernels as the small call's k_small_lists (refused when the model's
 * longest entry leaves k_score_pairs fewer than 256 threads), else as the run's separate launches.  Thresholds, weights, score_threshold
 * and StopAtExactMatch are the batch's; the launch is the run's own function (same kernel instances), with the per-slot outputs on.
 * Everything is validated on the host BEFORE anything is launched, ANX_EINVAL otherwise: query < inputs (and encoded), entry < entries,
 * fills <= 2^region_shift, capacities and blk in range, bit 31 only in a StopAtExactMatch batch, and bit 30 only on a pair inside the
 * scan's contract (analiticcl_amd/csrc/kernels_scan.hpp, the fused prefilter: an alphabet of <= 32 symbols, no StopAtExactMatch, query and
 * entry <= 16 symbols, the query's d <= 3, |lq - lc| <= d, and the band-match bound of anx_debug_band_bound does not reject the pair).
 * Outputs, each starting as 0xFF bytes (also after a refusal; out_surv / out_seg only when the capacity that sizes them is in range,
 * <= 65536 / <= 1024): out_meta[slots] (ld | samecase << 7 | lcs << 8 | prefix << 16 |
 * suffix << 24; ld 0x7F = None; UINT32_MAX = skipped) and out_score[slots] in the order of `slots`; out_qcount[3][inputs] = qsurv,
 * qmaxfreq, qexpand (the last only with variant lists); out_surv[64][surv_region_cap] 16-byte records {uint32 input, uint32 entry,
 * double score}; out_ctr[5][64] = per region the survivor list's counter, the counters of the slot lists of the 8-word kernel, the
 * general kernel and the deferred wide prefilter, and the selected pairs; out_seg[inputs][seg_cap] 16-byte records {double score,
 * uint32 entry, uint32 0} (may be NULL with seg_cap 0); *out_skipped = pairs StopAtExactMatch dropped.
 * tests/test_gpu_score_slots.py compares all of it exactly with the twin's measures and score (oracle/twin.py) on the slot layouts of
 * tests/score_cases.py. */
int anx_debug_score_slots(const anx_model *model, const anx_batch *batch, uint32_t region_shift, const uint32_t *fills,
                          const uint32_t *slots, uint32_t seg_cap, uint32_t surv_region_cap, uint32_t list_cap, uint32_t blk,
                          int one_launch, uint32_t *out_meta, double *out_score, uint32_t *out_qcount, void *out_surv,
                          uint32_t *out_ctr, void *out_seg, uint32_t *out_skipped);
/* Test hook: the scan stage (k_scan_adj, k_scan_bits, k_scan_sad; k_scan_small) alone, on tiles the product's own encoders made, with
 * the whole pair list returned.  Batch form (`batch` != NULL: anx_batch_encode[_packed] on a resident single-device model, one shard; it
 * need not have run and is left as it is; utf8 / n / params are ignored): the batch's tiles through the three launches of a run.  Small form
 * (`batch` == NULL): 1 .. 4096 strings of at most 64 bytes are encoded by the small call's encoder with opts->slots (8, 16 or 32; slots * n
 * <= 32768) tile slots per query and scanned by k_scan_small; want_exact, count_pairs and drop_len == 0 are refused there.  opts: the pair
 * list has 64 regions of 2^region_shift slots (10 .. 25); chunk, chunk_fused, chunk_first (32 .. 1024) are the slots a wave reserves at a
 * time (a run: 256 / 128 / 32, the small call: 64 / 32 / 64); fuse = the band-match bound where a pair is born; twins = queries with equal
 * planes are tested once; drop_len = pairs with |lq - lc| > d are counted, not written; want_exact = bit 31 on pairs of the query's exact
 * class (only with a batch encoded for StopAtExactMatch); count_pairs = per-query counts.  The kernel instance follows from these as in a
 * run.  Everything is validated on the host before anything is launched (ANX_EINVAL).
 * Outputs: out_counts[6] = tiles, of them in the adjacency / other bit-plane / count-vector launch (small form: 0), queries nq, slots
 * written behind the pair list (0 unless the kernel is wrong); *out_tiles = malloc'd [tiles][15] words (struct Tile of
 * analiticcl_amd/csrc/kernels_common.hpp, in launch order; the small form's unused slots have nq = 0; release with anx_counts_free);
 * out_query[4][N], N = the batch's inputs or n, the first nq of each row in the SORTED order the tiles' q0 refers to: input index, kind as
 * the tile tests the query (0 = count vectors, 1 .. 4 planes), len | k << 8 | d << 16 | lowercase << 24, per-query pair count;
 * out_raw[64 << region_shift][2] = the pair list (query in sorted order, entry id | flags; UINT32_MAX = an unused slot of a reservation;
 * 0xFEFEFEFE = never touched); out_rctr[64][32] = the regions' counter blocks (word 0 slots reserved, 1 scored pairs, 2 pairs the fused
 * filter tested, 4 + 2 * kind class tests as uint64, 14 / 15 adjacency rows streamed / by the first tile of a group).
 * tests/test_gpu_scan_door.py compares all of it with the reference set of tests/scan_cases.py. */
typedef struct anx_debug_scan_opts {
  uint32_t region_shift, chunk, chunk_fused, chunk_first;
  int32_t fuse, twins, drop_len, want_exact, count_pairs;
  uint32_t slots;
} anx_debug_scan_opts;
int anx_debug_scan_pairs(const anx_model *model, const anx_batch *batch, const char *const *utf8_inputs, size_t n,
                         const anx_params *params, const anx_debug_scan_opts *opts, uint32_t *out_counts, uint32_t **out_tiles,
                         uint32_t *out_query, uint32_t *out_raw, uint32_t *out_rctr);

/* ---- output of `analiticcl query` --------------------------------------------------
 * The TSV lines / JSON items of output_matches_as_tsv / output_matches_as_json (src/bin/analiticcl.rs:21-187) for n
 * inputs and their ranked rows as anx_find_variants_batch returns them: one malloc'd UTF-8 buffer (not NUL-safe:
 * use *out_len), released with anx_string_free.  JSON items are numbered from first_seqnr (1 = first of the run, which
 * gets no leading comma).  Scores print like Rust's `{}` for f64 (shortest round-trip digits, no exponent). */
int anx_format_query_output(const anx_model *, const char *const *utf8_inputs, size_t n, const anx_result *rows,
                            const size_t *offsets, float freq_weight, int json, int output_lexmatch,
                            uint64_t first_seqnr, char **out, size_t *out_len);
void anx_string_free(char *);

/* ---- confusables --------------------------------------------------------------
 * add_to_confusables / read_confusablelist / set_confusables_before_pruning: src/lib.rs:446-458, :409-443, :157-159.
 * Patterns are sesdiff edit scripts ("-[y]+[i]", "=[c|k]-[y]+[i]", "^...", "...$"; src/confusables.rs:13-44).  With
 * confusables loaded the ranked rows are weighted ON THE DEVICE as part of anx_batch_run (late: after the crop, then re-rank and
 * cutoff, src/lib.rs:1591-1622; or before the crop when set_confusables_before_pruning was called, :1505-1508), so the exports
 * and anx_batch_fetch_compact work as without confusables.  A batch with an input or candidate beyond the device kernel's fixed
 * working memory (64 code points) is redone with the host-side weighting (same results); the exports are refused for such a batch.
 * The edit script restates sesdiff 0.3.1 / dissimilar (diff-match-patch): parity unpinned beyond tests/main.rs:914-1020. */
int anx_model_add_to_confusables(anx_model *, const char *editscript, double weight);
int anx_model_read_confusablelist(anx_model *, const char *path);
void anx_model_set_confusables_before_pruning(anx_model *);
/* shortest_edit_script(source, target, false, false, false) in sesdiff notation, e.g. "=[hu]-[y]+[i]=[s]" */
int anx_edit_script(const char *source, const char *target, char *out, int cap);
/* compute_confusable_weight(input, candidate), src/lib.rs:1733-1756: the product of the weights of the patterns found in the
 * edit script input -> text of the vocabulary item (1.0 if none).  Host only. */
int anx_model_confusable_weight(const anx_model *, const char *input_utf8, uint64_t vocab_id, double *out_weight);

/* ---- search mode: the main caller of the hot path -------------------------------
 * VariantModel::find_all_matches(&self, text, &SearchParameters) -> Vec<Match>, src/lib.rs:1790, for n texts at once.
 * Host side: boundaries / n-gram windows / redundancy filter (src/search.rs:190-336), lattice decoding and bigram-LM
 * rerank (src/lib.rs:2088-2495, 2580-2674) with context rules (below).  Device side: every segment of one
 * n-gram order, over all texts, is ONE anx_find_variants_batch call. */
typedef struct anx_search_params {
  anx_params base;
  uint8_t max_ngram;          /* default 3 */
  uint32_t max_seq;           /* default 250: candidate sequences taken to the rerank stage */
  float lm_weight;            /* default 1.0 */
  float variantmodel_weight;  /* default 3.0 */
  float contextrules_weight;  /* default 1.0 */
  int32_t unicodeoffsets;     /* offsets in code points instead of UTF-8 bytes */
} anx_search_params;
/* Match, src/search.rs:40-68 */
typedef struct anx_match {
  uint64_t begin, end;        /* offset of the matched text in its input text */
  uint32_t n;                 /* tokens (boundaries) spanned */
  int32_t selected;           /* index of the chosen variant, -1 = none (out-of-vocabulary, copied from the input) */
  uint64_t var_begin, var_end; /* its ranked variants: rows [var_begin, var_end) of the row array */
  uint32_t tag_begin, tag_end; /* Match.tag / Match.seqnr: entries [tag_begin, tag_end) of the tag array */
} anx_match;
/* one (tag, sequence number) of a match, assigned by a context rule: src/search.rs:60-66 */
typedef struct anx_match_tag {
  uint16_t tag;   /* index for anx_model_tag_name */
  uint8_t seqnr;  /* position of the match inside the tagged span */
  uint8_t pad_;
} anx_match_tag;
void anx_default_search_params(anx_search_params *);
/* Test hook: search mode's lattice decoder (k_lattice<32|64>, k_ctx_rules, k_lattice_lm and their driver) alone, on lattices the caller
 * laid out, through the product's own lattice_decode / lattice_launch: launch order, pairing, pools and kernel instances are the run's.
 * `model` (resident) gives the LM tables, the n-gram token lists, the lexicon masks and the flat context rules; `params` max_seq (K)
 * and the three rerank weights.  The lattices, stretch after stretch: nstates[s] (without the virtual end state; >= 1); in_off = per
 * stretch nstates + 2 offsets into ITS arcs (entry d = first incoming arc of state d, the virtual end state is state nstates, the last
 * entry is the stretch's arc count); arcs = 3 words each (cost as float bits, source state, symbol | UINT32_MAX = epsilon), per
 * destination in (source state, arc number) order; nsyms[s] and syms = 2 words each (vocab_id, boundary); btok_off = per stretch nstates
 * offsets (nstates - 1 boundaries + 1) into ITS boundary tokens, btok = LM tokens (-1 = not in the vocabulary); best_cost_init[s].  The
 * hook computes the ring (1 + the widest span, end arcs included) as the lattice builder does.  Only the stretches [first, first + count)
 * are decoded (a replica's share).
 * Everything is validated on the host BEFORE anything is launched, ANX_EINVAL otherwise: offsets monotone and in range, state 0 without
 * an incoming arc, every arc's source below its destination and non-decreasing within a state, symbols below nsyms[s], boundary <
 * nstates - 1, vocab_id below the vocabulary size, tokens -1 or a vocabulary id, every cost (and best_cost_init) finite, sign bit clear,
 * at most 1e6 (the merge orders costs by bit pattern), nstates <= 65535 and the nodes of the call ((nstates + 1) * K per stretch) at
 * most 2^24.  States nothing reaches, and an end state nothing reaches, are accepted.
 * Outputs start as 0xFF bytes (also after a refusal): out_n[nst] (UINT32_MAX = handed back; the hook runs no host decoder), out_syms and
 * out_cover (NULL only for a model without rules) with nstates[s] slots per stretch, all stretches of the view back to back.  `dbg` may
 * be NULL; else budget_nodes (0 = the driver's own) cuts the launches and the arrays that are not NULL receive, per launch and before
 * the pools are reused, the device pools over a 0xFF fill: stretch j of the sub-range owns the states [sum of nstates + 1 before it ..)
 * of nodes (K nodes of 3 words (cost bits, parent, symbol) per state), lm (3 words (lp bits, n, prev) per node, LM only), marks ((K + 3
 * & ~3) bytes per state, LM only), cnts (one per state), and ctxval[j * K ..] (rules only); launch_of / width_of / lds_of [count].
 * tests/test_gpu_lattice_door.py compares all of it exactly with oracle/twin.py decode_lattice on the cases of tests/lattice_cases.py. */
typedef struct anx_lattice_debug {
  uint64_t budget_nodes;
  uint32_t *launch_of, *width_of, *lds_of;
  uint32_t *nodes, *lm;
  uint8_t *marks;
  uint16_t *cnts;
  double *ctxval;
  uint32_t lds_limit;   /* out: the device's dynamic LDS limit per block */
  uint32_t n_launches;  /* out */
} anx_lattice_debug;
int anx_debug_lattice_decode(const anx_model *model, const anx_search_params *params, size_t nst, const uint32_t *nstates,
                             const uint32_t *in_off, const uint32_t *arcs, const uint32_t *nsyms, const uint32_t *syms,
                             const uint32_t *btok_off, const int32_t *btok, const float *best_cost_init, size_t first, size_t count,
                             uint32_t *out_n, uint32_t *out_syms, uint32_t *out_cover, anx_lattice_debug *dbg);
/* Test hook: out[i] = the host build of the library's own logarithm (portable_log.hpp) of x[i]: a reference of the rerank computes
 * with the product's bits. */
int anx_debug_portable_log(const double *x, size_t n, double *out);
/* matches of text i are (*out_matches)[(*out_offsets)[i] .. (*out_offsets)[i+1]); out_tags may be NULL (tags are then
 * not reported); release with anx_matches_free */
int anx_find_all_matches_batch(const anx_model *, const char *const *utf8_texts, size_t n, const anx_search_params *,
                               anx_match **out_matches, size_t **out_offsets, anx_result **out_rows, size_t *out_n_rows,
                               anx_match_tag **out_tags);
void anx_matches_free(anx_match *matches, size_t *offsets, anx_result *rows, anx_match_tag *tags);   /* (the two large arrays are kept for the next call: see anx_shutdown) */
/* the text `analiticcl search` prints for the matches of n texts (src/bin/analiticcl.rs:21-187, 600-630): per match the
 * input slice, its offsets, tags, and the variants with the selected one first.  Needs byte offsets (unicodeoffsets
 * = 0).  *n_matches = matches formatted (JSON items are numbered from first_seqnr). */
int anx_format_search_output(const anx_model *, const char *const *utf8_texts, size_t n, const anx_match *matches,
                             const size_t *offsets, const anx_result *rows, const anx_match_tag *tags,
                             float freq_weight, int json, int output_lexmatch, uint64_t first_seqnr, char **out,
                             size_t *out_len);

/* ---- context rules of search mode -----------------------------------------------------------------------------
 * VariantModel::add_contextrule(pattern, score, tag, tagoffset), src/lib.rs:658-765; read_contextrules, :570-656.
 * pattern: ';'-separated expressions -- a vocabulary word, "?" (anything), "^" (in no lexicon), "@lexicon", "!x"
 * (negation), "a|b" (disjunction), "!(a|b)"; src/search.rs:413-459.  score > 1 favours, < 1 penalises a candidate
 * sequence the pattern occurs in (src/lib.rs:2501-2578).  tags / tagoffsets ("begin:length", either may be empty):
 * n_tags strings, n_tagoffsets strings.  Rules are applied to every candidate sequence of the lattice on the host. */
int anx_model_add_contextrule(anx_model *, const char *pattern, float score, const char *const *tags, size_t n_tags,
                              const char *const *tagoffsets, size_t n_tagoffsets);
int anx_model_read_contextrules(anx_model *, const char *path);
size_t anx_model_num_tags(const anx_model *);
const char *anx_model_tag_name(const anx_model *, size_t index); /* NULL when out of range */

/* ---- learn mode -------------------------------------------------------------------------------------
 * VariantModel::learn_variants(inputs, &SearchParameters, strict, auto_build) -> usize, src/lib.rs:1065-1139: every input is queried
 * against the model as it is at the start of the call, the ranked rows are folded into the model (new input strings become
 * TRANSPARENT entries of lexicon index 0 -- never indexed by build() --, frequencies count runs of the same string, (result, input)
 * links: ReferenceFor on the result, first mention wins; VariantOf on the input, appended every time).  *count = rows whose result
 * is not the input itself.  auto_build: build() and the upload to the model's devices again (replicas included).
 * anx_learn_variants: strict mode (find_variants per input); the fold runs on replica 0's device (ANX_LEARN_FOLD=host: on the host).
 * anx_learn_variants_search: non-strict mode (the selected variant of every match of find_all_matches, paired with the matched text).
 * anx_learn_apply_rows: the fold of caller-provided rows (rows[offsets[i] .. offsets[i+1]) of input i) on the host; no build. */
int anx_learn_variants(anx_model *, const char *const *utf8, size_t n, const anx_params *, int auto_build, uint64_t *count);
int anx_learn_variants_search(anx_model *, const char *const *utf8_texts, size_t n, const anx_search_params *, int auto_build,
                              uint64_t *count);
int anx_learn_apply_rows(anx_model *, const char *const *utf8, size_t n, const anx_result *rows, const size_t *offsets, uint64_t *count);
/* an item's variant references (VocabValue::variants, src/types.rs:315-324) in order: kind 0 = ReferenceFor, 1 = VariantOf.  Writes at
 * most cap entries (any output may be NULL); returns how many there are, negative on error. */
int64_t anx_model_variants(const anx_model *, uint64_t vocab_id, uint8_t *kinds, uint64_t *ids, double *scores, size_t cap);
uint32_t anx_model_vocab_type(const anx_model *, uint64_t vocab_id); /* ANX_VOCAB_* bits */
/* the weighted variant list `analiticcl learn` writes to standard output (src/bin/analiticcl.rs:233-269 TSV, 317-365 JSON): malloc'd,
 * release with anx_string_free */
int anx_format_variant_list(const anx_model *, int json, char **out);
/* out[0] device folds, out[1] host folds, out[2] rows folded, out[3] ReferenceFor links added -- since the library was loaded */
int anx_debug_learn_stats(uint64_t out[4]);
/* the last learn call's phases in ms: batch (encode, run, gather), device fold, host fold, host apply, build, upload */
int anx_debug_learn_times(double out[6]);
/* Test hook of the device fold (learn.hip): anx_learn_apply_rows' contract and validation, but the rows are folded ON replica 0's
 * DEVICE, as anx_learn_variants folds a batch's rows: packed into n_sections (>= 1) compact export sections (u32 offsets padded to 16
 * bytes, then 16-byte anx_topk_record rows) -- contiguous input ranges, some empty when n_sections > n, or with by_index index-listed
 * sections that deal the inputs out round-robin --, folded by learn.hip and applied by the host; no build.  Counts as a device fold in
 * anx_debug_learn_stats.  ANX_ENODEVICE without a resident model.
 * The test switch ANX_LEARN_HASH_BITS = 1..63 (anx_debug_set_switch; default 63) narrows the string hash of the fold, so that the
 * collision branches run; results do not depend on it. */
int anx_debug_learn_fold_rows(anx_model *, const char *const *utf8, size_t n, const anx_result *rows, const size_t *offsets, int n_sections,
                              int by_index, uint64_t *count);

/* ---- gold evaluation: where did the correct form end up, and if nowhere, which stage lost it -------------------------------------------
 * For pair i = (inputs[i], gold[i]) and the caller's parameters P, out[i] describes gold[i] against rows_i = exactly what
 * find_variants(inputs[i], P) returns on this model (ranked, variant lists expanded, confusables weighted late or early):
 *   gold_vocab_id  the vocabulary item whose text equals gold[i] byte for byte, UINT32_MAX if none
 *   rank           index of the first row of rows_i with vocab_id == gold_vocab_id, -1 if none.  On a model with variant lists a row
 *                  reached through `via` counts: the row's vocab_id is what is compared
 *   n_results, top_vocab_id   len(rows_i); rows_i[0].vocab_id or UINT32_MAX
 *   gold_score     rank >= 0: that row's dist_score, bit for bit; else the unweighted score anx_score_pairs gives for the pair (0 when
 *                  the pair has a status)
 *   k, d           the input's clamped max_anagram_distance / max_edit_distance (src/lib.rs:972-1027); 0 when the input is empty or
 *                  has more than 255 symbols
 *   ld, status     as anx_score_pairs gives them for (inputs[i], gold[i]): unbounded Damerau-Levenshtein; ANX_OK / ANX_EEMPTY / ANX_ELIMIT
 *   reason         the first ANX_GOLD_* that applies, in the order of the reference's pipeline.  The reasons other than RANKED always
 *                  describe the DIRECT pair (input, gold), also on a model with variant lists.
 * pairs (may be NULL): pairs[i] = byte for byte what anx_score_pairs writes for (inputs[i], gold[i]).
 * The ranked rows come from the staged batch path (never the small call) and stay on the device: every shard is gathered onto replica
 * 0 (anx_batch_gather_compact_via), whose device looks the gold strings up, encodes both sides, runs the pair kernels, searches the
 * rows (k_eval_rows) and classifies (k_eval_classify); 32 bytes per pair come back (56 with pairs).  Chunks of at most 2^20 pairs.
 * Limits: 255 symbols a side (status ANX_ELIMIT beyond); the pass runs on replica 0 alone; holds the learn lock for the call (the
 * vocabulary table is learn mode's).  Returns ANX_OK for n == 0; ANX_EINVAL for a NULL argument or string, and for a model whose
 * confusables are weighted on the host (ANX_CONFUSABLES=host, or a row the device could not weight: the rows exist on the host only);
 * ANX_ENOTBUILT before anx_model_build; ANX_ENODEVICE for a model that is not resident on a device; ANX_ELIMIT as anx_score_pairs.
 * _packed: inputs = the first n NUL-terminated spans of blob_in[0, len_in), gold likewise (as anx_score_pairs_packed). */
enum {
  ANX_GOLD_RANKED = 0,       /* rank >= 0 */
  ANX_GOLD_STATUS = 1,       /* status != ANX_OK */
  ANX_GOLD_NOT_A_RESULT = 2, /* no vocabulary item has that text, or one find_variants never returns: not INDEXED (src/lib.rs:198), or TRANSPARENT */
  ANX_GOLD_EXACT_STOP = 3,   /* P.stop_at_exact_match, the index holds the input's own anagram class and gold is not in it (src/lib.rs:1164-1173) */
  ANX_GOLD_ANAGRAM = 4,      /* gold's anagram class is not among the candidates at k: L1 of the count vectors > k, or no shared symbol */
  ANX_GOLD_EDIT = 5,         /* ld > d: the bounded Damerau-Levenshtein returns None (src/distance.rs:109-130) */
  ANX_GOLD_THRESHOLD = 6,    /* the unweighted pair score is below P.score_threshold (src/lib.rs:1475) */
  ANX_GOLD_CROPPED = 7       /* everything else: cutoff_threshold, max_matches, tie rules, the re-rank after confusable weights */
};
typedef struct anx_gold_eval {
  uint32_t gold_vocab_id;
  int32_t rank;
  uint32_t n_results;
  uint32_t top_vocab_id;
  double gold_score;
  uint16_t ld;
  uint8_t k, d;
  int8_t status;
  uint8_t reason;
  uint16_t _pad;
} anx_gold_eval; /* 32 bytes */
#ifdef __cplusplus
static_assert(sizeof(anx_gold_eval) == 32, "anx_gold_eval is 32 bytes");
#else
_Static_assert(sizeof(anx_gold_eval) == 32, "anx_gold_eval is 32 bytes");
#endif
int anx_evaluate_gold(anx_model *, const char *const *inputs, const char *const *gold, size_t n, const anx_params *, anx_gold_eval *out,
                      anx_pair_score *pairs);
int anx_evaluate_gold_packed(anx_model *, const char *blob_in, size_t len_in, const char *blob_gold, size_t len_gold, size_t n,
                             const anx_params *, anx_gold_eval *out, anx_pair_score *pairs);
/* Test hook: the same contract with a caller-chosen chunk size (1 .. 2^20 pairs), so that chunk seams are reached with small calls. */
int anx_debug_evaluate_gold_chunk(anx_model *, const char *const *inputs, const char *const *gold, size_t n, const anx_params *,
                                  anx_gold_eval *out, anx_pair_score *pairs, size_t chunk);

/* ---- parameter sweep: several parameter sets over the same gold pairs in one pass, the summary reduced on the device -------------------
 * For every set s of sets[0 .. n_sets), summaries[s] holds the integers one gets by reducing the records that
 * anx_evaluate_gold(model, inputs, gold, n, &sets[s], ...) writes for the same pairs -- every field equal, whatever the order in which
 * the device's blocks arrive (the summary is integers only; nothing is summed in floating point):
 *   n, gold_known   pairs; pairs whose gold_vocab_id != UINT32_MAX
 *   reasons[r]      pairs whose reason is the ANX_GOLD_* value r
 *   rank_hist[b]    ranked pairs by rank; the last bin holds every rank >= ANX_GOLD_RANK_BINS - 1
 *   rr_fixed        sum over ranked pairs of floor(2^32 / (rank + 1)): the reciprocal ranks as 32.32 fixed point
 *   n_results       sum of the records' n_results: how long the lists get under this set
 *   gained_at_1, lost_at_1   pairs whose gold is at rank 0 under this set but not under sets[0], and the reverse (both 0 for sets[0])
 * The host derives accuracy@1 = rank_hist[0] / n, ranked share = reasons[ANX_GOLD_RANKED] / n and mrr = rr_fixed / 2^32 / n.
 * out (may be NULL): [n_sets][n], set-major; out[s * n .. (s + 1) * n) is byte for byte what anx_evaluate_gold writes under sets[s].
 * pairs (may be NULL): [n], byte for byte what anx_score_pairs writes; it does not depend on the set.
 * Per chunk of at most 2^20 pairs the work that does not depend on the set runs once and stays on replica 0's device (one upload of the
 * 2 n strings, the encoder, the pair kernels, the vocabulary lookup of the gold strings, the vocabulary flags); per set the inputs go
 * through the staged batch path with that set, the rows are gathered onto replica 0 as anx_evaluate_gold gathers them, and
 * k_sweep_sections / k_sweep_rows / k_sweep_classify find the ranks, classify with the set's clamped k / d per input and reduce.  With
 * out == NULL the pass downloads 624 bytes per set and chunk; the summaries of a call's chunks are added up.
 * Errors and limits are anx_evaluate_gold's (the learn lock is held for the call; confusables weighted on the host are refused), and:
 * ANX_EINVAL for n_sets == 0, n_sets > ANX_SWEEP_MAX_SETS, sets == NULL or summaries == NULL; n == 0 zeroes the summaries and returns
 * ANX_OK without a build or a device.  The weights are the model's: a sweep over weights is anx_evaluate_sweep_weights (below); one over
 * confusable lists or variant lists is not built.  _packed: the blobs as anx_evaluate_gold_packed. */
#define ANX_SWEEP_MAX_SETS 256
#define ANX_GOLD_RANK_BINS 64
typedef struct anx_gold_summary {
  uint64_t n;
  uint64_t gold_known;
  uint64_t reasons[8];
  uint64_t rank_hist[ANX_GOLD_RANK_BINS];
  uint64_t rr_fixed;
  uint64_t n_results;
  uint64_t gained_at_1, lost_at_1;
} anx_gold_summary; /* 624 bytes */
#ifdef __cplusplus
static_assert(sizeof(anx_gold_summary) == 624, "anx_gold_summary is 624 bytes");
#else
_Static_assert(sizeof(anx_gold_summary) == 624, "anx_gold_summary is 624 bytes");
#endif
int anx_evaluate_sweep(anx_model *, const char *const *inputs, const char *const *gold, size_t n, const anx_params *sets, size_t n_sets,
                       anx_gold_summary *summaries, anx_gold_eval *out, anx_pair_score *pairs);
int anx_evaluate_sweep_packed(anx_model *, const char *blob_in, size_t len_in, const char *blob_gold, size_t len_gold, size_t n,
                              const anx_params *sets, size_t n_sets, anx_gold_summary *summaries, anx_gold_eval *out, anx_pair_score *pairs);
/* Test hook: the pointer form with a caller-chosen chunk size (1 .. 2^20 pairs). */
int anx_debug_evaluate_sweep_chunk(anx_model *, const char *const *inputs, const char *const *gold, size_t n, const anx_params *sets,
                                   size_t n_sets, anx_gold_summary *summaries, anx_gold_eval *out, anx_pair_score *pairs, size_t chunk);
/* Running totals of the sweep calls since process start, the first min(n, 7) of: [0] calls, [1] chunks, [2] sets run (per chunk),
 * [3] pair-side passes (upload, encoder, pair kernels: one per chunk), [4] gold lookups (one per chunk), [5] batch runs, [6] bytes the
 * sweep's own pass downloaded (624 per set and chunk, + 32 per pair and set with `out`, + 24 per pair with `pairs`; the batch path's
 * control reads inside anx_batch_run are not part of it). */
int anx_debug_sweep_stats(uint64_t *out, int n);

/* ---- weight sweep: sets that also differ in the five score weights, without a model, a build or a batch run per set -------------------
 * Set s is (sets[s], weights[s]).  summaries[s] holds the integers one gets by reducing the records that
 * anx_evaluate_gold(model_w, inputs, gold, n, &sets[s], ...) writes, model_w being a model with the same alphabet, lexicons and flags
 * created with weights[s] instead of its own weights; out (may be NULL; [n_sets][n], set-major) is byte for byte those records,
 * gold_score included: for rank >= 0 the row's dist_score under weights[s], else the direct pair's score under weights[s], recomputed
 * from the pair's measures.  gained_at_1 / lost_at_1 compare with set 0, as in anx_evaluate_sweep.  The model's own weights play no part
 * in any result.  There is no `pairs` output: its score would be the model's.
 * How: the candidates of an input are fixed by k, d and stop_at_exact_match, their five measures are integers and max_freq is taken
 * before the score threshold, so the sets are grouped by (max_anagram_distance, max_edit_distance, stop_at_exact_match != 0), groups in
 * order of first appearance, and per chunk and group ONE base run of the batch path yields every instance with ld <= d (max_matches 0, no
 * cutoff, no frequency weight, a score threshold of minus infinity) with its measures (the kernels of anx_batch_fetch_measures) on
 * replica 0.  Per set reweigh.hip re-scores the rows under the set's weights, applies the set's score threshold, ranks them with the
 * batch path's own k_rank under the set's max_matches / cutoff_threshold / freq_weight, classifies and reduces: no batch run per set,
 * and a download of 624 bytes per set and chunk (+ 32 per pair with out).
 * Errors and limits: everything anx_evaluate_sweep refuses; ANX_EINVAL for NULL sets / weights / summaries, n_sets == 0 or
 * > ANX_SWEEP_MAX_SETS, a weight that is not finite or below 0, a set whose five weights sum to 0, and for a model whose own weights are
 * not finite or sum to 0 (its base run would score NaN); n == 0 zeroes the summaries and returns ANX_OK without a build or a device.
 * PLAIN MODELS ONLY: a model with a variant list or a confusable list gets ANX_EINVAL (both multiply or expand the score after the
 * weights).  Models with frequencies are served, and a freq_weight per set.  The learn lock is held and the device pass runs on replica 0,
 * as for anx_evaluate_gold.  More than 2^31 base rows in one chunk and group: ANX_ELIMIT. */
int anx_evaluate_sweep_weights(anx_model *, const char *const *inputs, const char *const *gold, size_t n, const anx_params *sets,
                               const anx_weights *weights, size_t n_sets, anx_gold_summary *summaries, anx_gold_eval *out);
int anx_evaluate_sweep_weights_packed(anx_model *, const char *blob_in, size_t len_in, const char *blob_gold, size_t len_gold, size_t n,
                                      const anx_params *sets, const anx_weights *weights, size_t n_sets, anx_gold_summary *summaries,
                                      anx_gold_eval *out);
/* Test hook: the pointer form with a caller-chosen chunk size (1 .. 2^20 pairs). */
int anx_debug_evaluate_sweep_weights_chunk(anx_model *, const char *const *inputs, const char *const *gold, size_t n, const anx_params *sets,
                                           const anx_weights *weights, size_t n_sets, anx_gold_summary *summaries, anx_gold_eval *out,
                                           size_t chunk);
/* Running totals of the weight-sweep calls since process start, the first min(n, 8) of: [0] calls, [1] chunks, [2] groups (base runs per
 * chunk), [3] sets re-ranked (per chunk), [4] pair-side passes, [5] batch runs, [6] base rows re-scored (rows x sets), [7] bytes the
 * pass downloaded (624 per set and chunk, + 32 per pair and set with `out`). */
int anx_debug_weight_sweep_stats(uint64_t *out, int n);

/* ---- confusable sweep: candidate confusable patterns with one weight per pattern and set, without a model or a batch run per set -------
 * Set s is (sets[s], weights[s * n_patterns .. + n_patterns), early[s]).  summaries[s], and with out the records ([n_sets][n], set-major),
 * equal field by field what anx_evaluate_gold(model_s, inputs, gold, n, &sets[s], ...) writes, model_s being a model with the same
 * alphabet, lexicons and score weights whose confusable list is patterns[j] with weight weights[s][j], added in order with
 * anx_model_add_to_confusables, and anx_model_set_confusables_before_pruning iff early[s] (early == NULL: every set is late).  A weight
 * of exactly 1.0 switches a pattern off (x * 1.0 == x).  gained_at_1 / lost_at_1 compare with set 0, so a set 0 of all ones is the plain
 * baseline.  The model's score weights are the model's: this call does not sweep them.  There is no `pairs` output.
 * How: the candidates of an input, their measures and their unweighted scores do not depend on the list, and whether pattern j is found
 * in the edit script of (input, candidate) depends on the two texts alone; the weights enter as a product over the matching patterns in
 * list order.  So per chunk and group of (max_anagram_distance, max_edit_distance, stop_at_exact_match != 0) ONE base run yields every
 * instance (as for anx_evaluate_sweep_weights), csweep.hip scores them once and computes ONE 64-bit match mask per instance (a screen on
 * presence bits, then one edit script per row that a pattern can match; a row the device's lane memory cannot hold -- a side above 64
 * code points -- is done by the host), and per set applies the set's weights to the masks: early to the kept rows before k_rank, late
 * to the cropped list before the re-sort and the cutoff the batch path runs.  No batch run and no edit script per set; a download of
 * 624 bytes per set and chunk (+ 32 per pair with out).  Under ANX_CONFUSABLES=host every mask is computed on the host.
 * Errors, each ANX_EINVAL before the device is asked for: NULL sets / weights / patterns / summaries; n_patterns outside 1 .. 64
 * (ANX_SWEEP_CONF_MAX_PATTERNS); n_sets outside 1 .. ANX_SWEEP_MAX_SETS; a pattern the list parser rejects (the message names its
 * index); a weight that is not finite or not above 0; a model with a variant list; a model with a confusable list of its own (the
 * candidates would multiply on top of it: not built); a model whose own score weights are not finite or sum to 0.  n == 0 zeroes the
 * summaries and returns ANX_OK without a build or a device.  Otherwise anx_evaluate_gold's limits: replica 0, the learn lock, and
 * ANX_ELIMIT for more than 2^31 base rows in one chunk and group. */
#define ANX_SWEEP_CONF_MAX_PATTERNS 64
int anx_evaluate_sweep_confusables(anx_model *, const char *const *inputs, const char *const *gold, size_t n, const char *const *patterns,
                                   size_t n_patterns, const anx_params *sets, const double *weights /* [n_sets][n_patterns] */,
                                   const uint8_t *early /* [n_sets], may be NULL = all late */, size_t n_sets, anx_gold_summary *summaries,
                                   anx_gold_eval *out /* [n_sets][n] or NULL */);
int anx_evaluate_sweep_confusables_packed(anx_model *, const char *blob_in, size_t len_in, const char *blob_gold, size_t len_gold, size_t n,
                                          const char *const *patterns, size_t n_patterns, const anx_params *sets, const double *weights,
                                          const uint8_t *early, size_t n_sets, anx_gold_summary *summaries, anx_gold_eval *out);
/* Test hook: the pointer form with a caller-chosen chunk size (1 .. 2^20 pairs). */
int anx_debug_evaluate_sweep_confusables_chunk(anx_model *, const char *const *inputs, const char *const *gold, size_t n,
                                               const char *const *patterns, size_t n_patterns, const anx_params *sets, const double *weights,
                                               const uint8_t *early, size_t n_sets, anx_gold_summary *summaries, anx_gold_eval *out,
                                               size_t chunk);
/* Test hook: the mask pass alone.  The base rows of `inputs` under group's max_anagram_distance / max_edit_distance / stop_at_exact_match,
 * in the order the pass holds them: pair[r] = input index, vocab[r] = vocabulary id, mask[r] bit j = patterns[j] is found in the edit
 * script of (inputs[pair[r]], vocabulary item vocab[r]).  n <= 2^20.  The three arrays are malloc'ed: free() each. */
int anx_debug_sweep_conf_masks(anx_model *, const char *const *inputs, size_t n, const char *const *patterns, size_t n_patterns,
                               const anx_params *group, uint32_t **pair, uint32_t **vocab, uint64_t **mask, size_t *rows);
/* The host body of the mask kernel for one pair of texts (no model, no device): bit j of *mask = patterns[j] is found in the edit script
 * of (a -> b). */
int anx_debug_conf_mask_text(const char *const *patterns, size_t n_patterns, const char *a, const char *b, uint64_t *mask);
/* Running totals of the confusable-sweep calls since process start, the first min(n, 11) of: [0] calls, [1] chunks, [2] groups,
 * [3] sets, [4] pair-side passes, [5] batch runs (one per chunk and group), [6] base rows, [7] rows listed for an edit script (counted
 * when a group's mask pass ends: a set adds none), [8] of those, rows the host computed because the device could not hold them,
 * [9] rows the host computed under ANX_CONFUSABLES=host, [10] bytes the sets downloaded. */
int anx_debug_conf_sweep_stats(uint64_t *out, int n);

/* ---- confusable fit: a greedy coordinate ascent over the weights of candidate patterns, on the device (late mode only) ---------------
 * anx_fit_counts for a weight assignment w holds three fields of the anx_gold_summary that anx_evaluate_sweep_confusables returns for the
 * set (params, w, late) over the same pairs: at1 == rank_hist[0], ranked == reasons[ANX_GOLD_RANKED], rr_fixed == rr_fixed.
 * A round: every (pattern j, grid index g) with grid[g] != cur[j] is a trial "cur with cur[j] = grid[g]".  The key of a trial is
 * (at1, rr_fixed) under ANX_FIT_ACC1 and (rr_fixed, at1) under ANX_FIT_MRR, compared lexicographically as uint64; the best trial has the
 * largest key, ties go to the smallest j, then the smallest g.  It is accepted iff its key is greater than the current key and its
 * first component exceeds the current one by at least min_gain (min_gain == 0: any lexicographic improvement).  On acceptance
 * cur[j] = grid[g] and the round is appended to rounds.  The fit ends when no trial is accepted (stop = 0) or when max_rounds rounds
 * were accepted (stop = 1).  A pattern may be revisited; a grid holding 1.0 can switch a pattern off again.
 * weights_out: the final cur, every value start[j] or a grid value bit for bit.  trials (may be NULL): trials[r][j][g] = the counts of
 * every trial of evaluated round r < n_trial_rounds, a skipped trial (grid[g] == cur[j]) holding the current counts.  result->start /
 * final: the counts under the start weights and under weights_out.
 * How: in late mode the cropped list of an input does not depend on the list's weights (src/lib.rs:1535-1622: crop, then weights,
 * stable re-sort, cutoff), so per chunk the base run, the masks and the unweighted late ranking of the confusable sweep run ONCE, and
 * what stays resident is 24 bytes per ranked slot of the pairs whose gold is in the cropped list and 12 bytes per pair (fit.hip
 * k_fit_gold / k_fit_state).  A round is one launch of k_fit_trials per chunk -- every trial of every pair, gold's place found by
 * counting, no k_rank, no classification -- and one download of at most 26 KB.
 * Errors, each before the device is asked for: ANX_EINVAL for NULL arguments, n_patterns outside 1 .. 64, a pattern the list parser
 * rejects, n_grid outside 1 .. ANX_FIT_MAX_GRID, max_rounds outside 1 .. ANX_FIT_MAX_ROUNDS, an unknown objective, a grid or start weight
 * that is not finite or not above 0, and what anx_evaluate_sweep_confusables refuses of a model (a variant list, a confusable list of its
 * own, score weights that are not finite or sum to 0), a model with anx_model_set_confusables_before_pruning, confusables weighted on the
 * host; ANX_ENOTBUILT / ANX_ENODEVICE as the sweep; ANX_ELIMIT above 2^24 pairs per call (16 chunks of resident state: a stated limit) and
 * the sweep's other limits.  n == 0: ANX_OK, zero rounds, zero counts, weights_out = start, no build and no device.  The learn lock is
 * held and the pass runs on replica 0.  _packed: the blobs as anx_evaluate_sweep_confusables_packed. */
#define ANX_FIT_MAX_GRID 16
#define ANX_FIT_MAX_ROUNDS 256
#define ANX_FIT_MAX_PAIRS ((size_t)1 << 24)
enum { ANX_FIT_ACC1 = 0, ANX_FIT_MRR = 1 };
typedef struct anx_fit_counts { uint64_t at1, ranked, rr_fixed; } anx_fit_counts; /* 24 bytes */
typedef struct anx_fit_params {
  const double *grid; /* [n_grid] candidate weights, each finite and > 0; 1.0 = switch the pattern off */
  uint32_t n_grid;    /* 1 .. ANX_FIT_MAX_GRID */
  uint32_t _pad;
  const double *start; /* NULL (all 1.0) or [n_patterns], finite and > 0 */
  uint32_t objective;  /* ANX_FIT_ACC1 or ANX_FIT_MRR */
  uint32_t max_rounds; /* 1 .. ANX_FIT_MAX_ROUNDS */
  uint64_t min_gain;   /* in units of the key's first component (ANX_FIT_MRR: 32.32 fixed point) */
} anx_fit_params;
typedef struct anx_fit_round { uint32_t pattern, grid_index; double weight; anx_fit_counts counts; } anx_fit_round; /* 40 bytes */
typedef struct anx_fit_result { uint32_t n_rounds, n_trial_rounds, stop, _pad; anx_fit_counts start, final; } anx_fit_result; /* 64 bytes */
#ifdef __cplusplus
static_assert(sizeof(anx_fit_counts) == 24 && sizeof(anx_fit_round) == 40 && sizeof(anx_fit_result) == 64, "the fit's records");
#else
_Static_assert(sizeof(anx_fit_counts) == 24 && sizeof(anx_fit_round) == 40 && sizeof(anx_fit_result) == 64, "the fit's records");
#endif
int anx_fit_confusable_weights(anx_model *, const char *const *inputs, const char *const *gold, size_t n, const char *const *patterns,
                               size_t n_patterns, const anx_params *, const anx_fit_params *, double *weights_out /* [n_patterns] */,
                               anx_fit_round *rounds /* [max_rounds] */, anx_fit_counts *trials /* NULL or [max_rounds][n_patterns][n_grid] */,
                               anx_fit_result *);
int anx_fit_confusable_weights_packed(anx_model *, const char *blob_in, size_t len_in, const char *blob_gold, size_t len_gold, size_t n,
                                      const char *const *patterns, size_t n_patterns, const anx_params *, const anx_fit_params *,
                                      double *weights_out, anx_fit_round *rounds, anx_fit_counts *trials, anx_fit_result *);
/* Test hook: the pointer form with a caller-chosen chunk size (1 .. 2^20 pairs). */
int anx_debug_fit_confusable_weights_chunk(anx_model *, const char *const *inputs, const char *const *gold, size_t n,
                                           const char *const *patterns, size_t n_patterns, const anx_params *, const anx_fit_params *,
                                           double *weights_out, anx_fit_round *rounds, anx_fit_counts *trials, anx_fit_result *, size_t chunk);
/* The selection of a round alone (host only): trials[n_patterns][n_grid], cur[n_patterns], the current counts -> the accepted trial in
 * *pattern / *grid_index, or -1 / -1 when none is accepted.  A trial with grid[g] == cur[j] is never chosen. */
int anx_debug_fit_select(const anx_fit_counts *trials, const double *cur, size_t n_patterns, const double *grid, size_t n_grid,
                         const anx_fit_counts *cur_counts, uint32_t objective, uint64_t min_gain, int32_t *pattern, int32_t *grid_index);
/* Running totals of the fit calls since process start, the first min(n, 7) of: [0] calls, [1] chunks, [2] rounds evaluated,
 * [3] launches of k_fit_trials, [4] pairs in the state (gold in the cropped list), [5] slots in the state, [6] bytes downloaded. */
int anx_debug_fit_stats(uint64_t *out, int n);

/* ---- anx_mine_confusables: confusable patterns from (observed, correct) string pairs ---------------------------------------------------
 * For every pair (a[i], b[i]) the change sites of shortest_edit_script(a[i], b[i]) -- a site is a maximal run of consecutive non-`=`
 * instructions -- and the table of distinct sites in confusable-list notation with their counts: what a confusable list
 * (anx_model_read_confusablelist; src/confusables.rs) is written from.  Both strings are decoded as anx_model_confusable_weight_text
 * decodes them (malformed UTF-8: one byte, one character); nothing is normalised.
 * The text of a site under (context c, anchors): `^` if anchors and the site is the script's first instruction; `=[` + the last c code
 * points of the preceding identity (fewer if it is shorter) + `]` if c > 0 and there is one; the site's instructions in sesdiff notation;
 * `=[` + the first c code points of the following identity + `]` likewise; `$` if anchors and the site is the script's last instruction.
 * The table has one row per distinct text: sites = how many sites have it, count = the sum of the pairs' counts over those sites
 * (count[] == NULL: 1 per pair; two equal sites of one pair count twice), ordered by count descending, sites descending, text bytes
 * ascending.  A text with `[`, `]` or `|` among its characters is flagged ANX_MINE_UNREPRESENTABLE: the list parser could not read it.
 * The site list holds every pair's sites from left to right, pair i's at site[site_off[i] .. site_off[i + 1]).
 * The scripts, the sites' keys and the histogram are computed on the model's first replica, in chunks of at most 2^20 pairs; the host
 * builds the texts of the distinct sites, scripts the pairs the device hands back (a side above 64 code points, a script its working
 * memory cannot hold) and merges the chunks' tables by text.  ANX_MINE=host (anx_debug_set_switch): every pair on the host -- then the
 * call needs neither anx_model_build nor a device.  ANX_EINVAL: NULL argument, context > 8; ANX_ENOTBUILT / ANX_ENODEVICE as
 * anx_score_pairs; ANX_ELIMIT: 2^32 pairs or more, or a packed blob of 4 GB or more.  Thread-safe; each call has its own stream. */
typedef struct anx_mine_params {
  uint32_t context;  /* 0 .. 8 code points of the neighbouring identities */
  uint32_t anchors;  /* != 0: `^` / `$` */
  uint32_t no_sites; /* != 0: the site list is left out (not downloaded): site == site_off == NULL, n_sites still counts them */
  uint32_t _reserved;
} anx_mine_params;
enum { ANX_MINE_SITE_FIRST = 1, ANX_MINE_SITE_LAST = 2 }; /* anx_mine_site.flags: the site begins / ends the script */
enum { ANX_MINE_UNREPRESENTABLE = 1 };                    /* anx_mine_result.flags[] */
typedef struct anx_mine_site {
  uint32_t pair;                       /* index into a[] / b[] */
  uint32_t a_pos, a_len, b_pos, b_len; /* code points: a[a_pos, a_pos + a_len) is deleted, b[b_pos, b_pos + b_len) inserted */
  uint32_t pattern;                    /* row of the table */
  uint32_t flags;
  uint32_t _pad;
} anx_mine_site; /* 32 bytes */
typedef struct anx_mine_result {
  size_t n_patterns;
  const char *text;         /* the texts back to back, UTF-8 */
  const uint64_t *text_off; /* [n_patterns + 1]: row r = text[text_off[r] .. text_off[r + 1]) */
  const uint64_t *count;    /* [n_patterns] */
  const uint64_t *sites;    /* [n_patterns] */
  const uint32_t *flags;    /* [n_patterns] */
  size_t n_pairs, n_sites;
  const uint64_t *site_off; /* [n_pairs + 1], or NULL */
  const anx_mine_site *site; /* [n_sites], or NULL */
} anx_mine_result;
void anx_default_mine_params(anx_mine_params *out);
int anx_mine_confusables(const anx_model *, const char *const *a, const char *const *b, const uint32_t *count, size_t n,
                         const anx_mine_params *, anx_mine_result **out);
int anx_mine_confusables_packed(const anx_model *, const char *blob_a, size_t len_a, const char *blob_b, size_t len_b,
                                const uint32_t *count, size_t n, const anx_mine_params *, anx_mine_result **out);
void anx_mine_result_free(anx_mine_result *);
/* The rows with count >= min_count and no ANX_MINE_UNREPRESENTABLE flag as `pattern<TAB>weight` lines, in table order: a file
 * anx_model_read_confusablelist reads.  *text: malloc'd (anx_string_free). */
int anx_format_confusable_list(const anx_mine_result *, double weight, uint64_t min_count, char **text);
/* Running totals of the mine calls: [0] pairs scripted on the device, [1] pairs scripted on the host, [2] sites, [3] distinct patterns
 * (summed over calls), [4] hash runs that held more than one text, [5] pairs handed to the host because their script had a site that is
 * not -[..], +[..] or -[..]+[..], [6] bytes uploaded, [7] bytes downloaded. */
int anx_debug_mine_stats(uint64_t out[8]);
/* Test hook: pairs per chunk of the calls that follow (1 .. 2^20; 0: the default, 2^20). */
int anx_debug_mine_chunk(size_t chunk);

#ifdef __cplusplus
}
#endif
#endif
