"""The expected anx_gold_eval record of a pair (input, gold), from the oracle side alone (helper of test_evaluate_cpu.py and
test_gpu_evaluate.py; nothing here comes from the product).

The ranked rows are the C oracle's find_variants (oracle/cwrap.py).  The measures and reasons are the twin's own stages (oracle/twin.py):
clamp_threshold for k / d, find_nearest_anahashes for ANAGRAM / EXACT_STOP, damerau_levenshtein(., ., d) for EDIT, the dist_score
score_and_rank gives the direct pair for THRESHOLD.  On the full-size lexicons the twin's find_nearest_anahashes (Python big integers
against every class of seven charcount buckets) takes seconds per input, so `Side` may take the anagram stage from the C oracle's
find_nearest instead -- the same function ported line by line; test_evaluate_cpu.py holds the two against each other on the hand-made
model.

The record's rules (include/anx.h): reasons are tested in the order of the reference's pipeline, and apart from RANKED they
describe the DIRECT pair also on a model with variant lists."""
import random

from oracle import twin as T

REASONS = ("RANKED", "STATUS", "NOT_A_RESULT", "EXACT_STOP", "ANAGRAM", "EDIT", "THRESHOLD", "CROPPED")
RANKED, STATUS, NOT_A_RESULT, EXACT_STOP, ANAGRAM, EDIT, THRESHOLD, CROPPED = range(8)
OK, ELIMIT, EEMPTY = 0, -5, -6
NONE = 0xFFFFFFFF
MAX_ANAGRAM_DISTANCE, MAX_EDIT_DISTANCE = T.MAX_ANAGRAM_DISTANCE, T.MAX_EDIT_DISTANCE
FIELDS = ("gold_vocab_id", "rank", "n_results", "top_vocab_id", "gold_score", "ld", "k", "d", "status", "reason")


class Side:
    """What the helper needs to know of the model, all of it from the oracle side.
    alphabet / weights: the twin's; encoder: text -> vocabulary id; flags(vid) -> (indexed, transparent);
    rows(text, P) -> [(vocab_id, dist_score, freq_score, ...)]: the C oracle's ranked rows;
    nearest(text, k, stop) -> the anagram values find_nearest_anahashes returns; has_class(text): the index holds the text's own class."""

    def __init__(self, alphabet, weights, encoder, flags, rows, nearest, has_class):
        self.alphabet, self.weights, self.encoder, self.flags = alphabet, weights, encoder, flags
        self.rows, self.nearest, self.has_class = rows, nearest, has_class


def twin_side(tw, rows):
    """Every stage from the twin model `tw` (built); rows from the caller (the C oracle holding the same entries)."""
    return Side(tw.alphabet, tw.weights, tw.encoder, lambda v: (tw.decoder[v].indexed, tw.decoder[v].transparent), rows,
                lambda text, k, stop: tw.find_nearest_anahashes(T.anahash(text, tw.alphabet), k, stop),
                lambda text: bool(tw.index.get(T.anahash(text, tw.alphabet), ([], 0))[0]))


def oracle_side(o, alphabet, weights, encoder, flags, params_of):
    """The anagram stage and the rows from the C oracle `o`; params_of(P) -> its parameter struct."""
    return Side(alphabet, weights, encoder, flags, lambda text, P: o.find_variants_via(text, params_of(P)),
                lambda text, k, stop: o.find_nearest(text, k, stop), lambda text: len(o.anagram_instances(text)) > 0)


def pair_measures(side, a, g):
    """(status, ld, score) of the direct pair as anx_score_pairs defines them: the unbounded Damerau-Levenshtein and the dist_score
    score_and_rank computes for an instance with these distances (every measure computed, input_length = the symbols of a)."""
    if not a or not g:
        return EEMPTY, 0, 0.0
    na, ng = T.normalize_to_alphabet(a, side.alphabet), T.normalize_to_alphabet(g, side.alphabet)
    if len(na) > 255 or len(ng) > 255:
        return ELIMIT, 0, 0.0
    scorer = T.VariantModel(side.alphabet, side.weights)   # a model of the gold string alone: its stages applied to the direct pair
    vid = scorer.add_to_vocabulary(g)
    scorer.build()
    dist = T.Distance(T.damerau_levenshtein(na, ng, 255), T.longest_common_substring_length(na, ng), T.common_prefix_length(na, ng),
                      T.common_suffix_length(na, ng), T.is_lowercase(g[0]) == T.is_lowercase(a[0]))
    res = scorer.score_and_rank([(vid, dist)], len(na), 0, float("-inf"), 0.0, 0.0, a)
    assert len(res) == 1
    return OK, dist.ld, res[0].dist_score


def expected_record(side, a, g, P):
    """P: twin.SearchParameters.  -> dict of FIELDS."""
    rows = side.rows(a, P) if a else []
    gid = side.encoder.get(g, NONE)
    rank = next((i for i, r in enumerate(rows) if r[0] == gid), -1) if gid != NONE else -1
    status, ld, score = pair_measures(side, a, g)
    k = d = 0
    if status == OK:
        n = len(T.normalize_to_alphabet(a, side.alphabet))
        k = T.clamp_threshold(P.max_anagram_distance, n, MAX_ANAGRAM_DISTANCE)
        d = T.clamp_threshold(P.max_edit_distance, n, MAX_EDIT_DISTANCE)
    if rank >= 0:
        reason, score = RANKED, rows[rank][1]
    elif status != OK:
        reason = STATUS
    elif gid == NONE or not side.flags(gid)[0] or side.flags(gid)[1]:
        reason = NOT_A_RESULT
    else:
        na, ng = T.normalize_to_alphabet(a, side.alphabet), T.normalize_to_alphabet(g, side.alphabet)
        gold_av, focus = T.anahash(g, side.alphabet), T.anahash(a, side.alphabet)
        if P.stop_at_exact_match and side.has_class(a) and gold_av != focus:
            reason = EXACT_STOP
        elif gold_av not in set(side.nearest(a, k, bool(P.stop_at_exact_match))):
            reason = ANAGRAM
        elif T.damerau_levenshtein(na, ng, d) is None:
            reason = EDIT
        elif not score >= P.score_threshold:
            reason = THRESHOLD
        else:
            reason = CROPPED
    return {"gold_vocab_id": gid, "rank": rank, "n_results": len(rows), "top_vocab_id": rows[0][0] if rows else NONE, "gold_score": score,
            "ld": ld, "k": k, "d": d, "status": status, "reason": reason}


def edited_pairs(words, n, seed, min_len=4, max_len=14, letters="abcdefghijklmnopqrstuvwxyz"):
    """n (query, source word) pairs: one to three random edits (delete, insert, substitute, transpose) of words of the lexicon, the
    source word being the gold answer.  Seeded: the same pairs for the same arguments."""
    rng = random.Random(seed)
    pool = [w for w in words if min_len <= len(w) <= max_len and w.isalpha() and w.isascii()]
    out = []
    while len(out) < n:
        w = rng.choice(pool)
        cs = list(w)
        for _ in range(rng.randint(1, 3)):
            op = rng.randrange(4)
            if op == 0 and len(cs) > 2:
                del cs[rng.randrange(len(cs))]
            elif op == 1:
                cs.insert(rng.randrange(len(cs) + 1), rng.choice(letters))
            elif op == 2:
                cs[rng.randrange(len(cs))] = rng.choice(letters)
            elif len(cs) > 1:
                p = rng.randrange(len(cs) - 1)
                cs[p], cs[p + 1] = cs[p + 1], cs[p]
        out.append(("".join(cs), w))
    return out


# ---- the hand-made lexicon over simple_alphabet.tsv: every reason at least once ------------------------------------------------------------
HAND_WORDS = ["abcdef", "abcdeg", "abcdxf", "abcxef", "abxdef", "axcdef", "xbcdef", "abcdefgh", "abcd", "fedcba", "abcfed", "zzzzzz", "abcdfe",
              "abcdyz", "house", "mouse", "houses", "hose"]


def hand_params(**kw):
    """k = 2, d = 1, three rows kept, a score threshold between the one-edit candidates' scores (0.7083 < 0.71 < 0.7292), no cutoff"""
    d = dict(max_anagram_distance=("abs", 2), max_edit_distance=("abs", 1), max_matches=3, score_threshold=0.71, cutoff_threshold=0.0,
             stop_at_exact_match=False, freq_weight=0.0)
    d.update(kw)
    return T.SearchParameters(**d)


# (input, gold, reason, rank) under hand_params(); the rows of "abcdef" without a crop are abcdef, abcdeg, xbcdef | axcdef, abcdxf
HAND_PAIRS = [
    ("abcdef", "abcdef", RANKED, 0),          # gold at rank 0
    ("abcdef", "xbcdef", RANKED, 2),          # gold at the last kept rank, max_matches - 1
    ("abcdef", "axcdef", CROPPED, -1),        # the first row the crop drops
    ("abcdef", "abcdyz", ANAGRAM, -1),        # two anagram steps beyond k: L1 = 4
    ("abcdef", "abcd", EDIT, -1),             # ld == d + 1 inside k
    ("abcdef", "abcdfe", THRESHOLD, -1),      # 0.7083.. just below the score threshold
    ("abcdef", "nothere", NOT_A_RESULT, -1),  # gold unknown
    ("abcdef", "<unk>", NOT_A_RESULT, -1),    # gold known (id 2) but not INDEXED
    ("abcdef", "", STATUS, -1),               # empty gold
    ("abcdef", "a" * 256, STATUS, -1),        # gold of 256 symbols
    ("", "abcdef", STATUS, -1),               # an input that normalises to nothing
]
# under hand_params(stop_at_exact_match=True): the input is itself a lexicon word, gold another word
HAND_PAIRS_STOP = [("house", "mouse", EXACT_STOP, -1), ("house", "house", RANKED, 0), ("housf", "house", RANKED, 0)]


def light_twin(alphabet, entries, weights=None):
    """A twin model that only knows texts, ids, frequencies and flags of `entries` ([(text, frequency | None)], in file order): the
    vocabulary side of the twin without the per-entry normalisation and the index (seconds on a full-size lexicon).  read_variants,
    score_and_rank and the confusable weights work on it; build() and find_variants do not."""
    tw = T.VariantModel(alphabet, weights)
    for text, freq in entries:
        if freq is not None:
            tw.have_freq = True
        tw.encoder[text] = len(tw.decoder)
        tw.decoder.append(T.VocabValue(text, [], 1 if freq is None else freq))
    return tw


def rows_by_twin_tail(o, tw, params_of):
    """rows(text, P): the C oracle's gathered instances (its scored pairs, in enumeration order) through the TWIN's score_and_rank on
    `tw` -- confusables late or early, variant lists -- for models the C oracle's own tail does not cover."""
    def rows(text, P):
        _res, pl, npairs, _ncls = o.find_variants(text, params_of(P), want_pairs=True, cap=1 << 17)
        assert npairs == len(pl), (npairs, len(pl))
        inst = [(v, T.Distance(ld, lcs, pre, suf, bool(same))) for v, ld, lcs, pre, suf, same in pl if ld >= 0]
        n = len(T.normalize_to_alphabet(text, tw.alphabet))
        res = tw.score_and_rank(inst, n, P.max_matches, P.score_threshold, P.cutoff_threshold, P.freq_weight, text)
        return [(r.vocab_id, r.dist_score, r.freq_score, r.via) for r in res]
    return rows
