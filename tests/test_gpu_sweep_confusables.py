"""anx_evaluate_sweep_confusables on the device (analiticcl_amd/csrc/csweep.hip) against two independent sides: the product's own
evaluate_arrays on PRODUCT MODELS that hold every set's list (patterns[j] with the set's weight, before pruning iff the set is early),
and the oracle side -- the C oracle's instances through the TWIN's score_and_rank with the twin's confusable weights
(eval_twin.rows_by_twin_tail), classified by eval_twin.expected_record (the direct pair's UNWEIGHTED score for THRESHOLD) and reduced by
sweep_twin.summarize.  Every field of every summary is compared with `==`, records byte for byte; the masks alone against
oracle/sesdiff_twin.py pattern by pattern."""
import os
import random
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli, synth
from oracle import cwrap as O
from oracle import twin as T

import eval_twin as E
import sweep_twin as S
import sweep_conf_common as SC
import test_gpu_sweep_weights as W
from pairs_conf_common import edit

W_DEFAULT = W.W_DEFAULT
# over the letters of eval_twin.HAND_WORDS; "abcdef" -> "abcdeg" is matched by patterns 0, 1 and 8
HAND_PATTERNS = ("-[f]+[g]", "+[g]", "+[s]$", "-[u]", "^-[h]+[m]", "=[a]-[b]", "-[b|c]+[x]", "-[e]+[x]", "=[e]-[f]", "-[h]", "+[ë]", "-[d]=[e]")
ONES = (1.0,) * len(HAND_PATTERNS)


def weights_with(**at):
    w = list(ONES)
    for j, x in at.items():
        w[int(j[1:])] = x
    return tuple(w)


def product_model(alphabet, lexicon, patterns, weights, early, w=W_DEFAULT, devices=None):
    g = A.VariantModel(alphabet, W.product_weights(w), device=0)
    g.read_lexicon(lexicon)
    for p, x in zip(patterns, weights):
        g.add_to_confusables(p, x)
    if early:
        g.set_confusables_before_pruning()
    g.build()
    if devices:
        g.to_devices(devices)
    return g


class Sides:
    """The oracle side per (weights, early): one C oracle serves every set (its instances do not depend on the list); rows through the
    twin's score_and_rank on a light twin that holds the set's list; the direct pair's score from a twin WITHOUT a list."""

    def __init__(self, o, alphabet_path, entries, patterns, w=W_DEFAULT):
        self.o, self.alphabet, self.entries, self.patterns, self.w = o, T.read_alphabet(alphabet_path), entries, patterns, w
        self.cache, self.sides, self.nearest, self.has_class = W.CachedInstances(o), {}, {}, {}

    def side(self, weights, early):
        if (weights, early) not in self.sides:
            tw = E.light_twin(self.alphabet, self.entries, weights=T.Weights(*self.w))
            for p, x in zip(self.patterns, weights):
                tw.add_to_confusables(p, x)
            if early:
                tw.set_confusables_before_pruning()
            tail, memo = E.rows_by_twin_tail(self.cache, tw, W.oracle_params), {}

            def rows(text, P):   # an input's rows once per set, however many gold answers it is paired with
                key = (text, P.max_matches, P.score_threshold, P.cutoff_threshold, P.freq_weight, P.stop_at_exact_match, str(P.max_anagram_distance), str(P.max_edit_distance))
                if key not in memo:
                    memo[key] = tail(text, P)
                return memo[key]

            def nearest(text, k, stop):
                if (text, k, stop) not in self.nearest:
                    self.nearest[(text, k, stop)] = self.o.find_nearest(text, k, stop)
                return self.nearest[(text, k, stop)]

            def has_class(text):
                if text not in self.has_class:
                    self.has_class[text] = len(self.o.anagram_instances(text)) > 0
                return self.has_class[text]

            self.sides[(weights, early)] = E.Side(self.alphabet, T.Weights(*self.w), tw.encoder, lambda v, tw=tw: (tw.decoder[v].indexed, tw.decoder[v].transparent),
                                                  rows, nearest, has_class)
        return self.sides[(weights, early)]

    def records(self, pairs, sets):
        """sets: [(twin.SearchParameters, weights tuple, early)] -> per set the expected records"""
        return [[E.expected_record(self.side(w, e), a, b, P) for a, b in pairs] for P, w, e in sets]


def sweep(g, pairs, patterns, sets, **kw):
    return g.evaluate_sweep_confusables_arrays([a for a, _ in pairs], [b for _, b in pairs], list(patterns), [W.product_params(P) for P, _w, _e in sets],
                                               [list(w) for _P, w, _e in sets], [e for _P, _w, e in sets], **kw)


def product_records(models, pairs, sets):
    """models: (weights, early) -> product model holding that list"""
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    return [models[(w, e)].evaluate_arrays(a, b, W.product_params(P)) for P, w, e in sets]


def assert_equals_product(sums, rec, prod):
    for s, r in enumerate(prod):
        assert rec[s].tobytes() == r.tobytes(), s
    want = [S.summarize(r, baseline=prod[0]) for r in prod]
    W.assert_summaries(sums, want)


# ---- the hand-made lexicon ---------------------------------------------------------------------------------------------------------------
HAND_EXTRA = [("abcdef", "abcdeg"), ("abcdeh", "abcdeg"), ("abcdeh", "abcdef"), ("house", "houses"), ("house", "hose"), ("housf", "house"), ("abcdex", "abcdeg")]


@pytest.fixture(scope="module")
def hand(data_dir, tmp_path_factory):
    alphabet = os.path.join(data_dir, "simple.alphabet.tsv")
    lex = tmp_path_factory.mktemp("cshand") / "hand.lexicon"
    lex.write_text("\n".join(E.HAND_WORDS) + "\n")
    plain = W.product_model(alphabet, str(lex), W_DEFAULT)
    o = O.OracleModel(alphabet_path=alphabet)
    for i, w in enumerate(E.HAND_WORDS):
        assert o.add(w) == 3 + i
    o.build()
    sides = Sides(o, alphabet, [(w, None) for w in E.HAND_WORDS], HAND_PATTERNS)
    pairs = [(a, b) for a, b, _r, _k in E.HAND_PAIRS + E.HAND_PAIRS_STOP] + HAND_EXTRA
    models = {}

    def model(w, early):
        if (w, early) not in models:
            models[(w, early)] = product_model(alphabet, str(lex), HAND_PATTERNS, w, early)
        return models[(w, early)]

    return plain, str(lex), alphabet, pairs, sides, model, o


def with_models(model, sets):
    return {(w, e): model(w, e) for _P, w, e in sets}


# ---- 1. the masks alone ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic(data_dir, tmp_path_factory):
    """400 words over the letters the twelve patterns speak of, and 300 inputs: edited words and words themselves"""
    alphabet = os.path.join(data_dir, "simple.alphabet.tsv")
    rng = random.Random(21)
    short = sorted({"".join(rng.choice(SC.LETTERS) for _ in range(rng.randint(4, 10))) for _ in range(420)})[:400]
    long1, long2 = ("abcde" * 13)[:64], ("iykzabcde" * 8)[:69]
    words = short + [long1, long2]
    lex = tmp_path_factory.mktemp("cssyn") / "syn.lexicon"
    lex.write_text("\n".join(words) + "\n")
    g = W.product_model(alphabet, str(lex), W_DEFAULT)
    o = O.OracleModel(alphabet_path=alphabet)
    for w in words:
        o.add(w)
    o.build()
    inputs = [edit(rng, rng.choice(short), rng.randint(1, 2), SC.LETTERS) for _ in range(250)] + [rng.choice(short) for _ in range(50)]
    return g, o, words, inputs, (long1, long2)


MASK_PARAMS = T.SearchParameters(("abs", 3), ("abs", 2), 0, float("-inf"), 0.0, False, 0.0)


def oracle_rows(o, inputs, patterns):
    """{(input index, vocabulary id): mask} over the C oracle's instances with ld <= d"""
    memo, out = {}, {}
    for i, a in enumerate(inputs):
        _res, pl, npairs, _ncls = o.find_variants(a, W.oracle_params(MASK_PARAMS), want_pairs=True, cap=1 << 15)
        assert npairs == len(pl)
        for v, ld, *_rest in pl:
            if ld >= 0:
                out[(i, v)] = SC.oracle_mask(patterns, a, o.text(v), memo)
    return out


def device_rows(g, inputs, patterns):
    pair, vocab, mask = g.sweep_conf_masks(inputs, list(patterns), W.product_params(MASK_PARAMS))
    got = {(int(i), int(v)): int(m) for i, v, m in zip(pair, vocab, mask)}
    assert len(got) == len(pair)   # a row per instance
    return got


def test_masks_alone(synthetic):
    g, o, _words, inputs, _long = synthetic
    want = oracle_rows(o, inputs, SC.PATTERNS)
    # the data first: otherwise it is wrong, not the kernel
    bits = [bin(m).count("1") for m in want.values()]
    assert len(want) > 300 and bits.count(0) > 0 and bits.count(1) > 0 and max(bits) >= 3
    assert any(m == 0 and inputs[i] == o.text(v) for (i, v), m in want.items())   # equal texts: no `-` / `+` to match, the screen's zero
    assert all(len(a) <= 64 for a in inputs)   # no row needs the host
    before = A.VariantModel.conf_sweep_stats()
    got = device_rows(g, inputs, SC.PATTERNS)
    assert got == want
    after = A.VariantModel.conf_sweep_stats()
    assert after["rows_patched"] == before["rows_patched"] and after["rows_host_mode"] == before["rows_host_mode"]
    listed = after["rows_listed"] - before["rows_listed"]
    assert sum(1 for m in want.values() if m) <= listed < len(want)   # the screen drops rows, and none that matches
    assert after["base_rows"] - before["base_rows"] == len(want)
    L.set_switch("ANX_CONFUSABLES", "host")
    try:
        assert device_rows(g, inputs, SC.PATTERNS) == want
        assert A.VariantModel.conf_sweep_stats()["rows_host_mode"] - after["rows_host_mode"] == len(want)
    finally:
        L.set_switch("ANX_CONFUSABLES", None)


# ---- 2. the lane-memory fallback -----------------------------------------------------------------------------------------------------------
def test_lane_memory_fallback(synthetic):
    g, o, _words, _inputs, (long1, long2) = synthetic
    inputs = [long1 + "s", long2 + "s", "abcde"]
    assert [len(a) for a in inputs[:2]] == [65, 70]
    want = oracle_rows(o, inputs, SC.PATTERNS)
    long_rows = [k for k in want if k[0] < 2]
    assert len(long_rows) == 2 and all(want[k] == 1 << 3 for k in long_rows)   # one entry within d each, matched by "-[s]"
    before = A.VariantModel.conf_sweep_stats()
    assert device_rows(g, inputs, SC.PATTERNS) == want
    after = A.VariantModel.conf_sweep_stats()
    assert after["rows_patched"] - before["rows_patched"] == 2 and after["rows_host_mode"] == before["rows_host_mode"]


# ---- 3. the contract on the hand-made lexicon ----------------------------------------------------------------------------------------------
def hand_sets():
    up, down = weights_with(w0=1.5, w6=1.2, w7=1.1), weights_with(w0=0.7, w1=0.9, w2=0.8, w3=0.9, w9=0.6)
    mixed = weights_with(w0=1.1, w1=0.7, w8=1.3, w4=1.2, w6=1.25, w5=0.9)
    sets = []
    for early in (False, True):
        sets += [(E.hand_params(max_matches=1, score_threshold=0.0), up, early), (E.hand_params(max_matches=3), mixed, early),
                 (E.hand_params(max_matches=10, score_threshold=0.5), down, early), (E.hand_params(max_matches=3, cutoff_threshold=2.0, score_threshold=0.5), up, early),
                 (E.hand_params(max_matches=10, cutoff_threshold=2.0, score_threshold=0.0), mixed, early), (E.hand_params(max_matches=1), down, early),
                 (E.hand_params(max_matches=3, score_threshold=0.74), up, early), (E.hand_params(max_matches=3), ONES, early),
                 (E.hand_params(max_matches=10, score_threshold=0.72, cutoff_threshold=2.0), down, early)]
    return [(E.hand_params(), ONES, False)] + sets + [(E.hand_params(max_matches=1, score_threshold=0.0), ONES, False)]


def test_contract_on_the_hand_made_lexicon(hand):
    plain, _lex, _alphabet, pairs, sides, model, _o = hand
    sets = hand_sets()
    assert len(sets) == 20 and {P.max_matches for P, _w, _e in sets} == {1, 3, 10} and {P.cutoff_threshold for P, _w, _e in sets} == {0.0, 2.0}
    expected = sides.records(pairs, sets)
    want = [S.summarize(r, baseline=expected[0]) for r in expected]
    # what the oracle side says of the sets: the threshold bites, the weights and the mode move ranks
    assert any(w["reasons"][E.THRESHOLD] > 0 for w in want) and any(w["gained_at_1"] for w in want) and any(w["lost_at_1"] for w in want)
    assert sum(expected[1 + s] != expected[10 + s] for s in range(9)) >= 4   # late is not early
    assert expected[2] != expected[8] and expected[11] != expected[17]   # and the weights move what hand_params() gives, in both modes
    sums, rec = sweep(plain, pairs, HAND_PATTERNS, sets, with_records=True)
    W.assert_summaries(sums, want)
    W.assert_records(rec, expected)
    assert_equals_product(sums, rec, product_records(with_models(model, sets), pairs, sets))
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    for s in (0, 8, 17):   # all ones, late or early: the plain model's own answer
        assert sets[s][1] == ONES and rec[s].tobytes() == plain.evaluate_arrays(a, b, W.product_params(sets[s][0])).tobytes()
    only = sweep(plain, pairs, HAND_PATTERNS, sets)   # without records: the same summaries
    assert only.tobytes() == sums.tobytes()
    d, r2 = plain.evaluate_sweep_confusables(a, b, list(HAND_PATTERNS), [W.product_params(P) for P, _w, _e in sets], [list(w) for _P, w, _e in sets],
                                             [e for _P, _w, e in sets], records=True)
    assert r2.tobytes() == rec.tobytes() and d[1]["confusable_weights"] == {"-[f]+[g]": 1.5, "-[b|c]+[x]": 1.2, "-[e]+[x]": 1.1} and d[10]["early"] and not d[1]["early"]
    assert [x["reasons"] for x in d] == [dict(zip(E.REASONS, w["reasons"])) for w in want]


def test_frequencies_and_a_frequency_weight(data_dir, tmp_path):
    alphabet = os.path.join(data_dir, "simple.alphabet.tsv")
    freqs = [(w, 1 + (7 * i * i + 3 * i) % 23) for i, w in enumerate(E.HAND_WORDS)]
    lex = tmp_path / "freq.lexicon"
    lex.write_text("".join("%s\t%d\n" % e for e in freqs))
    plain = W.product_model(alphabet, str(lex), W_DEFAULT)
    o = O.OracleModel(alphabet_path=alphabet)
    for w, f in freqs:
        o.add(w, f)
    o.build()
    sides = Sides(o, alphabet, freqs, HAND_PATTERNS)
    pairs = [(a, b) for a, b, _r, _k in E.HAND_PAIRS + E.HAND_PAIRS_STOP] + HAND_EXTRA
    mixed = weights_with(w0=1.1, w1=0.7, w8=1.3, w2=1.2, w3=0.8)
    Ps = [E.hand_params(score_threshold=0.3), E.hand_params(score_threshold=0.3, freq_weight=0.5),
          E.hand_params(max_matches=0, score_threshold=0.0, freq_weight=0.5, cutoff_threshold=1.2)]
    sets = [(Ps[0], ONES, False)] + [(P, mixed, e) for P in Ps for e in (False, True)]
    expected = sides.records(pairs, sets)
    want = [S.summarize(r, baseline=expected[0]) for r in expected]
    assert want[1]["rank_hist"] != want[3]["rank_hist"] or want[2]["rank_hist"] != want[4]["rank_hist"]   # the frequency weight reorders something
    sums, rec = sweep(plain, pairs, HAND_PATTERNS, sets, with_records=True)
    W.assert_summaries(sums, want)
    W.assert_records(rec, expected)
    models = {(w, e): product_model(alphabet, str(lex), HAND_PATTERNS, w, e) for _P, w, e in sets}
    assert_equals_product(sums, rec, product_records(models, pairs, sets))


# ---- 4. the product's order --------------------------------------------------------------------------------------------------------------
def test_product_order(hand):
    plain, _lex, _alphabet, _pairs, _sides, model, _o = hand
    assert SC.oracle_mask(HAND_PATTERNS, "abcdef", "abcdeg") == (1 << 0) | (1 << 1) | (1 << 8)   # three patterns on one row
    x, y, z = 1.1, 0.7, 1.3
    orders = {struct.pack("<d", ((1.0 * p) * q) * r) for p, q, r in ((x, y, z), (x, z, y), (y, x, z), (y, z, x), (z, x, y), (z, y, x))}
    assert len(orders) > 1   # otherwise the test shows nothing
    pairs = [("abcdef", "abcdeg"), ("abcdeh", "abcdeg")]
    P = E.hand_params(max_matches=0, score_threshold=0.0)
    sets = [(P, ONES, False)] + [(P, weights_with(w0=p, w1=q, w8=r), e) for p, q, r in ((x, y, z), (z, x, y), (y, z, x)) for e in (False, True)]
    sums, rec = sweep(plain, pairs, HAND_PATTERNS, sets, with_records=True)
    prod = product_records(with_models(model, sets), pairs, sets)
    assert_equals_product(sums, rec, prod)
    for s in range(1, len(sets)):   # gold is ranked: gold_score is the weighted dist_score, bit for bit
        assert rec[s]["rank"][0] >= 0 and rec[s]["gold_score"][0].tobytes() == prod[s]["gold_score"][0].tobytes()
    assert len({rec[s]["gold_score"][0].tobytes() for s in (1, 3, 5)}) > 1   # and the order of the list shows in the bits


# ---- 5. late is not early ------------------------------------------------------------------------------------------------------------------
def test_late_is_not_early(hand):
    plain, _lex, _alphabet, _pairs, sides, model, _o = hand
    pairs = [("abcdef", "abcdeg"), ("abcdeh", "abcdeg")]
    P = E.hand_params(max_matches=1, score_threshold=0.0)
    fav = weights_with(w0=1.5, w1=1.3)   # both favour "abcdeg": 0.75 * 1.5 * 1.3 > 1.0
    sets = [(P, ONES, False), (P, fav, False), (P, fav, True)]
    expected = sides.records(pairs, sets)
    assert [(e[0]["reason"], e[0]["rank"]) for e in expected] == [(E.CROPPED, -1), (E.CROPPED, -1), (E.RANKED, 0)]   # gold outside the crop: not rescued late
    assert [(e[1]["rank"], e[1]["n_results"]) for e in expected] == [(1, 2), (0, 2), (0, 1)]   # a tie inside the crop: the late re-sort moves rank 0
    sums, rec = sweep(plain, pairs, HAND_PATTERNS, sets, with_records=True)
    W.assert_records(rec, expected)
    W.assert_summaries(sums, [S.summarize(r, baseline=expected[0]) for r in expected])
    assert_equals_product(sums, rec, product_records(with_models(model, sets), pairs, sets))
    assert (int(sums["gained_at_1"][1]), int(sums["gained_at_1"][2])) == (1, 2)


# ---- eng.aspell ----------------------------------------------------------------------------------------------------------------------------
ENG_PATTERNS = ("-[e]", "+[e]", "-[s]$", "+[s]$", "-[i]+[y]", "-[a]+[e]", "=[t]-[h]", "-[c|k]", "+[t]", "^-[t]", "-[é]+[e]", "-[e]+[a|i]")


@pytest.fixture(scope="module")
def eng(data_dir):
    alphabet, lexicon = os.path.join(data_dir, "simple.alphabet.tsv"), os.path.join(data_dir, "eng.aspell.lexicon")
    o = O.OracleModel(alphabet_path=alphabet)
    o.read_lexicon(lexicon)
    o.build()
    words = synth.load_lexicon_words(lexicon)
    return alphabet, lexicon, o, words


def eng_product(eng, weights, early, w=W_DEFAULT, patterns=ENG_PATTERNS, devices=None):
    alphabet, lexicon, _o, _words = eng
    return product_model(alphabet, lexicon, patterns, weights, early, w=w, devices=devices)


# ---- 6. ties in masses, a list beyond 128 rows ---------------------------------------------------------------------------------------------
def test_ties_in_masses_and_long_lists(eng):
    alphabet, lexicon, o, words = eng
    plain = W.product_model(alphabet, lexicon, W.W_LCS)   # lcs only: scores tie in masses
    sides = Sides(o, alphabet, [(w, None) for w in words], ENG_PATTERNS, w=W.W_LCS)
    ratio = (("ratio", 1.0), ("ratio", 1.0))
    base = o.find_variants("cat", W.oracle_params(T.SearchParameters(ratio[0], ratio[1], 0, float("-inf"), 0.0, False, 0.0)), want_pairs=True, cap=1 << 17)[0]
    assert len(base) > 128
    pairs = [("cat", "cut"), ("cat", "cats"), ("teh", "the"), ("recieve", "receive"), (W.NONE_INPUTS[0], "cat")]
    mixed = (0.8, 1.2, 0.9, 1.1, 1.3, 0.7, 1.05, 0.95, 1.15, 0.85, 1.25, 0.75)
    Ps = [T.SearchParameters(ratio[0], ratio[1], 0, 0.0, 0.0, False, 0.0), T.SearchParameters(ratio[0], ratio[1], 10, 0.25, 2.0, False, 0.0)]
    sets = [(Ps[0], (1.0,) * 12, False), (Ps[0], mixed, True), (Ps[1], mixed, False), (Ps[1], mixed, True)]
    expected = sides.records(pairs, sets)
    assert max(e["n_results"] for e in expected[1]) > 128
    sums, rec = sweep(plain, pairs, ENG_PATTERNS, sets, with_records=True)
    W.assert_summaries(sums, [S.summarize(r, baseline=expected[0]) for r in expected])
    W.assert_records(rec, expected)
    m = eng_product(eng, mixed, False, w=W.W_LCS)
    assert rec[2].tobytes() == m.evaluate_arrays([a for a, _ in pairs], [b for _, b in pairs], W.product_params(Ps[1])).tobytes()


# ---- 7. seams and replicas -----------------------------------------------------------------------------------------------------------------
def test_seams_groups_and_replicas(eng):
    alphabet, lexicon, _o, words = eng
    plain = W.product_model(alphabet, lexicon, W_DEFAULT)
    pairs = E.edited_pairs(words, 60, seed=3)
    mixed = (0.8, 1.2, 0.9, 1.1, 1.3, 0.7, 1.05, 0.95, 1.15, 0.85, 1.25, 0.75)
    ones = (1.0,) * 12
    A_, B_ = W.EDGE_PARAMS   # two groups of (k, d)
    sets = [(A_, ones, False), (B_, mixed, False), (A_, mixed, True), (B_, ones, True), (A_, mixed, False)]
    whole, whole_rec = sweep(plain, pairs, ENG_PATTERNS, sets, with_records=True)
    models = {(w, e): eng_product(eng, w, e) for _P, w, e in sets}
    assert_equals_product(whole, whole_rec, product_records(models, pairs, sets))   # gained / lost of a set in another group against set 0
    assert int(whole["gained_at_1"][1]) + int(whole["lost_at_1"][1]) > 0
    before = A.VariantModel.conf_sweep_stats()
    cut, cut_rec = sweep(plain, pairs, ENG_PATTERNS, sets, with_records=True, chunk=7)
    after = A.VariantModel.conf_sweep_stats()
    assert cut.tobytes() == whole.tobytes() and cut_rec.tobytes() == whole_rec.tobytes()
    assert (after["chunks"] - before["chunks"], after["groups"] - before["groups"], after["sets"] - before["sets"]) == (9, 18, 45)
    ptr, ptr_rec = sweep(plain, pairs, ENG_PATTERNS, sets, with_records=True, packed=False)
    assert ptr.tobytes() == whole.tobytes() and ptr_rec.tobytes() == whole_rec.tobytes()
    g2 = W.product_model(alphabet, lexicon, W_DEFAULT)
    g2.to_devices([0, 0])
    assert g2.num_replicas == 2
    s2, r2 = sweep(g2, pairs, ENG_PATTERNS, sets, with_records=True)
    assert s2.tobytes() == whole.tobytes() and r2.tobytes() == whole_rec.tobytes()
    with pytest.raises(A.AnxError):
        sweep(plain, pairs[:10], ENG_PATTERNS, sets, chunk=0)


# ---- 8. eng.aspell: mined patterns, one pattern on -------------------------------------------------------------------------------------------
def test_eng_mined_patterns_one_on(eng):
    alphabet, lexicon, _o, words = eng
    plain = W.product_model(alphabet, lexicon, W_DEFAULT)
    pairs = E.edited_pairs(words, 2000, seed=7)
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    table = [r for r in plain.mine_confusables(a, b) if r["representable"]]
    patterns = [r["pattern"] for r in table[:10]]
    assert len(patterns) == 10
    labels, rows = cli.candidate_grid(patterns, [1.1, 1.25, 0.9])
    assert len(rows) == 31
    P = T.SearchParameters(("abs", 3), ("abs", 2), 10, 0.25, 2.0, False, 0.0)
    sets = [(P, tuple(r), False) for r in rows]
    r0 = A.VariantModel.sweep_stats()
    plain.evaluate_sweep_arrays(a, b, [W.product_params(P)])
    runs_of_one_gold_call = A.VariantModel.sweep_stats()["batch_runs"] - r0["batch_runs"]
    t0 = A.VariantModel.conf_sweep_stats()
    one = sweep(plain, pairs, patterns, sets[:1])
    t1 = A.VariantModel.conf_sweep_stats()
    sums = sweep(plain, pairs, patterns, sets)
    t2 = A.VariantModel.conf_sweep_stats()
    d1, d31 = {k: t1[k] - t0[k] for k in t0}, {k: t2[k] - t1[k] for k in t1}
    assert (d31["calls"], d31["chunks"], d31["groups"], d31["sets"], d31["pair_passes"]) == (1, 1, 1, 31, 1)
    assert d31["batch_runs"] == d1["batch_runs"] == runs_of_one_gold_call   # one base run per group, whatever the number of sets
    assert d31["rows_listed"] == d1["rows_listed"] > 0 and d31["base_rows"] == d1["base_rows"]   # the edit scripts are the group's: thirty more sets add none
    assert d31["rows_patched"] == 0 and d31["bytes_down"] == 31 * 624
    assert one.tobytes() == sums[:1].tobytes()
    base = plain.evaluate_arrays(a, b, W.product_params(P))
    for s in (0, 1, 12, 30):
        m = eng_product(eng, rows[s], False, patterns=patterns)
        recs = m.evaluate_arrays(a, b, W.product_params(P))
        want = S.summarize(recs, baseline=base)
        got = S.of_product(sums[s])
        for k in S.KEYS:
            assert got[k] == want[k], (s, labels[s], k)
        es = A.VariantModel.evaluate_summary(recs)
        ss = A.VariantModel.sweep_summary(sums[s])
        assert ss["reasons"] == es["reasons"] and ss["accuracy_at_1"] == es["accuracy_at_1"] and ss["gold_known"] == es["gold_known"]
    assert any(int(sums["gained_at_1"][s]) + int(sums["lost_at_1"][s]) > 0 for s in range(1, 31))


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def test_cli_candidate_table(hand, tmp_path, capsys):
    plain, lex, alphabet, pairs, _sides, _model, _o = hand
    pairs = [p for p in pairs if p[0] and p[1] and len(p[1]) < 100]
    inp = tmp_path / "pairs.tsv"
    inp.write_text("".join("%s\t%s\n" % p for p in pairs))
    cand = tmp_path / "cand.tsv"
    cand.write_text("".join("%s\t0.5\n" % p for p in HAND_PATTERNS[:4]))
    argv = ["sweep", "-a", alphabet, "-l", lex, "-k", "2", "-d", "1", "-n", "1", "-t", "0", "-T", "0", "--device", "0", "--candidates", str(cand),
            "--candidate-weights", "1.5,0.7", str(inp)]
    outs = []
    for extra in ([], ["--early-confusables"]):
        assert cli.main(argv + extra) == 0
        outs.append(capsys.readouterr().out.splitlines())
    labels, rows = cli.candidate_grid(list(HAND_PATTERNS[:4]), [1.5, 0.7])
    P = W.product_params(E.hand_params(max_matches=1, score_threshold=0.0))
    for lines, early in zip(outs, (False, True)):
        want = plain.evaluate_sweep_confusables([a for a, _ in pairs], [b for _, b in pairs], list(HAND_PATTERNS[:4]), [P] * 9, rows, [early] * 9)
        assert len(lines) == 9
        for line, lab, e in zip(lines, labels, want):
            assert line == cli.candidate_tsv_line(lab, e)
            assert line.split("\t")[:2] == [lab[0], cli.rust_f64(lab[1])]
    assert outs[0] != outs[1]   # late is not early on these pairs
