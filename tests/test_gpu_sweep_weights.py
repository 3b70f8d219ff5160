"""anx_evaluate_sweep_weights on the device (analiticcl_amd/csrc/reweigh.hip) against two independent sides: the oracle side -- the C
oracle's instances (one oracle model serves every weight set) through the TWIN's score_and_rank under the set's weights
(eval_twin.rows_by_twin_tail), classified by eval_twin.expected_record and reduced by sweep_twin.summarize -- and the product's own
evaluate_arrays on models created with the set's weights.  Every field of every summary is compared with `==`, records byte for byte.
The shapes are the smallest at which the pass can go wrong: one lane, the wave edges, more than one block, row lists beyond 64 and
beyond RANK_LCAP = 128 rows, inputs without rows, inputs whose every row falls below the threshold, chunk seams, two replicas."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import cli, synth
from oracle import cwrap as O
from oracle import twin as T

import eval_twin as E
import sweep_twin as S

NONE_INPUTS = ["qqqqqqqqqqqqqqqqqqqqjjjjjjjjjj", "zzzzzzzzzzzzzzzzzzzzzzzzzzzzzzxxxxx"]   # inputs without rows (tests/test_gpu_sweep.py)
W_DEFAULT, W_LD, W_LCS = (0.5, 0.125, 0.125, 0.125, 0.125), (1.0, 0.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0, 0.0)
HAND_WEIGHTS = [W_DEFAULT, W_LD, W_LCS, (0.2, 0.1, 0.6, 0.05, 0.05), (0.0, 0.0, 0.0, 0.5, 0.5)]


def oracle_params(p):
    return O.make_params(p.max_anagram_distance, p.max_edit_distance, p.max_matches, p.score_threshold, p.cutoff_threshold,
                         p.stop_at_exact_match, p.freq_weight)


def product_params(p):
    def th(t):
        return int(t[1]) if t[0] == "abs" else float(t[1]) if t[0] == "ratio" else (float(t[1]), int(t[2]))
    return A.SearchParameters(max_anagram_distance=th(p.max_anagram_distance), max_edit_distance=th(p.max_edit_distance), max_matches=p.max_matches,
                              score_threshold=p.score_threshold, cutoff_threshold=p.cutoff_threshold, stop_criterion=bool(p.stop_at_exact_match),
                              freq_weight=p.freq_weight)


def product_weights(w):
    return A.Weights(ld=w[0], lcs=w[1], prefix=w[2], suffix=w[3], case=w[4])


class CachedInstances:
    """The C oracle's gathered instances per (input, k, d, stop): they do not depend on the weights, so every weight set reads one call."""

    def __init__(self, o):
        self.o, self.memo = o, {}

    def find_variants(self, text, params, want_pairs=False, cap=1 << 16):
        key = (text, bytes(params.max_anagram_distance), bytes(params.max_edit_distance), params.stop_at_exact_match, want_pairs, cap)
        if key not in self.memo:
            self.memo[key] = self.o.find_variants(text, params, want_pairs=want_pairs, cap=cap)
        return self.memo[key]


class OracleSides:
    """One E.Side per weight set over ONE oracle model: rows through the twin's tail under the set's weights, the anagram stage from
    the C oracle, the direct pair's score from the twin under the set's weights (E.pair_measures reads Side.weights)."""

    def __init__(self, o, alphabet, entries):
        self.o, self.alphabet, self.entries, self.cache, self.sides = o, alphabet, entries, CachedInstances(o), {}
        self.nearest, self.has_class = {}, {}

    def side(self, w):
        if w not in self.sides:
            tw = E.light_twin(self.alphabet, self.entries, weights=T.Weights(*w))
            rows = E.rows_by_twin_tail(self.cache, tw, oracle_params)

            def nearest(text, k, stop):
                if (text, k, stop) not in self.nearest:
                    self.nearest[(text, k, stop)] = self.o.find_nearest(text, k, stop)
                return self.nearest[(text, k, stop)]

            def has_class(text):
                if text not in self.has_class:
                    self.has_class[text] = len(self.o.anagram_instances(text)) > 0
                return self.has_class[text]

            self.sides[w] = E.Side(self.alphabet, T.Weights(*w), tw.encoder, lambda v, tw=tw: (tw.decoder[v].indexed, tw.decoder[v].transparent), rows,
                                   nearest, has_class)
        return self.sides[w]

    def records(self, pairs, sets):
        """sets: [(twin.SearchParameters, weight tuple)] -> per set the expected records"""
        return [[E.expected_record(self.side(w), a, b, P) for a, b in pairs] for P, w in sets]


def reduced(records_per_set):
    return [S.summarize(r, baseline=records_per_set[0]) for r in records_per_set]


def sweep(g, pairs, sets, **kw):
    return g.evaluate_sweep_weights_arrays([a for a, _ in pairs], [b for _, b in pairs], [product_params(P) for P, _w in sets],
                                           [product_weights(w) for _P, w in sets], **kw)


def assert_summaries(got, expected):
    assert len(got) == len(expected)
    for s, (g, e) in enumerate(zip(got, expected)):
        g = S.of_product(g)
        for k in S.KEYS:
            assert g[k] == e[k], (s, k, g[k], e[k])


def assert_records(rec, expected):
    assert rec.shape == (len(expected), len(expected[0]))
    for s, exp in enumerate(expected):
        for i, e in enumerate(exp):
            for k in E.FIELDS:
                assert rec[s][k][i] == e[k], (s, i, k, rec[s][k][i], e[k])
    assert not rec["_pad"].any()


def assert_against_product_models(rec, pairs, sets, models):
    """models: weight tuple -> a product model created with those weights"""
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    for s, (P, w) in enumerate(sets):
        assert rec[s].tobytes() == models[w].evaluate_arrays(a, b, product_params(P)).tobytes(), (s, w)


def product_model(alphabet, lexicon, w):
    g = A.VariantModel(alphabet, product_weights(w), device=0)
    g.read_lexicon(lexicon)
    g.build()
    return g


# ---- models ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand(data_dir, tmp_path_factory):
    alphabet = os.path.join(data_dir, "simple.alphabet.tsv")
    lex = tmp_path_factory.mktemp("rwhand") / "hand.lexicon"
    lex.write_text("\n".join(E.HAND_WORDS) + "\n")
    models = {w: product_model(alphabet, str(lex), w) for w in HAND_WEIGHTS}
    o = O.OracleModel(alphabet_path=alphabet)
    for i, w in enumerate(E.HAND_WORDS):
        assert o.add(w) == 3 + i
    o.build()
    sides = OracleSides(o, T.read_alphabet(alphabet), [(w, None) for w in E.HAND_WORDS])
    pairs = [(a, b) for a, b, _r, _k in E.HAND_PAIRS + E.HAND_PAIRS_STOP]
    Ps = [E.hand_params(), E.hand_params(max_matches=1, score_threshold=0.9), E.hand_params(cutoff_threshold=1.0, max_matches=0, score_threshold=0.5),
          E.hand_params(stop_at_exact_match=True)]
    sets = [(P, w) for P in Ps for w in HAND_WEIGHTS]   # sets 0 .. 4: hand_params() under the five weight sets
    expected = sides.records(pairs, sets)   # computed once, shared by the tests below
    return models, str(lex), alphabet, pairs, sets, expected


EDGE_PARAMS = [T.SearchParameters(("abs", 3), ("abs", 2), 10, 0.25, 2.0, False, 0.0), T.SearchParameters(("abs", 2), ("abs", 1), 1, 0.25, 2.0, False, 0.0)]
ENG_SETS = [(P, w) for P in EDGE_PARAMS for w in (W_DEFAULT, W_LD, W_LCS)]


@pytest.fixture(scope="module")
def eng(data_dir):
    alphabet, lexicon = os.path.join(data_dir, "simple.alphabet.tsv"), os.path.join(data_dir, "eng.aspell.lexicon")
    g = product_model(alphabet, lexicon, W_DEFAULT)
    o = O.OracleModel(alphabet_path=alphabet)
    o.read_lexicon(lexicon)
    o.build()
    words = synth.load_lexicon_words(lexicon)
    sides = OracleSides(o, T.read_alphabet(alphabet), [(w, None) for w in words])   # ids 0-2 are <bos>, <eos>, <unk>; every lexicon line is a new item
    pairs = E.edited_pairs(words, 257, seed=1)
    expected = sides.records(pairs, ENG_SETS)   # computed once, shared by the tests below
    return g, o, words, sides, pairs, expected, alphabet, lexicon


# ---- 1. the hand-made lexicon: twenty sets in one call ---------------------------------------------------------------------------------
def test_twenty_sets_on_the_hand_made_lexicon(hand):
    models, _lex, _alphabet, pairs, sets, expected = hand
    want = reduced(expected)
    # what the twin gives under hand_params() for the five weight sets: the weights move every weight-dependent field
    assert [(w["reasons"][E.RANKED], w["reasons"][E.THRESHOLD], w["reasons"][E.CROPPED]) for w in want[:5]] == [(5, 1, 1), (4, 0, 3), (5, 2, 0), (3, 4, 0), (5, 2, 0)]
    assert [w["n_results"] for w in want[:5]] == [37, 25, 37, 25, 34]
    assert (want[0]["rank_hist"][:3], want[1]["rank_hist"][:3], want[4]["rank_hist"][:3]) == ([3, 0, 2], [3, 1, 0], [2, 2, 1])
    assert want[4]["lost_at_1"] == 1
    assert sum(1 for x in range(5) for y in range(x) if want[x]["reasons"] != want[y]["reasons"]) >= 3
    g = models[HAND_WEIGHTS[3]]   # the model's own weights play no part: any of the five models gives the same bytes
    sums, rec = sweep(g, pairs, sets, with_records=True)
    assert_summaries(sums, want)
    assert_records(rec, expected)
    assert_against_product_models(rec, pairs, sets, models)
    other, other_rec = sweep(models[W_DEFAULT], pairs, sets, with_records=True)
    assert other.tobytes() == sums.tobytes() and other_rec.tobytes() == rec.tobytes()
    assert (sums["n"] == len(pairs)).all() and sums["gained_at_1"][0] == 0 and sums["lost_at_1"][0] == 0
    d = g.evaluate_sweep_weights([a for a, _ in pairs], [b for _, b in pairs], [product_params(P) for P, _w in sets], [product_weights(w) for _P, w in sets])
    for s, e in enumerate(want):
        assert d[s]["reasons"] == dict(zip(E.REASONS, e["reasons"])) and d[s]["rank_hist"] == e["rank_hist"]
        assert d[s]["weights"] == dict(zip(("ld", "lcs", "prefix", "suffix", "case"), sets[s][1]))


# ---- 2. eng.aspell: ties in masses (lcs only), wave and block edges ---------------------------------------------------------------------
def test_eng_three_weight_sets(eng):
    g, _o, _words, _sides, pairs, expected, _alphabet, _lexicon = eng
    want = reduced(expected)
    assert any(w["gained_at_1"] + w["lost_at_1"] > 0 for w in want[1:3])   # a non-default weight set moves gold to or from rank 0
    sums, rec = sweep(g, pairs, ENG_SETS, with_records=True)
    assert_summaries(sums, want)
    assert_records(rec, expected)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_wave_edges(eng, n):
    g, _o, _words, _sides, pairs, expected, _alphabet, _lexicon = eng
    sums, rec = sweep(g, pairs[:n], ENG_SETS, with_records=True)
    assert_summaries(sums, reduced([e[:n] for e in expected]))
    assert_records(rec, [e[:n] for e in expected])


# ---- 3. long and empty row lists --------------------------------------------------------------------------------------------------------
def test_long_and_empty_row_lists(eng):
    """Absolute thresholds are clamped to half the input's length (3-letter inputs run at k = d = 1), so k = 3, d = 2 gives lists beyond
    64 rows on this lexicon and the ratio thresholds of test_gpu_sweep.py's overflow test give the lists beyond RANK_LCAP = 128."""
    g, o, _words, sides, _pairs, _expected, _alphabet, _lexicon = eng
    abs32, ratio = (("abs", 3), ("abs", 2)), (("ratio", 1.0), ("ratio", 1.0))
    def base_rows(a, kd):
        return len(o.find_variants(a, oracle_params(T.SearchParameters(kd[0], kd[1], 0, float("-inf"), 0.0, False, 0.0)), want_pairs=True, cap=1 << 17)[0])
    assert 64 < base_rows("ther", abs32) <= 128 and base_rows("cat", ratio) > 128 and base_rows("teh", ratio) > 128
    pairs = [(NONE_INPUTS[0], "cat"), (NONE_INPUTS[1], "dog"), ("recieve", "receive"), ("recieve", "reprieve")]
    for a, kd in (("ther", abs32), ("them", abs32), ("cat", ratio), ("teh", ratio)):
        rows = o.find_variants_via(a, oracle_params(T.SearchParameters(kd[0], kd[1], 0, 0.0, 0.0, False, 0.0)), cap=1 << 15)
        pairs += [(a, o.text(rows[0][0])), (a, o.text(rows[len(rows) // 2][0])), (a, o.text(rows[-1][0])), (a, "incomprehensible")]
    Ps = [T.SearchParameters(ratio[0], ratio[1], 0, 0.0, 0.0, False, 0.0),      # every row kept and ranked: lists beyond RANK_LCAP
          T.SearchParameters(ratio[0], ratio[1], 10, 0.25, 2.0, False, 0.0),    # the crop of such a list
          T.SearchParameters(abs32[0], abs32[1], 0, 0.0, 0.0, False, 0.0),      # lists beyond one wave
          T.SearchParameters(abs32[0], abs32[1], 10, 0.99, 2.0, False, 0.0)]    # "recieve" is no word: every row of it falls below 0.99
    sets = [(P, w) for P in Ps for w in (W_DEFAULT, W_LCS)]
    expected = sides.records(pairs, sets)
    assert max(e["n_results"] for e in expected[0]) > 128 and max(e["n_results"] for e in expected[1]) > 128
    assert 64 < max(e["n_results"] for e in expected[4]) <= 128
    assert expected[6][2]["n_results"] == 0 and expected[6][2]["reason"] == E.THRESHOLD and expected[0][0]["n_results"] == 0
    sums, rec = sweep(g, pairs, sets, with_records=True)
    assert_summaries(sums, reduced(expected))
    assert_records(rec, expected)


# ---- 4. frequencies ---------------------------------------------------------------------------------------------------------------------
def test_frequencies_and_a_frequency_weight(data_dir, tmp_path):
    alphabet = os.path.join(data_dir, "simple.alphabet.tsv")
    freqs = [(w, 1 + (7 * i * i + 3 * i) % 23) for i, w in enumerate(E.HAND_WORDS)]
    lex = tmp_path / "freq.lexicon"
    lex.write_text("".join("%s\t%d\n" % e for e in freqs))
    weights = [W_DEFAULT, W_LCS, (0.0, 0.0, 0.0, 0.5, 0.5)]
    models = {w: product_model(alphabet, str(lex), w) for w in weights}
    o = O.OracleModel(alphabet_path=alphabet)
    for w, f in freqs:
        o.add(w, f)
    o.build()
    sides = OracleSides(o, T.read_alphabet(alphabet), freqs)
    pairs = [(a, b) for a, b, _r, _k in E.HAND_PAIRS + E.HAND_PAIRS_STOP]
    Ps = [E.hand_params(score_threshold=0.3), E.hand_params(score_threshold=0.3, freq_weight=0.5), E.hand_params(max_matches=0, score_threshold=0.0, freq_weight=0.5, cutoff_threshold=1.2)]
    sets = [(P, w) for P in Ps for w in weights]
    expected = sides.records(pairs, sets)
    want = reduced(expected)
    assert any(want[s]["rank_hist"] != want[s + 3]["rank_hist"] for s in range(3))   # the frequency weight reorders something
    sums, rec = sweep(models[W_DEFAULT], pairs, sets, with_records=True)
    assert_summaries(sums, want)
    assert_records(rec, expected)
    assert_against_product_models(rec, pairs, sets, models)


# ---- 5. what is shared between the sets -------------------------------------------------------------------------------------------------
def test_sharing_is_real(eng):
    g, _o, _words, _sides, pairs, _expected, _alphabet, _lexicon = eng
    a, b = [x for x, _ in pairs[:130]], [y for _, y in pairs[:130]]
    r0 = A.VariantModel.sweep_stats()
    for P in EDGE_PARAMS:
        g.evaluate_sweep_arrays(a, b, [product_params(P)])   # the batch runs of an anx_evaluate_gold call: one per parameter set here
    runs_of_two_gold_calls = A.VariantModel.sweep_stats()["batch_runs"] - r0["batch_runs"]
    t0 = A.VariantModel.weight_sweep_stats()
    assert list(t0) == ["calls", "chunks", "groups", "sets", "pair_passes", "batch_runs", "rows_rescored", "bytes_down"]
    sums = sweep(g, pairs[:130], ENG_SETS)
    t1 = A.VariantModel.weight_sweep_stats()
    grew = {k: t1[k] - t0[k] for k in t0}
    assert (grew["calls"], grew["chunks"], grew["pair_passes"], grew["groups"], grew["sets"]) == (1, 1, 1, 2, len(ENG_SETS))
    assert grew["batch_runs"] == runs_of_two_gold_calls == 2
    assert grew["bytes_down"] == 624 * len(ENG_SETS) and grew["rows_rescored"] > 0
    _s, rec = sweep(g, pairs[:130], ENG_SETS, with_records=True)
    t2 = A.VariantModel.weight_sweep_stats()
    assert t2["bytes_down"] - t1["bytes_down"] == len(ENG_SETS) * (624 + 130 * 32) and _s.tobytes() == sums.tobytes()


# ---- 6. chunk seams, replicas, the packed form ------------------------------------------------------------------------------------------
def test_chunk_seams_replicas_and_the_pointer_form(eng):
    g, _o, _words, _sides, pairs, expected, alphabet, lexicon = eng
    whole, whole_rec = sweep(g, pairs, ENG_SETS, with_records=True)
    assert_summaries(whole, reduced(expected))
    cut, cut_rec = sweep(g, pairs, ENG_SETS, with_records=True, chunk=100)
    assert cut.tobytes() == whole.tobytes() and cut_rec.tobytes() == whole_rec.tobytes()
    ptr, ptr_rec = sweep(g, pairs, ENG_SETS, with_records=True, packed=False)
    assert ptr.tobytes() == whole.tobytes() and ptr_rec.tobytes() == whole_rec.tobytes()
    g2 = A.VariantModel(alphabet, A.Weights(), device=0)
    g2.read_lexicon(lexicon)
    g2.build()
    g2.to_devices([0, 0])
    assert g2.num_replicas == 2
    for n in (2, 257):
        s2, r2 = sweep(g2, pairs[:n], ENG_SETS, with_records=True)
        s1, r1 = (whole, whole_rec) if n == 257 else sweep(g, pairs[:n], ENG_SETS, with_records=True)
        assert s2.tobytes() == s1.tobytes() and r2.tobytes() == r1.tobytes()
    with pytest.raises(A.AnxError):
        sweep(g, pairs[:10], ENG_SETS, chunk=0)


# ---- 7. the call and its neighbours ------------------------------------------------------------------------------------------------------
def test_no_side_effects(eng):
    g, _o, _words, _sides, pairs, _expected, _alphabet, _lexicon = eng
    a, b = [x for x, _ in pairs[:100]], [y for _, y in pairs[:100]]
    Ps = [product_params(P) for P in EDGE_PARAMS]
    before = g.find_variants_ids(a, Ps[0])
    sums_before, rec_before = g.evaluate_sweep_arrays(a, b, Ps, with_records=True)
    sweep(g, pairs[:100], ENG_SETS)
    assert g.find_variants_ids(a, Ps[0]) == before
    sums_after, rec_after = g.evaluate_sweep_arrays(a, b, Ps, with_records=True)
    assert sums_after.tobytes() == sums_before.tobytes() and rec_after.tobytes() == rec_before.tobytes()


# ---- 8. the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_weight_grid(hand, tmp_path, capsys):
    models, lex, alphabet, pairs, sets, _expected = hand
    inp = tmp_path / "pairs.tsv"
    inp.write_text("".join("%s\t%s\n" % p for p in pairs))
    grid = tmp_path / "grid.tsv"
    rows = [(1, W_DEFAULT), (3, HAND_WEIGHTS[3]), (3, W_LCS)]
    grid.write_text("n\tw-ld\tw-lcs\tw-prefix\tw-suffix\n" + "".join("%d\t%r\t%r\t%r\t%r\n" % ((n,) + w[:4]) for n, w in rows))
    summary = tmp_path / "summary.json"
    argv = ["sweep", "-a", alphabet, "-l", lex, "-k", "2", "-d", "1", "-n", "3", "-t", "0.71", "-T", "0", "--weight-case", "0.05", "--device", "0",
            "--grid", str(grid), "--summary-json", str(summary), str(inp)]
    assert cli.main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    ws = [w[:4] + (0.05,) for _n, w in rows]   # the absent column w-case takes --weight-case
    want = models[W_DEFAULT].evaluate_sweep_weights([a for a, _ in pairs], [b for _, b in pairs],
                                                    [product_params(E.hand_params(max_matches=n)) for n, _w in rows], [product_weights(w) for w in ws])
    assert len(lines) == 3
    for line, (n, _w), w, e in zip(lines, rows, ws, want):
        cells = line.split("\t")
        assert cells[:7] == ["2", "1", str(n), "0.71", "0", "0", "0"] and [float(c) for c in cells[7:12]] == list(w)
        assert cells[12] == str(len(pairs)) and cells[13] == cli.rust_f64(e["accuracy_at_1"]) and cells[14] == cli.rust_f64(e["mrr"])
        assert cells[16:24] == [str(e["reasons"][r]) for r in E.REASONS] and cells[24:26] == [str(e["gained_at_1"]), str(e["lost_at_1"])]
    js = json.loads(summary.read_text())
    assert [j["weights"] for j in js] == [e["weights"] for e in want] and [j["params"]["w-case"] for j in js] == ["0.05"] * 3
    assert [j["reasons"] for j in js] == [e["reasons"] for e in want]
