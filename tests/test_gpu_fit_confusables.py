"""anx_fit_confusable_weights on the device (analiticcl_amd/csrc/fit.hip) against the product's own confusable sweep: every count the
fit produces equals, with `==`, the three summary fields evaluate_sweep_confusables_arrays gives for the same weights (late), a path
that is itself pinned to the C oracle and the twin (test_gpu_sweep_confusables.py).  Whole fits are compared with the Python greedy of
fit_twin.py driven by that sweep, the final counts with product models that hold the fitted list."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli, synth
from oracle import twin as T

import eval_twin as E
import fit_twin as F
import sweep_twin as S
import test_gpu_sweep_confusables as CS
import test_gpu_sweep_weights as W

HAND_PATTERNS = CS.HAND_PATTERNS
GRID = (0.5, 0.8, 1.25, 2.0)
ONES = CS.ONES
START_ON = CS.weights_with(w0=1.1, w1=0.7, w8=1.3)   # the three patterns that match the row "abcdef" -> "abcdeg": the product's order matters
FIT_EXTRA = [("abcdeh", "abcdeg"), ("abcdex", "abcdeg"), ("abcdeh", "abcdef"), ("hous", "hose"), ("hous", "house"), ("hous", "hose"), ("housf", "house"),
             ("mousf", "mouse"), ("housx", "houses"), ("housx", "houses"), ("housx", "house"), ("abcdxg", "abcdeg"), ("abcdxg", "abcdxf"), ("abcdxg", "abcdeg")]
PAIRS = [(a, b) for a, b, _r, _k in E.HAND_PAIRS + E.HAND_PAIRS_STOP] + FIT_EXTRA


def counts_of_summary(s):
    return (int(s["rank_hist"][0]), int(s["reasons"][L.ANX_GOLD_RANKED]), int(s["rr_fixed"]))


def counts_of(c):
    return (int(c["at1"]), int(c["ranked"]), int(c["rr_fixed"]))


def sweep_counts(g, pairs, patterns, P, rows):
    """one counts triple per weight row: the existing sweep under P, late"""
    out = []
    for lo in range(0, len(rows), 256):
        part = [list(r) for r in rows[lo:lo + 256]]
        sums = g.evaluate_sweep_confusables_arrays([a for a, _ in pairs], [b for _, b in pairs], list(patterns), [P] * len(part), part)
        out += [counts_of_summary(s) for s in sums]
    return out


def sweep_table(g, pairs, patterns, P, cur, grid):
    """(counts under cur, table[j][g] = counts under "cur with w[j] = grid[g]") by the sweep: 1 + J * G sets"""
    J, G = len(patterns), len(grid)
    got = sweep_counts(g, pairs, patterns, P, [tuple(cur)] + [F.with_weight(cur, j, grid[x]) for j in range(J) for x in range(G)])
    return got[0], [[got[1 + j * G + x] for x in range(G)] for j in range(J)]


def fit(g, pairs, patterns, P, grid, **kw):
    return g.fit_confusables_arrays([a for a, _ in pairs], [b for _, b in pairs], list(patterns), P, list(grid), **kw)


def fit_table(g, pairs, patterns, P, grid, start):
    """round 0 of the fit: (start counts, trials[0] as a table of triples)"""
    _w, _rounds, res, trials = fit(g, pairs, patterns, P, grid, start=None if start is None else list(start), max_rounds=1, min_gain=0, with_trials=True)
    assert int(res[0]["n_trial_rounds"]) >= 1 and trials.shape[1:] == (len(patterns), len(grid))
    return counts_of(res[0]["start"]), [[counts_of(trials[0][j][x]) for x in range(len(grid))] for j in range(len(patterns))]


def assert_fit_equals_greedy(g, pairs, patterns, P, grid, start=None, objective="acc1", max_rounds=16, min_gain=1):
    """the whole fit against fit_twin.greedy over the sweep; -> the twin's result"""
    want = F.greedy(lambda rows: sweep_counts(g, pairs, patterns, P, rows), len(patterns), list(grid), start, objective, max_rounds, min_gain)
    gain = min_gain / 4294967296.0 if objective == "mrr" else min_gain   # the Python layer takes reciprocal-rank units for "mrr"
    weights, rounds, res, trials = fit(g, pairs, patterns, P, grid, start=None if start is None else list(start), objective=objective, max_rounds=max_rounds,
                                       min_gain=gain, with_trials=True)
    r = res[0]
    got_rounds = [(int(x["pattern"]), int(x["grid_index"]), float(x["weight"]).hex(), counts_of(x["counts"])) for x in rounds]
    assert got_rounds == [(j, x, float(w).hex(), c) for j, x, w, c in want["rounds"]]
    assert [float(w).hex() for w in weights] == [float(w).hex() for w in want["weights"]]
    assert (int(r["stop"]), int(r["n_rounds"]), int(r["n_trial_rounds"])) == (want["stop"], len(want["rounds"]), want["n_trial_rounds"])
    assert counts_of(r["start"]) == want["start"] and counts_of(r["final"]) == want["final"]
    assert trials.shape[0] == want["n_trial_rounds"]
    for t, table in enumerate(want["tables"]):
        assert [[counts_of(trials[t][j][x]) for x in range(len(grid))] for j in range(len(patterns))] == table, t
    return want


@pytest.fixture(scope="module")
def hand(data_dir, tmp_path_factory):
    alphabet = os.path.join(data_dir, "simple.alphabet.tsv")
    d = tmp_path_factory.mktemp("fithand")
    lex, flex = d / "hand.lexicon", d / "freq.lexicon"
    lex.write_text("\n".join(E.HAND_WORDS) + "\n")
    flex.write_text("".join("%s\t%d\n" % (w, 1 + (7 * i * i + 3 * i) % 23) for i, w in enumerate(E.HAND_WORDS)))
    return alphabet, str(lex), W.product_model(alphabet, str(lex), W.W_DEFAULT), str(flex), W.product_model(alphabet, str(flex), W.W_DEFAULT)


def hand_variants():
    """(name, parameters, on the lexicon with frequencies)"""
    return [("hand", E.hand_params(), False), ("n1", E.hand_params(max_matches=1, score_threshold=0.0), False),
            ("n2", E.hand_params(max_matches=2, score_threshold=0.0), False), ("n0", E.hand_params(max_matches=0, score_threshold=0.0), False),
            ("cut1.0", E.hand_params(cutoff_threshold=1.0), False), ("cut1.2", E.hand_params(cutoff_threshold=1.2), False),
            ("freq", E.hand_params(freq_weight=0.5), True), ("stop", E.hand_params(stop_at_exact_match=True), False)]


# ---- 1. the trial tables against the existing sweep ---------------------------------------------------------------------------------------
def test_trial_tables_against_the_sweep(hand):
    _alphabet, _lex, plain, _flex, fplain = hand
    above = below = ranked_moves = 0
    for name, Pt, freq in hand_variants():
        g, P = fplain if freq else plain, W.product_params(Pt)
        for start in (ONES, START_ON):
            now, table = sweep_table(g, PAIRS, HAND_PATTERNS, P, start, GRID)   # 49 sets: the reference side
            flat = [c for row in table for c in row]
            above += sum(c[0] > now[0] for c in flat)
            below += sum(c[0] < now[0] for c in flat)
            ranked_moves += sum(c[1] != now[1] for c in flat)
            got_now, got = fit_table(g, PAIRS, HAND_PATTERNS, P, GRID, None if start is ONES else start)
            assert got_now == now, (name, start)
            assert got == table, (name, start)
    # what the sweep says of these inputs: weights gain and lose a first rank, and the cutoff moves pairs in and out of the list
    assert above > 0 and below > 0 and ranked_moves > 0


# ---- 2. whole fits against the Python greedy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", ["acc1", "mrr"])
def test_whole_fits_against_the_greedy(hand, objective):
    _alphabet, _lex, plain, _flex, _fplain = hand
    for Pt in (E.hand_params(), E.hand_params(cutoff_threshold=1.2)):
        P = W.product_params(Pt)
        free = assert_fit_equals_greedy(plain, PAIRS, HAND_PATTERNS, P, GRID, objective=objective, min_gain=0)
        assert len(free["rounds"]) >= 2 and free["stop"] == 0   # the inputs do real work
        assert_fit_equals_greedy(plain, PAIRS, HAND_PATTERNS, P, GRID, objective=objective, min_gain=1)
        one = assert_fit_equals_greedy(plain, PAIRS, HAND_PATTERNS, P, GRID, objective=objective, min_gain=0, max_rounds=1)
        assert one["stop"] == 1 and len(one["rounds"]) == 1
    assert_fit_equals_greedy(plain, PAIRS, HAND_PATTERNS, W.product_params(E.hand_params()), GRID, start=START_ON, objective=objective, min_gain=0)


# ---- 3. the final counts against a product model that holds the fitted list ----------------------------------------------------------------
def test_final_counts_against_a_product_model(hand, tmp_path, capsys):
    alphabet, lex, plain, _flex, _fplain = hand
    a, b = [x for x, _ in PAIRS], [y for _, y in PAIRS]
    for Pt in (E.hand_params(), E.hand_params(cutoff_threshold=1.2)):
        P = W.product_params(Pt)
        weights, rounds, res = fit(plain, PAIRS, HAND_PATTERNS, P, GRID, min_gain=0)
        assert len(rounds) >= 1
        m = CS.product_model(alphabet, lex, HAND_PATTERNS, [float(w) for w in weights], False)
        want = S.summarize(m.evaluate_arrays(a, b, P))
        assert counts_of(res[0]["final"]) == (want["rank_hist"][0], want["reasons"][E.RANKED], want["rr_fixed"])
    # the command line: --fit-output, then read_confusablelist into a fresh model
    pairs = [p for p in PAIRS if p[0] and p[1] and len(p[1]) < 100]
    inp, cand, out = tmp_path / "pairs.tsv", tmp_path / "cand.tsv", tmp_path / "fitted.tsv"
    inp.write_text("".join("%s\t%s\n" % p for p in pairs))
    cand.write_text("".join("%s\t1.0\n" % p for p in HAND_PATTERNS))
    argv = ["sweep", "-a", alphabet, "-l", lex, "-k", "2", "-d", "1", "-n", "3", "-t", "0.71", "-T", "0", "--device", "0", "--candidates", str(cand),
            "--candidate-weights", ",".join(repr(x) for x in GRID), "--fit", "--fit-min-gain", "0", "--fit-output", str(out), str(inp)]
    assert cli.main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    P = W.product_params(E.hand_params())
    d = plain.fit_confusables([x for x, _ in pairs], [y for _, y in pairs], list(HAND_PATTERNS), P, list(GRID), min_gain=0)
    assert len(lines) == 2 + len(d["rounds"]) >= 3 and lines[0].split("\t")[0] == "-" and lines[-1].startswith("# stop:")
    assert [ln.split("\t")[0] for ln in lines[1:-1]] == [r["pattern"] for r in d["rounds"]]
    assert lines[-2] == cli.fit_tsv_line(d["rounds"][-1]["pattern"], d["rounds"][-1]["weight"], d["rounds"][-1])
    assert out.read_text() == cli.fit_list_text(d["weights"]) and d["weights"]
    fresh = A.VariantModel(alphabet, W.product_weights(W.W_DEFAULT), device=0)
    fresh.read_lexicon(lex)
    fresh.read_confusablelist(str(out))
    fresh.build()
    want = S.summarize(fresh.evaluate_arrays([x for x, _ in pairs], [y for _, y in pairs], P))
    assert (d["final"]["at1"], d["final"]["ranked"], d["final"]["rr_fixed"]) == (want["rank_hist"][0], want["reasons"][E.RANKED], want["rr_fixed"])
    assert d["final"]["accuracy_at_1"] == want["rank_hist"][0] / len(pairs)


# ---- eng.aspell ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(data_dir):
    alphabet, lexicon = os.path.join(data_dir, "simple.alphabet.tsv"), os.path.join(data_dir, "eng.aspell.lexicon")
    return alphabet, lexicon, synth.load_lexicon_words(lexicon)


# ---- 4. ties in masses, lists beyond 128 rows ----------------------------------------------------------------------------------------------
def test_ties_and_long_lists(eng):
    alphabet, lexicon, _words = eng
    plain = W.product_model(alphabet, lexicon, W.W_LCS)   # lcs only: scores tie in masses
    ratio = (("ratio", 1.0), ("ratio", 1.0))
    P = W.product_params(T.SearchParameters(ratio[0], ratio[1], 0, 0.0, 0.0, False, 0.0))   # every row kept and ranked
    # (three-letter inputs: lists of hundreds of rows; a longer input's list of thousands costs the sweep's stable re-sort a second per set)
    pairs = [("cat", "cut"), ("cat", "cats"), ("cat", "act"), ("teh", "the"), ("teh", "ten"), (W.NONE_INPUTS[0], "cat")]
    rec = plain.evaluate_arrays([a for a, _ in pairs], [b for _, b in pairs], P)
    assert max(int(x) for x in rec["n_results"]) > 128 and sum(int(r) > 0 for r in rec["rank"]) >= 2   # long lists, gold inside them
    grid = (0.8, 1.25)
    for Pt in (P, W.product_params(T.SearchParameters(ratio[0], ratio[1], 0, 0.0, 1.05, False, 0.0))):
        now, table = sweep_table(plain, pairs, CS.ENG_PATTERNS, Pt, (1.0,) * 12, grid)
        assert any(c != now for row in table for c in row)
        assert fit_table(plain, pairs, CS.ENG_PATTERNS, Pt, grid, None) == (now, table)


# ---- 5. chunk seams --------------------------------------------------------------------------------------------------------------------------
def test_chunk_seams(hand):
    _alphabet, _lex, plain, _flex, _fplain = hand
    P = W.product_params(E.hand_params(cutoff_threshold=1.2))
    before = A.VariantModel.fit_stats()
    whole = fit(plain, PAIRS, HAND_PATTERNS, P, GRID, min_gain=0, with_trials=True)
    mid = A.VariantModel.fit_stats()
    assert (mid["calls"] - before["calls"], mid["chunks"] - before["chunks"]) == (1, 1)
    assert mid["rounds"] - before["rounds"] == int(whole[2][0]["n_trial_rounds"]) == mid["trial_launches"] - before["trial_launches"]
    assert 0 < mid["state_pairs"] - before["state_pairs"] <= len(PAIRS) and mid["state_slots"] - before["state_slots"] >= mid["state_pairs"] - before["state_pairs"]
    assert len(whole[1]) >= 2
    for chunk in (3, 7):
        cut = fit(plain, PAIRS, HAND_PATTERNS, P, GRID, min_gain=0, with_trials=True, chunk=chunk)
        for x, y in zip(whole, cut):
            assert x.tobytes() == y.tobytes(), chunk
    ptr = fit(plain, PAIRS, HAND_PATTERNS, P, GRID, min_gain=0, with_trials=True, packed=False)
    for x, y in zip(whole, ptr):
        assert x.tobytes() == y.tobytes()
    with pytest.raises(A.AnxError):
        fit(plain, PAIRS, HAND_PATTERNS, P, GRID, chunk=0)


# ---- 6. replicas, host masks, an input the lane memory cannot hold ---------------------------------------------------------------------------
def test_replicas_and_host_masks(data_dir, tmp_path):
    alphabet = os.path.join(data_dir, "simple.alphabet.tsv")
    long1 = ("abcde" * 13)[:64]
    lex = tmp_path / "long.lexicon"
    lex.write_text("\n".join(E.HAND_WORDS + [long1]) + "\n")
    patterns = HAND_PATTERNS + ("-[s]",)
    pairs = PAIRS + [(long1 + "s", long1), (long1 + "s", "abcdef")]
    assert len(pairs[-2][0]) == 65
    P = W.product_params(E.hand_params(max_matches=2, score_threshold=0.0))
    plain = W.product_model(alphabet, str(lex), W.W_DEFAULT)
    now, table = sweep_table(plain, pairs, patterns, P, (1.0,) * 13, GRID)
    s0 = A.VariantModel.conf_sweep_stats()
    one = fit(plain, pairs, patterns, P, GRID, min_gain=0, with_trials=True)
    s1 = A.VariantModel.conf_sweep_stats()
    assert s1["rows_patched"] - s0["rows_patched"] >= 1   # the long input's row: its mask came from the host
    got = one[3][0]
    assert counts_of(one[2][0]["start"]) == now and [[counts_of(got[j][x]) for x in range(len(GRID))] for j in range(13)] == table
    two = W.product_model(alphabet, str(lex), W.W_DEFAULT)
    two.to_devices([0, 0])
    assert two.num_replicas == 2
    for x, y in zip(one, fit(two, pairs, patterns, P, GRID, min_gain=0, with_trials=True)):
        assert x.tobytes() == y.tobytes()
    L.set_switch("ANX_CONFUSABLES", "host")
    try:
        hosted = fit(plain, pairs, patterns, P, GRID, min_gain=0, with_trials=True)
        assert A.VariantModel.conf_sweep_stats()["rows_host_mode"] > s1["rows_host_mode"]
    finally:
        L.set_switch("ANX_CONFUSABLES", None)
    for x, y in zip(one, hosted):
        assert x.tobytes() == y.tobytes()


# ---- 7. a full-size lexicon ------------------------------------------------------------------------------------------------------------------
def test_eng_mined_patterns(eng):
    alphabet, lexicon, words = eng
    plain = W.product_model(alphabet, lexicon, W.W_DEFAULT)
    pairs = E.edited_pairs(words, 2000, seed=7)
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    patterns = [r["pattern"] for r in plain.mine_confusables(a, b) if r["representable"]][:8]
    assert len(patterns) == 8
    grid = (0.8, 1.25)
    P = W.product_params(T.SearchParameters(("abs", 3), ("abs", 2), 10, 0.25, 2.0, False, 0.0))
    start = plain.evaluate_sweep_confusables_arrays(a, b, patterns, [P], [[1.0] * 8])[0]
    assert int(start["n"]) == len(pairs) and int(start["reasons"][L.ANX_GOLD_RANKED]) * 2 >= len(pairs)   # gold is in the cropped list of half the pairs at least
    now, table = sweep_table(plain, pairs, patterns, P, (1.0,) * 8, grid)
    assert now == counts_of_summary(start) and any(c[0] != now[0] for row in table for c in row)
    assert fit_table(plain, pairs, patterns, P, grid, None) == (now, table)
    assert_fit_equals_greedy(plain, pairs, patterns, P, grid, min_gain=1, max_rounds=4)
