"""Queries with equal count vectors in one scan tile (csrc/scan_twins.hpp, kernels_scan.hpp): the production bit-plane scan
tests a run of equal thermometer planes once and copies the leader's hit bit onto its followers; both encoders sort equal planes
next to each other.  Every (query, entry) pair is still materialised, band-tested and scored on its own, so nothing a caller
sees may change.  Small models from a handful of words; for every case

  * the ranked rows are == the C oracle's,
  * n_pairs == the sum of anx_batch_pair_counts (the general scan instance, which shares nothing),
  * rows and statistics are identical with ANX_SCAN_TWINS=0 (every query its own leader).

Two models: the default signature groups, and ONE signature group (ANX_SIG_GROUPS=1: the signature is the length, so every
word of a length lands in the same tile and the test composes the tile -- kinds, runs, what comes first and last)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import synth
from oracle import cwrap as O

STAT_KEYS = ("n_pairs", "n_survivors", "n_selected", "n_class_tests", "n_prefiltered_in_scan")
K, D, N = 3, 2, 10

# anagram sets of six letters: kind 1 (no letter twice) and kind 2 (a doubled letter)
LISTEN = ["listen", "silent", "enlist", "tinsel", "inlets"]
MASTER = ["master", "stream", "tamers"]
DANGER = ["danger", "garden", "gander"]
DETEST = ["detest", "tested"]
LETTER = ["letter"]
SINGLES = ["planet", "forest", "bridge", "copied", "jumble"]
LEXICON = LISTEN + MASTER + DANGER + DETEST + LETTER + SINGLES + [
    "listens", "listed", "list", "lists", "inlet", "stone", "notes", "onset", "liste", "silents", "tinsels", "masters", "streams",
    "dangers", "gardens", "tester", "detests", "letters", "latter", "litter", "planets", "forests", "bridges", "lister", "linted",
    "minted", "salted", "tilted", "sifted", "lasted", "mister", "muster", "garner", "grader", "danker", "hanger", "ranged"]


def _pair(tmp_path_factory, data_dir, words, name):
    lex = tmp_path_factory.mktemp(name) / "small.lexicon"
    lex.write_text("".join(f"{w}\t{1 + i % 7}\n" for i, w in enumerate(words)), encoding="utf-8")
    alpha = os.path.join(data_dir, "simple.alphabet.tsv")
    g = A.VariantModel(alpha, A.Weights(), device=0)
    g.read_lexicon(str(lex))
    g.build()
    o = O.OracleModel(alphabet_path=alpha)
    o.read_lexicon(str(lex))
    o.build()
    return g, o


@pytest.fixture(scope="module")
def small(tmp_path_factory, data_dir):
    return _pair(tmp_path_factory, data_dir, LEXICON, "twins")


@pytest.fixture(scope="module")
def one_group(tmp_path_factory, data_dir):
    """one signature group: all queries of a length share the tile (the groups are chosen when the model is built)"""
    A.set_switch("ANX_SIG_GROUPS", "1")
    try:
        return _pair(tmp_path_factory, data_dir, LEXICON, "twins1")
    finally:
        A.set_switch("ANX_SIG_GROUPS", None)


@pytest.fixture(scope="module")
def generated(tmp_path_factory, data_dir):
    """a sample of the English lexicon and the benchmark generator's queries over it: repeated words, zero-edit queries and
    transpositions give the tiles their twins"""
    words = synth.load_lexicon_words(os.path.join(data_dir, "eng.aspell.lexicon"))[::40]
    g, o = _pair(tmp_path_factory, data_dir, words, "twinsgen")
    return g, o, synth.make_queries(words, 4000, max_len=16, seed=synth.SEED)


GP = A.SearchParameters(max_anagram_distance=K, max_edit_distance=D, max_matches=N)
OP = O.make_params(("abs", K), ("abs", D), N, 0.25, 2.0)


def _run(b):
    b.run()
    st = b.stats()
    return b.fetch(), {k: st[k] for k in STAT_KEYS}, st


def check(g, o, queries, sample=1, switches=()):
    """the three properties of the module docstring; -> (rows, full statistics of the default run)"""
    try:
        for name, value in switches:
            A.set_switch(name, value)
        b = g.encode_batch(queries, GP)   # the tile switches are read when the tiles are built
        try:
            rows, stats, full = _run(b)
            A.set_switch("ANX_SCAN_TWINS", "0")   # read by every run
            rows0, stats0, _ = _run(b)
            A.set_switch("ANX_SCAN_TWINS", None)
            counts = b.pair_counts()
        finally:
            b.free()
    finally:
        A.set_switch("ANX_SCAN_TWINS", None)
        for name, _ in switches:
            A.set_switch(name, None)
    assert rows == rows0
    assert stats == stats0
    assert int(counts.sum()) == stats["n_pairs"]
    for i in range(0, len(queries), sample):
        assert rows[i] == o.find_variants(queries[i], OP), queries[i]
    return rows, full


def test_anagram_twins_with_different_strings(small):
    """five anagrams and transpositions of them: one count vector, one run, every string scored on its own"""
    g, o = small
    qs = LISTEN + ["lisetn", "isletn", "tinsle", "enlits", "slient"]
    rows, st = check(g, o, qs)
    assert st["n_scan_blocks"] == 1                      # one tile: one (length, signature) group of ten
    assert len({tuple(r) for r in rows[:5]}) == 5        # the same classes hit, different rows
    assert all(rows[i] and g.vocab_text(rows[i][0][0]) == LISTEN[i] for i in range(5))


@pytest.mark.parametrize("n", [32, 33])
def test_one_word_fills_a_tile(small, n):
    """32 times: a run of 31 followers (five doubling steps); 33 times: the run is cut by the tile"""
    g, o = small
    rows, st = check(g, o, ["listen"] * n)
    assert st["n_scan_blocks"] == (n + 31) // 32
    assert all(r == rows[0] for r in rows)


def test_run_meets_the_pass_boundary(small):
    """tiles of 64 (ANX_SCAN_TQ): 40 equal queries in one tile, the run is cut at query 32 where the second pass begins"""
    g, o = small
    rows, st = check(g, o, ["listen"] * 40, switches=(("ANX_SCAN_TQ", "64"),))
    assert st["n_scan_blocks"] == 1
    assert all(r == rows[0] for r in rows)


def test_twins_first_and_last_in_the_tile(one_group):
    """every count vector of the tile twice or more: whatever order the hash gives the runs, the first queries of the tile are a run
    and the last ones are"""
    g, o = one_group
    qs = [w for ws in zip(LISTEN, MASTER + MASTER[:2], DANGER + DANGER[:2]) for w in ws]   # interleaved in the input
    rows, st = check(g, o, qs)
    assert st["n_scan_blocks"] == 1


def test_tile_without_twins(one_group):
    g, o = one_group
    rows, st = check(g, o, ["listen", "master", "danger"] + SINGLES)
    assert st["n_scan_blocks"] == 1


def test_runs_on_both_sides_of_a_kind_boundary(one_group):
    """one tile, queries sorted by kind: the kind-1 queries are ONE run and the kind-2 queries (a doubled letter) another, so the
    boundary has a run on either side; then the same with single queries around them"""
    g, o = one_group
    rows, st = check(g, o, ["silent", "detest", "listen", "tested", "enlist", "detest"])
    assert st["n_scan_blocks"] == 1 and st["n_tests_kind"][1] > 0 and st["n_tests_kind"][2] > 0
    rows, st = check(g, o, ["silent", "detest", "listen", "tested", "enlist", "detest", "letter", "planet", "letter", "forest"])
    assert st["n_scan_blocks"] == 1


def _both_encoders(g, qs):
    out = {}
    for mode in ("device", "host"):
        A.set_switch("ANX_ENCODE", "host" if mode == "host" else None)
        try:
            b = g.encode_batch(qs, GP)
            b.run()
            st = b.stats()
            out[mode] = (b.fetch_arrays(), st, b.pair_counts())
            b.free()
        finally:
            A.set_switch("ANX_ENCODE", None)
    return out


def test_host_and_device_encoder_order_queries_alike(generated):
    """the statistics that only agree when both encoders order and tile the queries identically (as tests/test_gpu_encode.py),
    and each encoder's rows against the oracle on a sample"""
    g, o, qs = generated
    out = _both_encoders(g, qs)
    (da, ds, dc), (ha, hs, hc) = out["device"], out["host"]
    for x, y in zip(da, ha):
        assert np.array_equal(x, y)
    for k in ("n_queries", "n_pairs", "n_class_tests", "n_scan_blocks", "n_results", "n_survivors", "n_selected", "n_prefiltered_in_scan"):
        assert ds[k] == hs[k], k
    assert list(ds["n_tests_kind"]) == list(hs["n_tests_kind"])
    assert np.array_equal(dc, hc)
    assert ds["n_adj_tiles"] > 0
    for mode in ("device", "host"):
        check(g, o, qs, sample=37, switches=(("ANX_ENCODE", "host"),) if mode == "host" else ())


def test_tiles_without_a_list_take_k_scan_bits(generated):
    g, o, qs = generated
    rows, st = check(g, o, qs, sample=41, switches=(("ANX_SCAN_ADJ", "0"),))
    assert st["n_adj_tiles"] == 0 and st["n_scan_blocks"] > 100


def test_small_call_with_repeats(generated):
    """the small call: one tile per query (no run can form), input order kept"""
    g, o, qs = generated
    q64 = (qs[:24] + qs[:8] + ["listen"] * 16 + qs[24:40])[:64]
    assert len(q64) == 64
    got = g.find_variants_ids(q64, GP)
    try:
        A.set_switch("ANX_SCAN_TWINS", "0")
        got0 = g.find_variants_ids(q64, GP)
    finally:
        A.set_switch("ANX_SCAN_TWINS", None)
    assert got == got0
    for q, r in zip(q64, got):
        assert [tuple(x) for x in r] == o.find_variants(q, OP), q
