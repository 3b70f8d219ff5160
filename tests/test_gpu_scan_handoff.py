"""The scan's path from hit masks to pair-list slots (kernels_scan.hpp: process(), the LDS hit list, flush(), WaveOut).

Tiles that stream an adjacency list count the hits of rows whose record length fails the DL's length test where they are found
and keep them out of the hit list; the list holds entry ids, so it is expanded when the next chunk could overflow it and not
after every chunk; a wave's pair-list reservations start at ANX_SCAN_CHUNK_FIRST slots and double up to the chunk.  None of it
may change a result: every case runs at the default and with ANX_SCAN_CHUNK_FIRST at the cap (flat reservations, as before),
against the CPU oracle.

1. Counts and rows for (k, d) with four, two and no count-only sections, on queries at the edges: lengths 1-3 (sections of
   length < 1 are empty), 14-16 symbols cut from 17-19-symbol words (candidates beyond 16 symbols: the not-fused wide path), one
   signature 32 and 33 times (a full tile; a full tile plus a tile of one), 200 copies of the heaviest query of a lexicon sample
   (the hit list passes the deferred-flush bound several times in a tile).
2. A model with a 7-group signature at ANX_SCAN_TQ=64: two passes per chunk, where the list is still expanded after every chunk.
3. The growing reservations leave fewer pair-list slots than the flat ones, and nothing else differs.
4. A batch sized from the hints of a light batch overflows its pair list, is regrown and repeated once.
5. The small call (k_scan_small shares scan_tile and its LDS arrays): 1 and 64 inputs."""
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import synth
from oracle import cwrap as O

CAP = 256   # >= the chunk of every tile (256; 128 in tiles that run the fused filter): the first reservation is a whole chunk


def _models(data_dir, groups=None):
    alphabet, lexicon = os.path.join(data_dir, "simple.alphabet.tsv"), os.path.join(data_dir, "eng.aspell.lexicon")
    A.set_switch("ANX_SIG_GROUPS", groups)   # read when the index is built
    try:
        g = A.VariantModel(alphabet, A.Weights(), device=0)
        g.read_lexicon(lexicon)
        g.build()
    finally:
        A.set_switch("ANX_SIG_GROUPS", None)
    return g


@pytest.fixture(scope="module")
def eng(data_dir):
    g = _models(data_dir)
    o = O.OracleModel(alphabet_path=os.path.join(data_dir, "simple.alphabet.tsv"))
    o.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    o.build()
    words = [w for w in synth.load_lexicon_words(os.path.join(data_dir, "eng.aspell.lexicon")) if w.isascii() and w.isalpha()]
    return g, o, words


def _run(g, qs, p, counts=False):
    b = g.encode_batch(qs, p)
    try:
        b.run()
        out = [b.fetch_arrays(), b.stats()]
        if counts:
            out.append(b.pair_counts())   # the GEN instance of the scan: per-query counts, the list's count-only flag
        return out
    finally:
        b.free()


def _both(fn):
    """fn() at the default and with flat reservations"""
    res = []
    for first in (None, CAP):
        A.set_switch("ANX_SCAN_CHUNK_FIRST", first)
        try:
            res.append(fn())
        finally:
            A.set_switch("ANX_SCAN_CHUNK_FIRST", None)
    return res


def _assert_oracle(arrays, qs, oracle, idx=None):
    off, vid, dist, freq = arrays
    counts, ovid, odist, ofreq = oracle
    idx = np.arange(len(qs)) if idx is None else idx
    return O.assert_rows_equal(off, vid, dist, freq, idx, counts, ovid, odist, ofreq, what=lambda i: qs[i])


@pytest.fixture(scope="module")
def edge_queries(eng):
    g, _o, words = eng
    rng = random.Random(41)
    short = [w for w in words if len(w) <= 3]
    qs = rng.sample(short, min(150, len(short))) + ["".join(rng.choice("aeiostrn") for _ in range(rng.randint(1, 3))) for _ in range(150)]
    for w in [w for w in words if 17 <= len(w) <= 19]:   # (180 words) 14-16 symbols, 1-5 deletions away from a 17-19-symbol word
        cs = list(w)
        while len(cs) > 16 or (len(cs) > 14 and rng.random() < 0.5):
            del cs[rng.randrange(len(cs))]
        qs.append("".join(cs))
    mid = [w for w in words if 5 <= len(w) <= 8]
    qs += [mid[100]] * 32 + [mid[2000]] * 33
    # the heaviest query (scored pairs at k = 3) of a sample of the lexicon's own words
    sample = mid[::3]
    _arr, _st, pc = _run(g, sample, A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10), counts=True)
    heavy = sample[int(np.argmax(pc))]
    # 32 copies in a tile hit the same records, one list entry each: more than 1 200 scored pairs, most of them within the length
    # test, pass the bound of 256 waiting entries three times or more
    assert int(pc.max()) > 1200, (heavy, int(pc.max()))
    qs += [heavy] * 200
    qs += synth.make_queries(words, 1000, max_len=16, seed=43)
    rng.shuffle(qs)
    return qs


@pytest.mark.parametrize("k,d", [(3, 2), (3, 1), (3, 3), (2, 2), (1, 1)])
def test_counts_and_rows_against_the_oracle(eng, edge_queries, k, d):
    g, o, _words = eng
    qs = edge_queries
    p = A.SearchParameters(max_anagram_distance=k, max_edit_distance=d, max_matches=10, score_threshold=0.25, cutoff_threshold=2.0)
    counts, ovid, odist, ofreq, opairs, _cls = O.batch_rows(o, qs, O.make_params(("abs", k), ("abs", d), 10, 0.25, 2.0), nthreads=16, stride=16)
    for arrays, st, pc in _both(lambda: _run(g, qs, p, counts=True)):
        assert st["n_adj_tiles"] > 0.9 * st["n_scan_blocks"]
        assert st["n_pairs"] == int(pc.sum()) == opairs
        assert _assert_oracle(arrays, qs, (counts, ovid, odist, ofreq)) > len(qs)


def test_two_passes_per_chunk(data_dir, eng):
    _g, o, words = eng
    g7 = _models(data_dir, groups=7)
    rng = random.Random(7)
    mid = [w for w in words if 5 <= len(w) <= 8]
    # groups of 40-64 equal signatures (tiles of more than 32 queries: two passes) among ordinary queries
    qs = synth.make_queries(words, 2400, max_len=16, seed=47)
    for w, n in zip(rng.sample(mid, 11), (33, 40, 48, 63, 64, 64, 65, 50, 57, 60, 56)):
        qs += [w] * n
    qs = qs[:3000]
    rng.shuffle(qs)
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10, score_threshold=0.25, cutoff_threshold=2.0)
    counts, ovid, odist, ofreq, opairs, _cls = O.batch_rows(o, qs, O.make_params(("abs", 3), ("abs", 2), 10, 0.25, 2.0), nthreads=16, stride=16)
    A.set_switch("ANX_SCAN_TQ", 64)   # read when the tiles are cut
    try:
        for arrays, st in _both(lambda: _run(g7, qs, p)):
            assert st["n_pairs"] == opairs
            assert _assert_oracle(arrays, qs, (counts, ovid, odist, ofreq)) > len(qs)
    finally:
        A.set_switch("ANX_SCAN_TQ", None)


def test_growing_reservations_leave_fewer_slots(eng):
    g, _o, words = eng
    qs = synth.make_queries(words, 50_000, max_len=16, seed=synth.SEED)
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
    (grow, st), (flat, st0) = _both(lambda: _run(g, qs, p))
    assert st["n_pair_slots"] < st0["n_pair_slots"], (st["n_pair_slots"], st0["n_pair_slots"])
    for key in ("n_pairs", "n_survivors", "n_class_tests", "n_prefiltered_in_scan"):
        assert st[key] == st0[key], key
    for x, y in zip(grow, flat):
        assert np.array_equal(x, y)


def test_hinted_batch_regrows_once(eng):
    g, o, words = eng
    rng = random.Random(5)
    light = ["".join(rng.choice("qxzjvkw") for _ in range(rng.randint(10, 16))) for _ in range(4096)]   # hardly a candidate each
    heavy = synth.make_queries(words, 40_000, max_len=12, seed=53)
    # parameters no other test of the module uses: the hints hold the light batch's fills and nothing else
    kw = dict(max_anagram_distance=3, max_edit_distance=2, max_matches=10, score_threshold=0.26, cutoff_threshold=2.0)
    p = A.SearchParameters(**kw)
    idx = np.arange(0, len(heavy), 20)
    counts, ovid, odist, ofreq, _tp, _cls = O.batch_rows(o, [heavy[i] for i in idx], O.make_params(("abs", 3), ("abs", 2), 10, 0.26, 2.0), nthreads=16, stride=16)
    A.set_switch("ANX_HINTS", "0")
    try:
        ref, st_ref = _run(g, heavy, p)
    finally:
        A.set_switch("ANX_HINTS", None)

    def hinted():
        _arr, st_light = _run(g, light, p)        # its first run records the hints
        assert st_light["n_pair_slots"] * 8 < st_ref["n_pair_slots"]
        L.kernel_timer(True)
        try:
            got, st = _run(g, heavy, p)
            _ms, launches = L.kernel_time("k_scan")
        finally:
            L.kernel_timer(False)
        return got, st, launches
    for got, st, launches in _both(hinted):
        assert launches == 2                      # the hinted pair list overflowed: regrown, one repeat
        assert st["n_pairs"] == st_ref["n_pairs"] and st["n_survivors"] == st_ref["n_survivors"]
        for x, y in zip(got, ref):
            assert np.array_equal(x, y)
        assert _assert_oracle(got, heavy, (counts, ovid, odist, ofreq), idx) > len(idx)


@pytest.mark.parametrize("n", [1, 64])
def test_small_call(eng, edge_queries, n):
    g, o, _words = eng
    qs = [q for q in edge_queries if len(q) >= 4][:n]
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10, score_threshold=0.25, cutoff_threshold=2.0)
    op = O.make_params(("abs", 3), ("abs", 2), 10, 0.25, 2.0)
    exp = [o.find_variants(q, op) for q in qs]
    for got in _both(lambda: g.find_variants_ids(qs, p)):
        assert got == exp
