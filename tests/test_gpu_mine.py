"""anx_mine_confusables on the device (mine.hip: k_mine_script, the sort / representative / reduce histogram, k_mine_emit): the table
and the site list `==` the twin (tests/mine_twin.py) on hand-made pairs and on the CPU test's 20 000 random pairs; malformed bytes
`==` the host path; narrowed site hashes, small chunks and sites=False change nothing; what the counters say about pairs the device
hands back; and the mined patterns, one at a time as a confusable list, weigh the pairs they came from."""
import os

import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import synth
from oracle.sesdiff_twin import Confusable
import mine_twin as MT

CF_MAXCP, CF_DIFFS = 64, 48  # conf_lane.hpp: code points a side and diffs of a script the lane memory holds


@pytest.fixture(scope="module")
def model(data_dir):
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    g.build()
    return g


@pytest.fixture(scope="module")
def pairs(data_dir):
    eng = synth.load_lexicon_words(os.path.join(data_dir, "eng.aspell.lexicon"))
    nld = synth.load_lexicon_words(os.path.join(data_dir, "nld.aspell.lexicon"))
    return MT.random_pairs(eng, nld, 20000)


def mine(g, pr, counts=None, context=0, anchors=False, sites=True):
    return MT.lib_result(g.mine_confusables_arrays([a for a, _ in pr], [b for _, b in pr], counts, context=context, anchors=anchors,
                                                   sites=sites), with_sites=sites)


def delta(before):
    after = A.VariantModel.mine_stats()
    return {k: after[k] - before[k] for k in after}


def many_instructions():
    """a pair of at most 64 code points a side whose script has more instructions than the diff stack holds: identities of two letters
    between one-character deletions and insertions in turn"""
    a = b = ""
    for k in range(25):
        two = chr(ord("a") + k) * 2
        a += two + ("1" if k % 2 == 0 else "")
        b += two + ("" if k % 2 == 0 else "2")
    assert len(a) <= CF_MAXCP and len(b) <= CF_MAXCP and len(MT.script(a, b)) > CF_DIFFS
    return a, b


HAND = [
    ("huis", "huis"), ("", "abc"), ("abc", ""), ("", ""),                          # equal; empty a; empty b; both empty
    ("huys", "huis"), ("abcd", "abdc"), ("xhuysx", "yhuisy"),                      # a substitution; a transposition; sites first and last
    ("abcdefghijkl", "abXdefgYijkZ"),                                              # three sites
    ("abcabc", "abdabd"),                                                          # the same site twice in one pair
    ("café", "cafe"),
    ("a" * 62 + "x", "a" * 62 + "y"), ("a" * 63 + "x", "a" * 63 + "y"),          # 63 and 64 code points
    ("é" * 63 + "x", "é" * 63 + "y"),                                              # 64 code points in 127 bytes
    ("a]b", "a[b"), ("a|b", "ab"), ("x[y", "xy"),
]


def test_hand_pairs(model):
    counts = [(0, 0xFFFFFFFF, 3)[k % 3] for k in range(len(HAND))]
    for context, anchors in MT.GRID:
        before = A.VariantModel.mine_stats()
        assert mine(model, HAND, None, context, anchors) == MT.twin_result(HAND, None, context, anchors), (context, anchors)
        assert mine(model, HAND, counts, context, anchors) == MT.twin_result(HAND, counts, context, anchors), (context, anchors)
        d = delta(before)
        assert d["device_pairs"] == 2 * len(HAND) and d["host_pairs"] == 0 and d["odd_shape_pairs"] == 0
    table = model.mine_confusables([a for a, _ in HAND], [b for _, b in HAND])
    assert {t["pattern"] for t in table if not t["representable"]} == {"-[]]+[[]", "-[|]", "-[[]"}


def test_pairs_the_device_hands_back(model):
    long_pair = ("a" * 64 + "x", "a" * 64 + "y")  # 65 code points
    pr = [("huys", "huis"), long_pair, ("cat", "kat"), many_instructions(), ("huys", "huis")]
    before = A.VariantModel.mine_stats()
    for context, anchors in MT.GRID:
        assert mine(model, pr, [1, 2, 3, 4, 5], context, anchors) == MT.twin_result(pr, [1, 2, 3, 4, 5], context, anchors)
    d = delta(before)
    assert d["host_pairs"] == 2 * len(MT.GRID) and d["device_pairs"] == 3 * len(MT.GRID) and d["odd_shape_pairs"] == 0


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_small_calls(model, pairs, n):
    pr, counts = pairs[0][:n], pairs[1][:n]
    assert mine(model, pr, counts, 1, True) == MT.twin_result(pr, counts, 1, True)


def test_malformed_bytes_equal_the_host_path(model):
    bad = [b"ab\x80cd", b"ab\xc3", b"\xc0\xafxy", b"\xe0\x80\xafz", b"\xf8\x88\x80\x80\x80", b"a\xe2\x82", b"\xc1\x81bc", b"\xf0\x9f\x98", b"Abc"]
    a = [x for x in bad for _ in bad]
    b = [y for _ in bad for y in bad]
    for context, anchors in ((0, False), (2, True)):
        dev = model.mine_confusables_arrays(a, b, context=context, anchors=anchors, sites=True)
        L.set_switch("ANX_MINE", "host")
        try:
            host = model.mine_confusables_arrays(a, b, context=context, anchors=anchors, sites=True)
        finally:
            L.set_switch("ANX_MINE", None)
        assert dev["text"] == host["text"]
        for k in ("text_off", "count", "sites", "flags", "site_off", "site"):
            assert dev[k].tolist() == host[k].tolist(), k


@pytest.mark.parametrize("context,anchors", MT.GRID)
@pytest.mark.parametrize("counted", [False, True])
def test_random_pairs_equal_the_twin(model, pairs, context, anchors, counted):
    pr, counts = pairs
    cnt = counts if counted else None
    before = A.VariantModel.mine_stats()
    got = mine(model, pr, cnt, context, anchors)
    want = MT.twin_result(pr, cnt, context, anchors)
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    d = delta(before)
    assert d["device_pairs"] == len(pr) and d["host_pairs"] == 0 and d["sites"] == len(want[2]) and d["collision_runs"] == 0


def test_narrow_hash_changes_nothing(model, pairs):
    pr, counts = pairs[0][:2500], pairs[1][:2500]
    want = MT.twin_result(pr, counts, 1, True)
    L.set_switch("ANX_MINE_HASH_BITS", 4)
    try:
        before = A.VariantModel.mine_stats()
        assert mine(model, pr, counts, 1, True) == want
        d = delta(before)
    finally:
        L.set_switch("ANX_MINE_HASH_BITS", None)
    assert 1 <= d["collision_runs"] <= 16  # (16 hash values, more than a thousand texts)
    assert len(want[0]) > 1000


def test_chunks_and_no_sites(model, pairs):
    pr, counts = pairs[0][:2500], pairs[1][:2500]
    pr = pr[:1500] + [("a" * 64 + "x", "a" * 64 + "y")] + pr[1500:]  # (a host pair inside the second chunk)
    counts = counts[:1500] + [7] + counts[1500:]
    whole = mine(model, pr, counts, 2, True)
    assert whole == MT.twin_result(pr, counts, 2, True)
    A.VariantModel.mine_chunk(1000)
    try:
        assert mine(model, pr, counts, 2, True) == whole
        assert mine(model, pr, counts, 2, True, sites=False) == whole[0]
    finally:
        A.VariantModel.mine_chunk(0)
    assert mine(model, pr, counts, 2, True, sites=False) == whole[0]


@pytest.mark.parametrize("context,anchors", [(0, False), (1, False), (0, True)])
def test_mined_patterns_weigh_their_pairs(model, pairs, data_dir, context, anchors):
    pr = pairs[0]
    table, _off, sites = mine(model, pr, None, context, anchors)
    top = [k for k, (_t, _c, _s, f) in enumerate(table) if not f][:20]
    members = {k: set() for k in top}
    for p, _ap, _al, _bp, _bl, pat, _fl in sites:
        if pat in members:
            members[pat].add(p)
    for k in top:
        m = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=-1)
        m.add_to_confusables(table[k][0], 0.5)
        twin = Confusable(table[k][0], 0.5)
        for p in sorted(members[k]):
            a, b = pr[p]
            w = m.confusable_weight_text(a, b)
            if context == 0 and not anchors:
                assert w == 0.5, (table[k][0], a, b)
            else:  # the reference's greedy found_in misses a few sites of such patterns: whatever it says
                assert w == (0.5 if twin.found_in(MT.script(a, b)) else 1.0), (table[k][0], a, b)
