"""anx_score_pairs_weighted on the device (conf.hip k_pairs_conf_screen + k_pairs_conf_script behind the pair kernels of pairs.hip):
every weight `==` oracle/confusable_oracle.py (compute_confusable_weight, src/lib.rs:1733-1756), every record byte-equal to
anx_score_pairs', score * weight `==` the dist_score of the rows find_variants ranks on the same model (late and early mode), the
host path (beyond 64 code points a side, ANX_CONFUSABLES=host) and what the counters say about it, a plain model, the chunk boundary
and concurrent first calls.  Model: nld.aspell + confusables10.tsv + four added patterns (pairs_conf_common.py)."""
import ctypes as C
import os
import random
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import synth
import pairs_conf_common as PC

CF_MAXCP = 64  # code points a side the device's lane memory holds (conf.hip)
REC = np.dtype([("score", "<f8"), ("ld", "<u2"), ("lcs", "<u2"), ("prefixlen", "<u2"), ("suffixlen", "<u2"),
                ("len_a", "u1"), ("len_b", "u1"), ("samecase", "u1"), ("status", "i1"), ("_pad", "<u4")])


def nld_model(data_dir, early=False):
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g.read_lexicon(os.path.join(data_dir, "nld.aspell.lexicon"))
    PC.load_patterns(g)
    if early:
        g.set_confusables_before_pruning()
    g.build()
    return g


@pytest.fixture(scope="module")
def nld(data_dir):
    return nld_model(data_dir)


@pytest.fixture(scope="module")
def words(data_dir):
    return synth.load_lexicon_words(os.path.join(data_dir, "nld.aspell.lexicon"))


@pytest.fixture(scope="module")
def pats():
    return PC.oracle_patterns()


@pytest.fixture(scope="module")
def lex_pairs(words, pats):
    """test 2's pairs and the oracle's weights, computed once"""
    pairs = PC.lexicon_pairs(words, 20000)
    return pairs, PC.oracle_weights(pats, pairs)


def stats():
    s = A.VariantModel.pairs_conf_stats()
    return s["pairs"], s["screened"], s["device_scripts"], s["host_pairs"]


def packed_call(g, a, b, weighted=True):
    """a, b: lists of bytes -> (records, weights | None) through the packed calls"""
    n = len(a)
    ba, bb = b"".join(x + b"\0" for x in a), b"".join(x + b"\0" for x in b)
    return blob_call(g, ba, bb, n, weighted)


def blob_call(g, ba, bb, n, weighted=True):
    assert REC.itemsize == C.sizeof(L.PairScore) == 24
    out = np.zeros(max(n, 1), dtype=REC)
    optr = out.ctypes.data_as(C.POINTER(L.PairScore))
    if not weighted:
        L.check(L.lib().anx_score_pairs_packed(g.h, ba, len(ba), bb, len(bb), n, optr))
        return out[:n], None
    w = np.full(max(n, 1), -7.0)
    L.check(L.lib().anx_score_pairs_weighted_packed(g.h, ba, len(ba), bb, len(bb), n, optr, w.ctypes.data_as(C.POINTER(C.c_double))))
    return out[:n], w[:n]


def check_pairs(g, pats, pairs, exp=None):
    """weights == the oracle's, records byte-equal to the unweighted call's (packed and pointer form)"""
    a, b = [x.encode() for x, _ in pairs], [y.encode() for _, y in pairs]
    rec, w = packed_call(g, a, b)
    plain, _ = packed_call(g, a, b, weighted=False)
    assert rec.tobytes() == plain.tobytes()
    exp = PC.oracle_weights(pats, pairs) if exp is None else exp
    bad = [(pairs[i][0][:40], pairs[i][1][:40], w[i], exp[i]) for i in range(len(pairs)) if not w[i] == exp[i]]
    assert not bad, (len(bad), bad[:5])
    return rec, w


def test_hand_made_set_and_shapes(nld, pats):
    rng = random.Random(3)
    pairs = [(a, b) for a, b, _ in PC.HAND] + [(b, a) for a, b, _ in PC.HAND]
    nhand = len(pairs)
    # the capacities of the lane memory: 1 / 1, 63 / 64, 64 / 64, 64 / 65 and 65 / 1 code points, every pair one the screen must list
    fill = lambda n: "".join(rng.choice("abdr") for _ in range(n))  # noqa: E731
    t = fill(70)
    caps = [("y", "i"), ("y" + t[:62], "i" + t[:63]), (t[:30] + "y" + t[30:63], t[:30] + "i" + t[30:63]),
            ("y" + t[:63], "i" + t[:64]), ("y" * 65, "i")]
    assert [(len(a), len(b)) for a, b in caps] == [(1, 1), (63, 64), (64, 64), (64, 65), (65, 1)]
    pairs += caps
    # 2-, 3- and 4-byte characters around an edit (nine characters in 18 bytes are in the hand-made set)
    pairs += [("héys", "héis"), ("hu€ys", "hu€is"), ("𝔘huys", "𝔘huis"), ("cyrk€l", "cirk€l"), ("vrÿheid", "vrijheid"), ("ſien", "zien")]
    pairs += [("ab" * 32, "ba" * 32), ("yi" * 32, "iy" * 32), ("sz" * 32, "zs" * 32)]
    # long scripts: 200 random 64-letter strings over ab (up to 36 diffs; intermediate lists may go beyond the device's 48), and the same
    # strings over letters the patterns speak of, so that the screen cannot settle them
    S = ["".join(rng.choice("ab") for _ in range(64)) for _ in range(200)]
    pairs += [(S[i], S[i + 1]) for i in range(0, 200, 2)]
    pairs += [(S[i].replace("b", "y"), S[i + 1].replace("b", "i")) for i in range(0, 200, 2)]
    pairs += [(S[i].replace("b", "s").replace("a", "e"), S[i + 1].replace("b", "z").replace("a", "e")) for i in range(0, 200, 2)]
    s0 = stats()
    rec, w = check_pairs(nld, pats, pairs)
    s1 = stats()
    for (a, b, e), x in zip(PC.HAND, w[:len(PC.HAND)]):
        assert x == e, (a, b)
    assert (rec["status"] == 0).all()
    assert w[nhand] == 1.1 and w[nhand + 3] == 1.1 and w[nhand + 4] == 1.1
    over = sum(1 for a, b in pairs if len(a) > CF_MAXCP or len(b) > CF_MAXCP)
    assert over == 2
    seen, screened, scripts, host = (s1[k] - s0[k] for k in range(4))
    assert seen == len(pairs) and screened + scripts + host == len(pairs)
    assert host >= over                       # above 64 code points a pair takes the host (so may one whose script outgrows the lane memory)
    # the y/i and s/z strings and the five capacity pairs cannot be settled by the screen (whether a 64-letter script fits the lane
    # memory is not asserted); the hand-made pairs with a weight are short and were weighted by a device script
    assert scripts + host >= 200 + len(caps) and scripts >= sum(1 for _, _, e in PC.HAND if e != 1.0)


def test_invalid_utf8_equals_the_host_function(nld):
    a = [b"hu\xffys", b"\xc3", b"ab\xe2\x82y", b"\xc3(y", b"y\x80", b"\xf0\x9d\x94y", b"cy\xc3", b"\x80\x80y", b"\xf8yrkel", b"y\xe2\x82"]
    b = [b"hu\xffis", b"\xc3\xa9", b"ab\xe2\x82\xaci", b"\xc3(i", b"i\x80", b"\xf0\x9d\x94\x98i", b"ci\xc3", b"\x80i", b"\xf8irkel", b"i\xe2"]
    # bytes the decoder reads differently from what they look like: a lead byte that swallows an ASCII byte on one side only (the host
    # script of the first pair is =[U+00E5]+[e]: `+[e]$`), overlong forms that decode to ASCII (0xC1 0xB9 is 'y': `-[y]+[i]`)
    a += [b"\xc3e", b"\xc1\xb9", b"hu\xc1\xb9s", b"\xe0\x81\xb9", b"he\xc3bb", b"\xc3\xa5e", b"i"]
    b += [b"\xc3\xa5e", b"i", b"huis", b"i", b"he\xc3\xa2bbe", b"\xc3e", b"\xc1\xb9"]
    rec, w = packed_call(nld, a, b)
    plain, _ = packed_call(nld, a, b, weighted=False)
    assert rec.tobytes() == plain.tobytes()
    assert w[10] == 0.95 and w[11] == 1.1 and w[12] == 1.1
    hits = 0
    for x, y, got in zip(a, b, w):
        d = C.c_double()
        L.check(L.lib().anx_model_confusable_weight_text(nld.h, x, y, C.byref(d)))
        assert got == d.value, (x, y, got, d.value)
        hits += d.value != 1.0
    assert hits >= 4


def test_random_pairs(nld, pats, lex_pairs):
    pairs, exp = lex_pairs
    assert len(pairs) == 20000
    assert sum(1 for x in exp if x != 1.0) >= 0.02 * len(pairs)  # the comparison cannot pass on a screen that lets nothing through
    s0 = stats()
    check_pairs(nld, pats, pairs, exp)
    s1 = stats()
    assert s1[0] - s0[0] == 20000 and s1[2] - s0[2] >= 0.02 * 20000 and s1[1] - s0[1] > 0


@pytest.mark.parametrize("early", [False, True])
def test_ranked_rows(nld, data_dir, words, early):
    g = nld_model(data_dir, early=True) if early else nld
    qs = synth.make_queries(words, 500, seed=41)
    rows = g.find_variants_ids(qs, A.SearchParameters())
    flat = [(qs[i], g.vocab_text(v), d) for i, r in enumerate(rows) for v, d, _ in r]
    assert len(flat) > 1000
    got = g.score_pairs([q for q, _, _ in flat], [t for _, t, _ in flat], weighted=True)
    for (q, t, d), r in zip(flat, got):
        assert r["status"] == 0 and r["score"] * r["weight"] == d and r["weighted_score"] == d, (q, t, r, d)
    assert sum(1 for r in got if r["weight"] != 1.0) >= 1


def test_statuses(nld):
    pairs = [("", "huis"), ("huys", ""), ("", ""), ("y" * 256, "i"), ("y", "i" * 300), ("", "i" * 256), ("huys", "huis")]
    got = nld.score_pairs([a for a, _ in pairs], [b for _, b in pairs], weighted=True)
    for (a, b), r in zip(pairs[:-1], got):
        assert r["status"] == (L.ANX_EEMPTY if not a or not b else L.ANX_ELIMIT), (a[:8], b[:8], r)
        assert r["weight"] == 1.0 and r["score"] == 0.0 and r["weighted_score"] == 0.0, (a[:8], b[:8], r)
    assert got[-1]["status"] == 0 and got[-1]["weight"] == 1.1
    a, b = [x.encode() for x, _ in pairs], [y.encode() for _, y in pairs]
    assert packed_call(nld, a, b)[0].tobytes() == packed_call(nld, a, b, weighted=False)[0].tobytes()


def test_plain_model(data_dir, lex_pairs):
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    g.build()
    pairs = lex_pairs[0][:3000] + [("", "x"), ("huys", "huis"), ("y" * 70, "i" * 70)]
    a, b = [x.encode() for x, _ in pairs], [y.encode() for _, y in pairs]
    s0 = stats()
    rec, w = packed_call(g, a, b)
    s1 = stats()
    assert (w == 1.0).all()
    assert rec.tobytes() == packed_call(g, a, b, weighted=False)[0].tobytes()
    assert s1[0] - s0[0] == len(pairs) and s1[2] == s0[2] and s1[3] == s0[3]
    cols = g.score_pairs_arrays([x for x, _ in pairs], [y for _, y in pairs], packed=False, weighted=True)
    assert (cols["weight"] == 1.0).all() and cols["weight"].shape == (len(pairs),)


def test_host_switch_equals_the_device(nld, lex_pairs):
    pairs, exp = lex_pairs
    a, b = [x.encode() for x, _ in pairs], [y.encode() for _, y in pairs]
    rec_d, w_d = packed_call(nld, a, b)
    A.set_switch("ANX_CONFUSABLES", "host")
    try:
        s0 = stats()
        rec_h, w_h = packed_call(nld, a, b)
        s1 = stats()
    finally:
        A.set_switch("ANX_CONFUSABLES", None)
    assert s1[2] == s0[2] and s1[3] - s0[3] == len(pairs) and s1[0] - s0[0] == len(pairs)
    assert np.array_equal(w_h, w_d) and np.array_equal(w_h, np.array(exp))
    assert rec_h.tobytes() == rec_d.tobytes()
    s2 = stats()
    packed_call(nld, a[:100], b[:100])
    assert stats()[3] == s2[3]  # restored: the device weights again


def test_chunk_boundary(nld, lex_pairs):
    pairs, exp = lex_pairs
    hot = [i for i, x in enumerate(exp) if x != 1.0][:24]
    pool = [pairs[i] for i in hot] + [p for p in pairs[:200] if len(p[0].encode()) <= 24][:38] + [("", "huis"), ("y" * 65, "i")]
    assert len(pool) == 64
    a, b = [x.encode() for x, _ in pool], [y.encode() for _, y in pool]
    rec64, w64 = packed_call(nld, a, b)
    assert (w64 != 1.0).sum() >= 24
    n = (1 << 20) + 3
    ba, bb = b"".join(x + b"\0" for x in a), b"".join(x + b"\0" for x in b)
    reps = n // 64
    rec, w = blob_call(nld, ba * reps + b"".join(x + b"\0" for x in a[:3]), bb * reps + b"".join(x + b"\0" for x in b[:3]), n)
    ix = np.arange(n) % 64
    assert np.array_equal(w, w64[ix])
    assert rec.tobytes() == rec64[ix].tobytes()


def test_four_threads_first_call(lex_pairs):
    g = A.VariantModel("", alphabet_text="\n".join("abcdefghijklmnopqrstuvwxyz") + "\n", device=0)
    for wd in ("huis", "kat", "zien", "cirkel"):
        g.add_to_vocabulary(wd)
    PC.load_patterns(g)
    g.build()
    pairs = lex_pairs[0]
    got, errors = {}, []

    def work(t):
        try:
            p = pairs[2000 * t:2000 * (t + 1)]
            got[t] = packed_call(g, [x.encode() for x, _ in p], [y.encode() for _, y in p])
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    rec, w = packed_call(g, [x.encode() for x, _ in pairs[:8000]], [y.encode() for _, y in pairs[:8000]])
    assert (w != 1.0).sum() >= 100
    for t in range(4):
        assert np.array_equal(got[t][1], w[2000 * t:2000 * (t + 1)]), t
        assert got[t][0].tobytes() == rec[2000 * t:2000 * (t + 1)].tobytes(), t
