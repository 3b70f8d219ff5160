"""The searched symbol groups of the signature (host_model.cpp, search_sig_groups) change which records the scan meets and nothing
else: rows, scores and the scored pairs per query of a model built with the search equal those of the greedy groups
(ANX_SIG_SEARCH=0) exactly, and the C oracle's; on a slice of the golden lexicon and on lexicons where the search has little or
nothing to move."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import synth
from oracle import cwrap as O

LATIN = [chr(c) for c in range(ord("a"), ord("z") + 1)]
WIDE = [chr(c) for c in range(0x3B1, 0x3B1 + 25)] + [chr(c) for c in range(0x430, 0x430 + 15)]  # 40 classes: the count-vector scan


def tsv(letters):
    return "\n".join(letters) + "\n"


def models(alphabet_text, words):
    out = {}
    for search in (0, 1):
        A.set_switch("ANX_SIG_SEARCH", search)
        try:
            g = A.VariantModel("", alphabet_text=alphabet_text, device=0)
            for w in words:
                g.add_to_vocabulary(w)
            g.build()
        finally:
            A.set_switch("ANX_SIG_SEARCH", None)
        out[search] = g
    o = O.OracleModel(alphabet_text=alphabet_text)
    for w in words:
        o.add(w)
    o.build()
    return out, o


def groups_of(g, letters):
    out = []
    s = C.c_uint64()
    for ch in letters:
        L.check(L.lib().anx_debug_signature(g.h, ch.encode("utf-8"), C.byref(s)))
        out.append([i for i in range(8) if (s.value >> (8 * i)) & 0xFF][0])
    return out


def check(gs, o, queries, n_oracle):
    """Rows and per-query pair counts of the two models are equal; the first n_oracle queries also equal the oracle's."""
    gp = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
    op = O.make_params(("abs", 3), ("abs", 2), 10, 0.25, 2.0)
    got = {}
    for search, g in gs.items():
        b = g.encode_batch(queries, gp)
        b.run()
        got[search] = (b.fetch_arrays(), b.pair_counts().copy(), b.fetch()[:n_oracle], b.stats())
        b.free()
    for x, y in zip(got[0][0], got[1][0]):
        assert np.array_equal(x, y)
    assert np.array_equal(got[0][1], got[1][1])
    for i, q in enumerate(queries[:n_oracle]):
        if q == "":
            continue
        exp, _pairs, npairs, _ncls = o.find_variants(q, op, want_pairs=True, cap=1 << 17)
        assert [(v, d, f) for v, d, f in got[1][2][i]] == exp, q
        assert int(got[1][1][i]) == npairs, q
    return got[0][3], got[1][3]


def test_golden_slice_rows_equal_greedy_and_oracle():
    words = synth.load_lexicon_words(synth.GOLDEN_DATA + "/eng_aspell.lexicon.gz")[::24]
    assert 4500 < len(words) < 5500
    with open(synth.GOLDEN_DATA + "/simple_alphabet.tsv", encoding="utf-8") as f:
        alphabet = f.read()
    gs, o = models(alphabet, words)
    assert groups_of(gs[0], LATIN) != groups_of(gs[1], LATIN)  # the search moved slots: the two models scan different records
    queries = synth.make_queries(words, 4096, max_len=16, seed=41)
    st0, st1 = check(gs, o, queries, 256)
    assert st0["n_pairs"] == st1["n_pairs"] > 0 and st0["n_results"] == st1["n_results"]
    print(f"class tests: greedy {st0['n_class_tests']}, searched {st1['n_class_tests']}")


def test_fewer_symbols_than_groups():
    rng = random.Random(5)
    words = sorted({"".join(rng.choice("abc") for _ in range(rng.randrange(1, 9))) for _ in range(400)})
    gs, o = models(tsv(LATIN), words)
    queries = synth.make_queries(words, 300, max_len=12, seed=3) + ["", "abcz", "zzz", "c" * 11]
    check(gs, o, queries, len(queries))


def test_one_symbol_lexicon():
    words = ["a" * n for n in range(1, 13)]
    gs, o = models(tsv(LATIN), words)
    queries = ["a", "aaa", "aab", "b", "a" * 13, "a" * 20, "baaab", "", "aaaaaa"]
    check(gs, o, queries, len(queries))


def test_small_lexicon_on_a_wide_alphabet():
    rng = random.Random(40)
    words = sorted({"".join(rng.choice(WIDE[:14] if rng.random() < 0.5 else WIDE) for _ in range(rng.randrange(2, 12))) for _ in range(210)})[:200]
    assert len(words) == 200
    gs, o = models(tsv(WIDE), words)
    queries = []
    for _ in range(300):
        cs = list(rng.choice(words))
        for _ in range(rng.randrange(0, 3)):
            op = rng.randrange(3)
            if op == 0 and len(cs) > 1:
                del cs[rng.randrange(len(cs))]
            elif op == 1:
                cs.insert(rng.randrange(len(cs) + 1), rng.choice(WIDE))
            else:
                cs[rng.randrange(len(cs))] = rng.choice(WIDE)
        queries.append("".join(cs))
    st0, st1 = check(gs, o, queries, len(queries))
    for st in (st0, st1):
        assert st["n_tests_kind"][0] > 0 and sum(st["n_tests_kind"][1:]) == 0  # every tile took the count-vector kernel
