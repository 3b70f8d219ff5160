"""The small call on models with variant lists (small_path.hpp: k_compact_expand in k_compact_grouped's place, k_rank<false>): the
call is answered by the small path, and its rows -- ids, `via`, order, both scores bit for bit -- are those of the batch pipeline
(ANX_SMALL=0) and of the C oracle with the same lists loaded."""
import os
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import synth
from oracle import cwrap as O

from variant_models_common import (HAND_QUERIES, assert_has_variant_lists, build_pair, hand_made_lists, learn_inputs, learned_list,
                                   listed_variants, queries_for, small_stats, via_batch_path)


@pytest.fixture(scope="module")
def words(data_dir):
    return synth.load_lexicon_words(os.path.join(data_dir, "eng.aspell.lexicon"))


@pytest.fixture(scope="module")
def hand(data_dir, tmp_path_factory, words):
    lists = hand_made_lists(tmp_path_factory.mktemp("hand"), words)
    return build_pair(data_dir, lists) + (lists,)


@pytest.fixture(scope="module")
def learned(data_dir, tmp_path_factory, words):
    lists = learned_list(data_dir, tmp_path_factory.mktemp("learned"), words)
    return build_pair(data_dir, lists) + (lists,)


def n_via(rows):
    return sum(1 for r in rows for x in r if x[3] is not None)


@pytest.mark.parametrize("n", [1, 64, 1000, 4096])
@pytest.mark.parametrize("which", ["hand", "learned"])
def test_small_call_takes_variant_list_models(request, words, which, n):
    g, o, lists = request.getfixturevalue(which)
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10, score_threshold=0.25, cutoff_threshold=2.0)
    op = O.make_params(("abs", 3), ("abs", 2), 10, 0.25, 2.0)
    if n == 1:   # one input that has a `via` row on the model: the first listed variant whose reference the oracle returns within max_matches
        qs = ["recieve"] if which == "hand" else next([q] for q in listed_variants(lists) if any(x[3] is not None for x in o.find_variants_via(q, op)))
    else:
        qs = queries_for(words, lists, n, seed=700 + n)
    t0 = small_stats()
    got = g.find_variants_ids(qs, p, with_via=True)
    t1 = small_stats()
    assert t1[0] == t0[0] + 1, "the small path did not take the call"
    assert got == via_batch_path(g, qs, p)
    assert small_stats()[0] == t1[0]       # (the A/B call did not)
    assert n_via(got) >= 1, "no row with a via: the comparison would pass on unexpanded rows"
    idx = [i for i in range(n) if any(x[3] is not None for x in got[i])][:100]
    idx += random.Random(n).sample(range(n), min(n, 200))
    for i in idx:
        assert got[i] == o.find_variants_via(qs[i], op), qs[i]


@pytest.mark.parametrize("fw", [0.0, 0.5])
@pytest.mark.parametrize("mm", [1, 10, 0])
@pytest.mark.parametrize("which", ["hand", "learned"])
def test_freq_weight_and_max_matches(request, words, which, mm, fw):
    g, _o, lists = request.getfixturevalue(which)
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=mm, score_threshold=0.0, cutoff_threshold=0.0, freq_weight=fw)
    qs = queries_for(words, lists, 600, seed=41) + ["", "a", "x" * 64, "héllo"]
    t0 = small_stats()
    got = g.find_variants_ids(qs, p, with_via=True)
    assert sum(small_stats()) == sum(t0) + 1   # taken, or discarded after a capacity overflow and answered by the batch path
    assert got == via_batch_path(g, qs, p)
    assert n_via(got) >= 1


def test_capacity_overflow_falls_back(hand, words):
    """An entry with 150 references in a call of one input (its ranked rows do not fit the caller's block of 16 n + 64 rows), and
    thousands of 3- and 4-letter queries at d = 3 with unlimited matches: either the small path takes the call or the overflow counter
    grows and the batch path answers -- the rows are the same."""
    g, o, _lists = hand
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=3, max_matches=0, score_threshold=0.0, cutoff_threshold=0.0)
    t0 = small_stats()
    got = g.find_variants_ids(["qwertyx"], p, with_via=True)
    t1 = small_stats()
    assert sum(t1) == sum(t0) + 1
    assert t1[1] == t0[1] + 1, "150 expanded rows fitted a block of 80"
    assert got == via_batch_path(g, ["qwertyx"], p)
    assert got[0] == o.find_variants_via("qwertyx", O.make_params(("abs", 3), ("abs", 3), 0, 0.0, 0.0))
    assert n_via(got) >= 150
    short = sorted({w for w in words if 3 <= len(w) <= 4 and w.isalpha()})[:4090] + HAND_QUERIES[:6]
    t0 = small_stats()
    got = g.find_variants_ids(short, p, with_via=True)
    assert sum(small_stats()) == sum(t0) + 1
    assert got == via_batch_path(g, short, p)
    assert sum(len(r) for r in got) > 20 * len(short) and n_via(got) >= 1


def test_two_models_share_the_context_pool(hand, data_dir, words):
    """A model without lists beside the one with lists, calls alternating: the cold arguments of a context (FsCold) follow the model."""
    g, _o, lists = hand
    plain = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    plain.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    plain.build()
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
    sets = [queries_for(words, lists, n, seed=60 + n) for n in (1, 300, 64, 1000)]
    want = {id(m): [via_batch_path(m, qs, p) for qs in sets] for m in (g, plain)}
    assert n_via(want[id(g)][1]) >= 1 and all(n_via(r) == 0 for r in want[id(plain)])
    for _round in range(3):
        for k, qs in enumerate(sets):
            for m in (g, plain, plain, g):
                t0 = small_stats()
                assert m.find_variants_ids(qs, p, with_via=True) == want[id(m)][k]
                assert small_stats()[0] == t0[0] + 1


def test_concurrent_small_calls(hand, words):
    """Eight host threads, each issuing calls of 1 .. 1000 inputs on the one variant-list model (a context per call in flight)."""
    g, _o, lists = hand
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
    sets = [queries_for(words, lists, n, seed=900 + i) for i, n in enumerate((1, 1000, 37, 512, 3, 1000, 250, 64))]
    want = [via_batch_path(g, qs, p) for qs in sets]
    assert n_via(want[1]) >= 1
    errors = []

    def work(i):
        try:
            for _ in range(30):
                if g.find_variants_ids(sets[i], p, with_via=True) != want[i]:
                    errors.append(i)
                    return
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
    t0 = small_stats()
    th = [threading.Thread(target=work, args=(i,)) for i in range(len(sets))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert small_stats()[0] == t0[0] + 30 * len(sets)


def test_small_call_after_learning(data_dir, words):
    """learn_variants(auto_build=True) on a resident model turns it into a model with variant lists: the next call takes the small path."""
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    g.build()
    inputs = learn_inputs(words)
    g.learn_variants(inputs, A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=3), strict=True, auto_build=True)
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
    qs = inputs[:300] + inputs[-300:]
    t0 = small_stats()
    got = g.find_variants_ids(qs, p, with_via=True)
    assert small_stats()[0] == t0[0] + 1
    assert_has_variant_lists(g)
    assert got == via_batch_path(g, qs, p)
    assert n_via(got) >= 1
