"""The small call (small_path.hpp) on multi-device models: anx_find_variants_batch runs a call of at most 4096 short inputs WHOLE on one
replica -- the one with the fewest small calls in flight, ties broken by a rotating start -- instead of handing it to the sharded batch
pipeline.  The GPU boxes have one device, so the replicas are {0, 0} / {0, 0, 0}: they share one context pool, and a context caches the
lexicon-side arguments of the replica it served last (FsCold, small_find's cold_key) -- the one way this can return wrong rows, so the
threads below alternate between replicas AND between two models on the same contexts.  Rows are compared with `==` against the
one-replica model, the batch path (ANX_SMALL=0) and the C oracle."""
import os
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import synth
from oracle import cwrap as O

from variant_models_common import build_pair, hand_made_lists, queries_for, small_stats, via_batch_path

CONF = os.path.join(synth.GOLDEN_DATA, "confusables10.tsv")
P = dict(max_anagram_distance=3, max_edit_distance=2, max_matches=10)


def ids(model, qs, p):
    """anx_find_variants_batch -> [[(vocab_id, dist, freq, via | None)]], the shape via_batch_path returns"""
    return model.find_variants_ids(qs, p, with_via=True)


def _model(data_dir, lex, devices, confusables=False, early=False):
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), devices=devices)
    g.read_lexicon(os.path.join(data_dir, f"{lex}.aspell.lexicon"))
    if confusables:
        g.read_confusablelist(CONF)
        if early:
            g.set_confusables_before_pruning()
    g.build()
    assert g.num_replicas == len(devices)
    return g


@pytest.fixture(scope="module")
def words(data_dir):
    return synth.load_lexicon_words(os.path.join(data_dir, "eng.aspell.lexicon"))


@pytest.fixture(scope="module")
def eng3(data_dir):
    return _model(data_dir, "eng", [0, 0, 0])


@pytest.fixture(scope="module")
def eng1(data_dir):
    return _model(data_dir, "eng", [0])


@pytest.fixture(scope="module")
def oracle(data_dir):
    o = O.OracleModel(alphabet_path=os.path.join(data_dir, "simple.alphabet.tsv"))
    o.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    o.build()
    return o


@pytest.mark.parametrize("n", [1, 7, 1000])
def test_three_replicas_take_the_small_call(eng3, eng1, oracle, words, n):
    p = A.SearchParameters(**P)
    op = O.make_params(("abs", 3), ("abs", 2), 10, 0.25, 2.0)
    qs = synth.make_queries(words, n, max_len=16, seed=1300 + n)
    t0, r0 = small_stats(), eng3.small_replica_stats()
    got = ids(eng3, qs, p)
    t1, r1 = small_stats(), eng3.small_replica_stats()
    assert t1[0] == t0[0] + 1, "the small path did not take the call on the three-replica model"
    assert len(r1) == 3 and sum(r1) == sum(r0) + 1 and all(b >= a for a, b in zip(r0, r1))
    assert got == ids(eng1, qs, p)
    assert got == via_batch_path(eng3, qs, p)
    assert small_stats()[0] == t1[0] + 1       # (the one-replica call was a small call, the A/B call was not)
    for i in random.Random(n).sample(range(n), min(n, 100)):
        assert [x[:3] for x in got[i]] == oracle.find_variants(qs[i], op) and all(x[3] is None for x in got[i]), qs[i]


def test_sequential_calls_walk_the_replicas(eng3, eng1, words):
    p = A.SearchParameters(**P)
    assert eng1.small_replica_stats() == [sum(eng1.small_replica_stats())]   # one replica: one counter
    r0 = eng3.small_replica_stats()
    sets = [synth.make_queries(words, 5, max_len=16, seed=1400 + i) for i in range(30)]
    got = [ids(eng3, qs, p) for qs in sets]
    r1 = eng3.small_replica_stats()
    delta = [b - a for a, b in zip(r0, r1)]
    assert sum(delta) == 30 and all(d >= 1 for d in delta), delta
    for k in (0, 1, 2, 29):   # consecutive calls ran on different replicas: each equals the one-replica model's call
        assert got[k] == ids(eng1, sets[k], p)


def test_concurrent_calls_on_two_models_share_the_contexts(eng3, data_dir, words):
    """Eight threads x 30 calls, every thread alternating between a three-replica eng model and a two-replica nld model, all five replicas
    on device 0: a context serves whichever (model, replica) comes next."""
    nld2 = _model(data_dir, "nld", [0, 0])
    nwords = synth.load_lexicon_words(os.path.join(data_dir, "nld.aspell.lexicon"))
    p = A.SearchParameters(**P)
    sizes = (1, 1000, 37, 512, 3, 1000, 250, 64)
    sets = {id(eng3): [synth.make_queries(words, n, max_len=16, seed=1500 + i) for i, n in enumerate(sizes)],
            id(nld2): [synth.make_queries(nwords, n, max_len=16, seed=1600 + i) for i, n in enumerate(sizes)]}
    want = {id(m): [via_batch_path(m, qs, p) for qs in sets[id(m)]] for m in (eng3, nld2)}
    assert sum(len(r) for r in want[id(eng3)][1]) > 1000 and sum(len(r) for r in want[id(nld2)][1]) > 1000
    t0, r0, n0 = small_stats(), eng3.small_replica_stats(), nld2.small_replica_stats()
    errors = []

    def work(i):
        try:
            for k in range(30):
                m = (eng3, nld2)[(k + i) & 1]
                if ids(m, sets[id(m)][i], p) != want[id(m)][i]:
                    errors.append((i, k, "eng" if m is eng3 else "nld"))
                    return
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
    th = [threading.Thread(target=work, args=(i,)) for i in range(len(sizes))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    t1 = small_stats()
    assert sum(t1) == sum(t0) + 240
    de = [b - a for a, b in zip(r0, eng3.small_replica_stats())]
    dn = [b - a for a, b in zip(n0, nld2.small_replica_stats())]
    assert sum(de) + sum(dn) == t1[0] - t0[0] and all(d >= 1 for d in de + dn), (de, dn)


def test_variant_list_model_on_two_replicas(data_dir, tmp_path, words):
    lists = hand_made_lists(tmp_path, words)
    one, _ = build_pair(data_dir, lists, want_oracle=False)
    two, _ = build_pair(data_dir, lists, devices=[0, 0], want_oracle=False)
    assert two.num_replicas == 2
    p = A.SearchParameters(**P)
    r0 = two.small_replica_stats()
    for k, n in enumerate((1, 300, 64, 300)):
        qs = ["recieve"] if n == 1 else queries_for(words, lists, n, seed=1700 + k)
        t0 = small_stats()
        got = ids(two, qs, p)
        assert small_stats()[0] == t0[0] + 1
        assert got == ids(one, qs, p)
        assert small_stats()[0] == t0[0] + 2
        assert sum(1 for r in got for x in r if x[3] is not None) >= 1, "no row with a via"
    assert all(b > a for a, b in zip(r0, two.small_replica_stats())), "one of the two replicas answered none of four calls"


@pytest.mark.parametrize("early", [False, True])
def test_confusable_model_on_two_replicas(data_dir, early):
    nwords = synth.load_lexicon_words(os.path.join(data_dir, "nld.aspell.lexicon"))
    one = _model(data_dir, "nld", [0], confusables=True, early=early)
    two = _model(data_dir, "nld", [0, 0], confusables=True, early=early)
    p = A.SearchParameters(**P)
    r0 = two.small_replica_stats()
    for k, n in enumerate((1, 400, 50, 400)):
        qs = synth.make_queries(nwords, n, max_len=16, seed=1800 + k)
        t0 = small_stats()
        got = ids(two, qs, p)
        assert small_stats() == (t0[0] + 1, t0[1])
        assert got == ids(one, qs, p)
        assert small_stats() == (t0[0] + 2, t0[1])
    assert all(b > a for a, b in zip(r0, two.small_replica_stats()))


def test_hand_overs_stay_hand_overs_on_three_replicas(eng3, eng1, words):
    """StopAtExactMatch, an input of 65 bytes, 4097 inputs: the batch pipeline answers on a multi-device model too."""
    p = A.SearchParameters(**P)
    t0, r0 = small_stats(), eng3.small_replica_stats()
    ps = A.SearchParameters(stop_criterion=True, **P)
    qs = ["separate", "seperate", "recieve"]
    assert ids(eng3, qs, ps) == via_batch_path(eng3, qs, ps) == via_batch_path(eng1, qs, ps)
    qs = ["recieve", "x" * 65, "seperate"]
    got = ids(eng3, qs, p)
    assert got == via_batch_path(eng3, qs, p) and got[1] == [] and got[0] and got[2]
    qs = synth.make_queries(words, 4097, max_len=16, seed=1900)
    assert ids(eng3, qs, p) == via_batch_path(eng3, qs, p)
    assert small_stats() == t0 and eng3.small_replica_stats() == r0
