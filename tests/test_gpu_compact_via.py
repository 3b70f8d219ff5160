"""Compact records with `via` (anx_batch_fetch_compact_via, anx_compact_to_results_via, anx_pipeline_next_via): the 16-byte records of
anx_batch_fetch_compact plus a parallel uint32 array, for models with variant lists -- against anx_batch_fetch of the same batch."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import synth

from variant_models_common import assert_compact_equals_fetch, build_pair, fetch_columns, hand_made_lists, learned_list, queries_for

PARAMS = (dict(max_anagram_distance=3, max_edit_distance=2, max_matches=10),
          dict(max_anagram_distance=3, max_edit_distance=3, max_matches=0, freq_weight=0.3))


@pytest.fixture(scope="module")
def words(data_dir):
    return synth.load_lexicon_words(os.path.join(data_dir, "eng.aspell.lexicon"))


@pytest.fixture(scope="module")
def hand_lists(tmp_path_factory, words):
    return hand_made_lists(tmp_path_factory.mktemp("hand"), words)


@pytest.fixture(scope="module")
def learned_lists(data_dir, tmp_path_factory, words):
    return learned_list(data_dir, tmp_path_factory.mktemp("learned"), words)


@pytest.fixture(scope="module")
def hand(data_dir, hand_lists):
    return build_pair(data_dir, hand_lists, want_oracle=False)[0]


@pytest.fixture(scope="module")
def learned(data_dir, learned_lists):
    return build_pair(data_dir, learned_lists, want_oracle=False)[0]


def check_batches(g, words, lists, n):
    qs = ["", "recieve"] + queries_for(words, lists, n, seed=91) + ["x" * 300, ""]
    for kw in PARAMS:
        b = g.encode_batch(qs, A.SearchParameters(**kw))
        b.run()
        coff, rec, via = b.fetch_compact(with_via=True)
        assert assert_compact_equals_fetch(b, coff, rec, via) >= 1, "no row with a via"
        with pytest.raises(A.AnxError, match="variant lists"):
            b.fetch_compact()
        b.free()
        del coff, rec, via
    b = g.encode_batch([], A.SearchParameters())
    b.run()
    coff, rec, via = b.fetch_compact(with_via=True)
    assert list(coff) == [0] and rec.size == 0 and via.size == 0
    b.free()


@pytest.mark.parametrize("which", ["hand", "learned"])
def test_fetch_compact_via_equals_fetch(request, words, which):
    g, lists = request.getfixturevalue(which), request.getfixturevalue(which + "_lists")
    check_batches(g, words, lists, 20000)


@pytest.mark.parametrize("policy", ["range", None])
@pytest.mark.parametrize("which", ["hand", "learned"])
def test_three_replicas_both_shard_policies(request, data_dir, words, which, policy):
    """Three replicas on one device: contiguous shards (ANX_SHARD_POLICY=range) and the length-partitioned (scattered) shards."""
    lists = request.getfixturevalue(which + "_lists")
    g = build_pair(data_dir, lists, devices=[0, 0, 0], want_oracle=False)[0]
    assert g.num_replicas == 3
    A.set_switch("ANX_SHARD_MIN", 64)
    A.set_switch("ANX_SHARD_POLICY", policy)
    try:
        qs = queries_for(words, lists, 30000, seed=17)
        b = g.encode_batch(qs, A.SearchParameters(**PARAMS[0]))
        assert len(b.shards()) == 3
        scattered = any(b.shard_inputs(s) is not None for s in range(3))
        assert scattered == (policy is None)
        b.free()
        check_batches(g, words, lists, 30000)
    finally:
        A.set_switch("ANX_SHARD_MIN", None)
        A.set_switch("ANX_SHARD_POLICY", None)


def test_plain_model(data_dir, words, hand_lists):
    """No variant lists: every `via` word is 0xFFFFFFFF, rows and offsets are byte-equal to anx_batch_fetch_compact's."""
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    g.build()
    qs = ["", "seperate"] + queries_for(words, hand_lists, 20000, seed=5) + ["x" * 300, ""]
    for kw in PARAMS:
        b = g.encode_batch(qs, A.SearchParameters(**kw))
        b.run()
        off0, rec0 = b.fetch_compact()
        off1, rec1, via = b.fetch_compact(with_via=True)
        assert rec0.size > 20000 and off0.tobytes() == off1.tobytes() and rec0.tobytes() == rec1.tobytes()
        assert via.shape == (rec0.size,) and bool((via == 0xFFFFFFFF).all())
        b.free()


@pytest.mark.parametrize("which", ["hand", "learned"])
def test_pipeline_on_variant_list_models(request, words, which):
    """Four jobs at depth 3: next(with_via=True) returns, in submission order, what fetch() of the same inputs returns; next() without
    it still answers ANX_EINVAL (it has nowhere to put `via`), and so does fetch_compact()."""
    g, lists = request.getfixturevalue(which), request.getfixturevalue(which + "_lists")
    p = A.SearchParameters(**PARAMS[0])
    sets = [queries_for(words, lists, n, seed=200 + i) for i, n in enumerate((8000, 1, 20000, 500))]
    blobs = [b"".join(q.encode("utf-8") + b"\0" for q in qs) for qs in sets]
    want = []
    for qs, blob in zip(sets, blobs):
        b = g.encode_packed(blob, len(qs), p)
        b.run()
        want.append(fetch_columns(b))
        with pytest.raises(A.AnxError, match="variant lists") as e:
            b.fetch_compact()
        assert e.value.code == L.ANX_EINVAL
        b.free()
    pl = A.Pipeline(g, depth=3)
    try:
        got, nxt = [], 0
        for i in range(len(sets)):
            while nxt < len(sets):
                try:
                    pl.submit(blobs[nxt], len(sets[nxt]), p)
                    nxt += 1
                except A.AnxError as e:
                    assert e.code == L.ANX_ELIMIT
                    break
            got.append(pl.next(with_via=True))
        assert nxt == len(sets) and pl.pending() == 0
        n_with_via = 0
        for (off, vid, dist, freq, fvia), (coff, rec, via) in zip(want, got):
            assert np.array_equal(coff, off) and np.array_equal(rec["vocab_id"], vid) and np.array_equal(rec["dist_score"], dist)
            assert np.array_equal(rec["freq_score"], freq.astype(np.float32))
            assert np.array_equal(np.where(via == 0xFFFFFFFF, np.uint64(0xFFFFFFFFFFFFFFFF), via.astype(np.uint64)), fvia)
            n_with_via += int((via != 0xFFFFFFFF).sum())
        assert n_with_via >= 1
        pl.submit(blobs[3], len(sets[3]), p)
        with pytest.raises(A.AnxError, match="variant lists") as e:
            pl.next()
        assert e.value.code == L.ANX_EINVAL
        assert pl.pending() == 0
    finally:
        pl.close()


def test_pipeline_next_via_on_a_plain_model(data_dir, words, hand_lists):
    """Both calls work on a plain model, in any order (a job fetched before the caller first asked for `via` gets its array on the host)."""
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    g.build()
    p = A.SearchParameters(**PARAMS[0])
    qs = queries_for(words, hand_lists, 5000, seed=9)
    blob = b"".join(q.encode("utf-8") + b"\0" for q in qs)
    b = g.encode_packed(blob, len(qs), p)
    b.run()
    off0, rec0 = b.fetch_compact()
    b.free()
    pl = A.Pipeline(g, depth=3)
    try:
        for _ in range(3):
            pl.submit(blob, len(qs), p)
        off, rec = pl.next()
        assert off.tobytes() == off0.tobytes() and rec.tobytes() == rec0.tobytes()
        pl.submit(blob, len(qs), p)
        for _ in range(3):
            off, rec, via = pl.next(with_via=True)
            assert off.tobytes() == off0.tobytes() and rec.tobytes() == rec0.tobytes() and via.shape == (rec0.size,) and bool((via == 0xFFFFFFFF).all())
        pl.submit(blob, len(qs), p)   # (fetched with room for `via` by now: the plain call takes it all the same)
        off, rec = pl.next()
        assert off.tobytes() == off0.tobytes() and rec.tobytes() == rec0.tobytes()
    finally:
        pl.close()


@pytest.mark.parametrize("which", ["hand", "learned"])
def test_compact_to_results_via(request, words, which):
    """anx_compact_to_results_via reproduces anx_batch_fetch's anx_result rows up to the float32 freq_score."""
    g, lists = request.getfixturevalue(which), request.getfixturevalue(which + "_lists")
    qs = queries_for(words, lists, 20000, seed=33)   # (more than 2^16 rows: the threaded conversion)
    b = g.encode_batch(qs, A.SearchParameters(**PARAMS[1]))
    b.run()
    off, vid, dist, freq, fvia = fetch_columns(b)
    coff, rec, via = b.fetch_compact(with_via=True)
    b.free()
    total = int(coff[-1])
    assert total == int(off[-1]) and total > (1 << 16)
    out = (L.Result * total)()
    L.lib().anx_compact_to_results_via(C.c_void_p(rec.ctypes.data), via.ctypes.data_as(C.POINTER(C.c_uint32)), total, out)
    a = np.frombuffer(out, dtype=np.dtype([("vocab_id", "<u8"), ("dist", "<f8"), ("freq", "<f8"), ("via", "<u8")]))
    assert np.array_equal(a["vocab_id"], vid) and np.array_equal(a["dist"], dist) and np.array_equal(a["via"], fvia)
    assert np.array_equal(a["freq"], freq.astype(np.float32).astype(np.float64))
    assert int((a["via"] != 0xFFFFFFFFFFFFFFFF).sum()) >= 1
