"""`via` through the device-side exports (export_capi.cpp): anx_batch_export_compact_via, anx_batch_gather_compact_via and
anx_batch_export_topk_via against anx_batch_fetch_compact_via / anx_batch_fetch on the same batch.  The via-less exports write 16-byte
records, which lose the `via` of every row of a model with variant lists; the new calls add one uint32 per row and must leave offsets
and records byte-equal to the via-less export."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import shard as SH
from analiticcl_amd import synth

from variant_models_common import assert_compact_equals_fetch, build_pair, hand_made_lists, queries_for

NONE = 0xFFFFFFFF
P = dict(max_anagram_distance=3, max_edit_distance=2, max_matches=10)


@pytest.fixture(scope="module")
def words(data_dir):
    return synth.load_lexicon_words(os.path.join(data_dir, "eng.aspell.lexicon"))


@pytest.fixture(scope="module")
def lists(tmp_path_factory, words):
    return hand_made_lists(tmp_path_factory.mktemp("hand"), words)


@pytest.fixture(scope="module")
def hand(data_dir, lists):
    return build_pair(data_dir, lists, want_oracle=False)[0]


@pytest.fixture(scope="module")
def plain(data_dir):
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    g.build()
    return g


def _device_buffer(nbytes, fill=0xAB):
    import torch
    return torch.full((max(nbytes, 16),), fill, dtype=torch.uint8, device="cuda:0")


def _bytes(buf, used):
    import torch
    torch.cuda.synchronize()
    return buf[:used].cpu().numpy().tobytes()


def _split(raw, n):
    """export_compact(with_via=True) bytes -> (offsets u32[n + 1], records, via u32, the offsets + records bytes)"""
    off = np.frombuffer(raw, dtype="<u4", count=n + 1)
    total = int(off[n])
    ob = SH.compact_offsets_bytes(n)
    rec = np.frombuffer(raw, dtype=SH.TOPK_DTYPE, count=total, offset=ob)
    via = np.frombuffer(raw, dtype="<u4", count=total, offset=ob + 16 * total)
    assert len(raw) == ob + 20 * total
    return off, rec, via, raw[:ob + 16 * total]


def _run(model, qs, p):
    b = model.encode_batch(qs, p)
    b.run()
    return b


def _check_compact_export(b, n):
    """-> (offsets, records, via) of export_compact(with_via=True), checked against fetch_compact(with_via=True), the fetch and the via-less export"""
    foff, frec, fvia = b.fetch_compact(with_via=True)
    buf = _device_buffer(SH.compact_capacity(n, max(1, int(np.diff(foff.astype(np.int64)).max(initial=0))), with_via=True) + 64)
    used = b.export_compact(buf.data_ptr(), buf.numel(), with_via=True)
    raw = _bytes(buf, used)
    off, rec, via, head = _split(raw, n)
    assert np.array_equal(off, foff) and rec.tobytes() == frec.tobytes() and np.array_equal(via, fvia)
    plain_buf = _device_buffer(len(head) + 64)
    plain_used = b.export_compact(plain_buf.data_ptr(), plain_buf.numel())
    assert plain_used == len(head) and _bytes(plain_buf, plain_used) == head
    # the bytes behind `used` were not touched
    import torch
    torch.cuda.synchronize()
    assert bool((buf[used:] == 0xAB).all())
    # shard.py's decoder on the same bytes
    dec = SH.decode_compact(raw, n, with_via=True)
    assert [len(x) for x in dec] == list(np.diff(off.astype(np.int64)))
    flat = [r for x in dec for r in x]
    assert [r[0] for r in flat] == [int(v) for v in rec["vocab_id"]] and [r[3] for r in flat] == [None if v == NONE else int(v) for v in via]
    return off, rec, via


def test_export_compact_via_on_a_variant_list_model(hand, words, lists):
    qs = queries_for(words, lists, 300, seed=2100)
    b = _run(hand, qs, A.SearchParameters(**P))
    off, rec, via = _check_compact_export(b, len(qs))
    assert assert_compact_equals_fetch(b, off, rec, via) >= 1, "no row with a via"
    assert int((via != NONE).sum()) >= 1
    b.free()


def test_export_compact_via_on_a_plain_model(plain, words):
    qs = synth.make_queries(words, 300, max_len=16, seed=2200)
    b = _run(plain, qs, A.SearchParameters(**P))
    off, rec, via = _check_compact_export(b, len(qs))
    assert via.size == int(off[-1]) > 300 and bool((via == NONE).all())
    poff, prec = b.fetch_compact()
    assert np.array_equal(off, poff) and rec.tobytes() == prec.tobytes()
    b.free()


def test_gather_compact_via_over_three_replicas(data_dir, words, lists):
    A.set_switch("ANX_SHARD_MIN", 64)
    try:
        g = build_pair(data_dir, lists, devices=[0, 0, 0], want_oracle=False)[0]
        qs = queries_for(words, lists, 600, seed=2300)
        b = _run(g, qs, A.SearchParameters(**P))
        shards = b.shards()
        assert len(shards) == 3
        foff, frec, fvia = b.fetch_compact(with_via=True)
        assert int((fvia != NONE).sum()) >= 1
        buf, other = _device_buffer(4 << 20), _device_buffer(4 << 20)
        with pytest.raises(A.AnxError, match="several replicas"):
            b.export_compact(buf.data_ptr(), buf.numel(), with_via=True)
        with pytest.raises(A.AnxError, match="too small") as e:
            b.gather_compact(0, buf.data_ptr(), 1024, with_via=True)
        assert e.value.code == L.ANX_ELIMIT
        so, used = b.gather_compact(0, buf.data_ptr(), buf.numel(), with_via=True)
        _pso, pused = b.gather_compact(0, other.data_ptr(), other.numel())
        raw = _bytes(buf, used)
        assert so[-1] == used and len(so) == 4 and all(int(x) % 256 == 0 for x in so) and used > pused
        seen = np.zeros(len(qs), dtype=bool)
        n_via = 0
        for s, (_dev, lo, cnt) in enumerate(shards):
            ix = b.shard_inputs(s)
            ix = np.arange(lo, lo + cnt) if ix is None else ix
            o = np.frombuffer(raw, dtype="<u4", count=cnt + 1, offset=int(so[s]))
            total = int(o[cnt])
            base = int(so[s]) + SH.compact_offsets_bytes(cnt)
            assert base + 20 * total <= int(so[s + 1])
            r = np.frombuffer(raw, dtype=SH.TOPK_DTYPE, count=total, offset=base)
            v = np.frombuffer(raw, dtype="<u4", count=total, offset=base + 16 * total)
            assert np.array_equal(np.diff(o).astype(np.int64), foff[ix + 1].astype(np.int64) - foff[ix].astype(np.int64))
            rows = np.concatenate([np.arange(foff[i], foff[i + 1], dtype=np.int64) for i in ix]) if len(ix) else np.zeros(0, dtype=np.int64)
            assert r.tobytes() == frec[rows].tobytes() and np.array_equal(v, fvia[rows])
            dec = SH.decode_compact(raw[int(so[s]):int(so[s + 1])], cnt, with_via=True)
            assert [x[3] for d in dec for x in d] == [None if w == NONE else int(w) for w in v]
            n_via += int((v != NONE).sum())
            seen[ix] = True
        assert seen.all() and n_via == int((fvia != NONE).sum())
        b.free()
    finally:
        A.set_switch("ANX_SHARD_MIN", None)


def test_export_topk_via(hand):
    import torch
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=0, score_threshold=0.0, cutoff_threshold=0.0)
    qs = ["recieve", "qwertyx", "", "seperate", "thier", "zzzzzzzzzzzzzzzz"]
    b = _run(hand, qs, p)
    off, rec, via = b.fetch_compact(with_via=True)
    counts = np.diff(off.astype(np.int64))
    stride = int(counts.max())
    assert counts[1] >= 150 and stride >= 150    # `qwertyx` has 150 references
    n = len(qs)
    out = torch.full((n * stride * 16,), 0xFF, dtype=torch.uint8, device="cuda:0")
    vout = torch.zeros(n * stride, dtype=torch.int32, device="cuda:0")   # zeroed: every word must be WRITTEN, padding included
    b.export_topk(out.data_ptr(), stride, via_ptr=vout.data_ptr())
    torch.cuda.synchronize()
    got = np.frombuffer(out.cpu().numpy().tobytes(), dtype=SH.TOPK_DTYPE).reshape(n, stride)
    gvia = np.frombuffer(vout.cpu().numpy().tobytes(), dtype="<u4").reshape(n, stride)
    for i in range(n):
        c = int(counts[i])
        assert got[i, :c].tobytes() == rec[off[i]:off[i + 1]].tobytes(), qs[i]
        assert np.array_equal(gvia[i, :c], via[off[i]:off[i + 1]]), qs[i]
        assert bool((got[i, c:]["vocab_id"] == NONE).all()) and bool((gvia[i, c:] == NONE).all()), qs[i]
    assert int((gvia != NONE).sum()) == int((via != NONE).sum()) >= 150
    # the records equal the via-less export's
    out2 = torch.full((n * stride * 16,), 0xFF, dtype=torch.uint8, device="cuda:0")
    b.export_topk(out2.data_ptr(), stride)
    torch.cuda.synchronize()
    assert bool((out == out2).all())
    dec = SH.decode_topk(out, n, stride, via=vout)
    assert [len(x) for x in dec] == list(counts) and [x[3] for x in dec[0]] == [None if w == NONE else int(w) for w in via[off[0]:off[1]]]
    with pytest.raises(A.AnxError, match="smaller than the longest result list") as e:
        b.export_topk(out.data_ptr(), stride - 1, via_ptr=vout.data_ptr())
    assert e.value.code == L.ANX_ELIMIT
    b.free()


@pytest.mark.parametrize("qs", [[""], ["", "", ""], ["recieve"], ["zzzzzzzzzzzzzzzz", ""]])
def test_edge_batches(hand, qs):
    b = _run(hand, qs, A.SearchParameters(**P))
    off, rec, via = _check_compact_export(b, len(qs))
    if qs == ["recieve"]:
        assert int(off[-1]) >= 1 and int((via != NONE).sum()) >= 1
    if not any(qs):
        assert int(off[-1]) == 0 and via.size == 0
    b.free()


def test_capacity_and_not_run(hand, words, lists):
    import ctypes as C
    qs = queries_for(words, lists, 50, seed=2400)
    p = A.SearchParameters(**P)
    b = hand.encode_batch(qs, p)
    buf = _device_buffer(1 << 20)
    for call in (lambda: b.export_compact(buf.data_ptr(), buf.numel(), with_via=True),
                 lambda: b.gather_compact(0, buf.data_ptr(), buf.numel(), with_via=True),
                 lambda: b.export_topk(buf.data_ptr(), 64, via_ptr=buf.data_ptr() + (1 << 19))):
        with pytest.raises(A.AnxError, match="has not been run") as e:
            call()
        assert e.value.code == L.ANX_EINVAL
    b.run()
    # one byte short: ANX_ELIMIT and `used` = the size that then succeeds
    used = C.c_size_t(0)
    rc = L.lib().anx_batch_export_compact_via(b.h, C.c_void_p(buf.data_ptr()), 0, None, C.byref(used))
    need = used.value
    assert rc == L.ANX_ELIMIT and need > SH.compact_offsets_bytes(len(qs))
    used = C.c_size_t(0)
    assert L.lib().anx_batch_export_compact_via(b.h, C.c_void_p(buf.data_ptr()), need - 1, None, C.byref(used)) == L.ANX_ELIMIT
    assert used.value == need
    assert b.export_compact(buf.data_ptr(), need, with_via=True) == need
    gused = C.c_size_t(0)
    assert L.lib().anx_batch_gather_compact_via(b.h, 0, C.c_void_p(buf.data_ptr()), need - 1, None, C.byref(gused)) == L.ANX_ELIMIT
    assert gused.value == (need + 255) // 256 * 256
    so, u = b.gather_compact(0, buf.data_ptr(), gused.value, with_via=True)
    assert u == gused.value and list(so) == [0, u]
    foff, frec, fvia = b.fetch_compact(with_via=True)
    off, rec, via, _head = _split(_bytes(buf, need), len(qs))
    assert np.array_equal(off, foff) and rec.tobytes() == frec.tobytes() and np.array_equal(via, fvia)
    b.free()
