"""analiticcl_amd/shard.py on the exports with `via` (anx_batch_export_compact_via / anx_batch_gather_compact_via / anx_batch_export_topk_via):
decode_compact(with_via=True), compact_capacity(with_via=True) and decode_topk(via=...) on hand-built buffers, zero rows included; the
via-less forms return on the same buffers what they returned before the `via` words existed."""
import numpy as np

from analiticcl_amd import shard as SH

NONE = 0xFFFFFFFF


def _compact(lists, with_via):
    """[[(vocab_id, dist, freq, via or None)]] per input -> the bytes of the compact export"""
    n = len(lists)
    off = np.zeros(n + 1, dtype="<u4")
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = [r for x in lists for r in x]
    rec = np.zeros(len(flat), dtype=SH.TOPK_DTYPE)
    for k, (v, d, f, _via) in enumerate(flat):
        rec[k] = (v, f, d)
    head = off.tobytes()
    head += bytes(SH.compact_offsets_bytes(n) - len(head))
    out = head + rec.tobytes()
    if with_via:
        out += np.array([NONE if r[3] is None else r[3] for r in flat], dtype="<u4").tobytes()
    return out


LISTS = [[(7, 1.0, 0.5, None), (9, 0.75, 0.25, 7)], [], [(3, 0.5, 1.0, 11), (4, 0.5, 0.0, None), (5, 0.25, 0.0, 0)], [(1, 0.125, 0.0, None)]]


def test_offsets_are_padded_to_16_bytes():
    assert [SH.compact_offsets_bytes(n) for n in (0, 1, 3, 4, 7, 8)] == [16, 16, 16, 32, 32, 48]


def test_decode_compact_with_via():
    buf = _compact(LISTS, True)
    assert len(buf) == 32 + 6 * 16 + 6 * 4
    assert SH.decode_compact(buf, 4, with_via=True) == [list(x) for x in LISTS]
    # a via of 0 is a vocabulary id, not "none"
    assert SH.decode_compact(buf, 4, with_via=True)[2][2][3] == 0
    # the via-less view of the same bytes: the records alone, as 3-tuples, and equal to the decoding of the via-less export
    plain = [[r[:3] for r in x] for x in LISTS]
    assert SH.decode_compact(buf, 4) == plain
    assert SH.decode_compact(_compact(LISTS, False), 4) == plain
    assert SH.decode_compact(buf, 4, with_via=False) == plain


def test_decode_compact_zero_rows_and_one_input():
    for n in (1, 3, 4):
        empty = [[] for _ in range(n)]
        for with_via in (False, True):
            buf = _compact(empty, with_via)
            assert len(buf) == SH.compact_offsets_bytes(n)
            assert SH.decode_compact(buf, n, with_via=with_via) == empty
    one = [[(42, 1.0, 0.0, 41)]]
    assert SH.decode_compact(_compact(one, True), 1, with_via=True) == one
    assert SH.decode_compact(_compact(one, True), 1) == [[(42, 1.0, 0.0)]]
    # a section inside a larger buffer (the gather pads sections to 256 bytes): the bytes behind it are not read
    padded = _compact(LISTS, True) + b"\xAB" * 100
    assert SH.decode_compact(padded, 4, with_via=True) == [list(x) for x in LISTS]


def test_compact_capacity():
    assert SH.compact_capacity(4, 3) == 32 + 4 * 3 * 16
    assert SH.compact_capacity(4, 3, with_via=False) == SH.compact_capacity(4, 3)
    assert SH.compact_capacity(4, 3, with_via=True) == 32 + 4 * 3 * 20
    assert SH.compact_capacity(0, 5, with_via=True) == 16
    assert SH.compact_capacity(4, 3, with_via=True) >= len(_compact(LISTS, True))


def _topk(lists, stride):
    n = len(lists)
    rec = np.zeros((n, stride), dtype=SH.TOPK_DTYPE)
    rec["vocab_id"] = NONE
    via = np.full((n, stride), NONE, dtype="<u4")
    for i, x in enumerate(lists):
        for k, (v, d, f, w) in enumerate(x):
            rec[i, k] = (v, f, d)
            via[i, k] = NONE if w is None else w
    return rec.tobytes(), via.tobytes()


def test_decode_topk_with_via():
    rec, via = _topk(LISTS, 3)
    assert SH.decode_topk(rec, 4, 3, via=via) == [list(x) for x in LISTS]
    assert SH.decode_topk(rec, 4, 3) == [[r[:3] for r in x] for x in LISTS]
    rec5, via5 = _topk(LISTS, 5)   # a wider stride: more padding, the same lists
    assert SH.decode_topk(rec5, 4, 5, via=via5) == [list(x) for x in LISTS]
    empty = [[], []]
    rec0, via0 = _topk(empty, 2)
    assert SH.decode_topk(rec0, 2, 2, via=via0) == empty and SH.decode_topk(rec0, 2, 2) == empty
