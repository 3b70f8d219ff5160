"""k_rank (kernels_rank.hpp) by itself, through the test hook anx_debug_rank_rows, on the hand-made candidate rows of tests/rank_cases.py
against the tail of the twin's score_and_rank (oracle/twin.py rank_tail: normalise, stable rank, dedup, crop with its tie rule, cutoff).
The reference gets each query's rows in enumeration order, the device the same rows shuffled.  Everything is compared exactly: counts,
vocab ids and via as integers, dist_score and freq_score as f64 with == (which holds -0.0 and +0.0 equal, as the kernel's comparison
does); no tolerance anywhere.  Which branches of the kernel the batches reach is asserted by tests/test_rank_cases_cpu.py."""
import numpy as np
import pytest

import rank_cases as R
from analiticcl_amd import _lib as L

pytestmark = pytest.mark.gpu

DEVROW = np.dtype([("vocab_id", "<u4"), ("via", "<u4"), ("dist_score", "<f8"), ("freq_score", "<f8")])  # kernels_common.hpp DevRow


def rank_raw(b, seg_cap=0, row_cap=None, overflow=0):
    """(r_count[nq], r_rows[total]) as the kernel left them (0xFF bytes where it wrote nothing); the rows go to the device shuffled"""
    P, nq, total = b.params, b.counts.size, b.score.size
    ph = b.phys
    arrs = [np.ascontiguousarray(a) for a in (b.counts, b.maxfreq, b.qexpand, b.score[ph], b.order[ph], b.position[ph], b.vocab[ph],
                                              b.freq[ph], b.via[ph])]
    out_count = np.zeros(max(nq, 1), dtype=np.uint32)
    out_rows = np.zeros(max(total, 1), dtype=DEVROW)
    ptr = [a.ctypes.data if a.size else None for a in arrs]
    if not P.any_variants:
        ptr[8] = None  # no row has a via
    rc = L.lib().anx_debug_rank_rows(0, nq, *ptr, P.cutoff, P.max_matches, P.freq_weight, P.have_freq, P.any_variants, seg_cap,
                                     total if row_cap is None else row_cap, overflow, out_count.ctypes.data, out_rows.ctypes.data)
    assert rc == 0, L.last_error()
    return out_count[:nq], out_rows[:total]


def ranked(b, count, rows):
    """the r_count[q] rows from soff[q] of every query, back to back"""
    soff = b.soff
    assert (count <= b.counts).all(), "r_count beyond the query's candidate rows"
    idx = np.concatenate([np.arange(s, s + c) for s, c in zip(soff[:-1], count.astype(np.int64))]) if count.size else np.zeros(0, dtype=np.int64)
    return rows[idx.astype(np.int64)]


def check(b, count, rows, what):
    ecount, evocab, evia, edist, efreq = R.reference(b)
    bad = np.nonzero(count != ecount)[0]
    assert bad.size == 0, (what, b.params, "r_count of query", int(bad[0]), "rows", int(b.counts[bad[0]]), "got", int(count[bad[0]]), "expected", int(ecount[bad[0]]))
    got = ranked(b, count, rows)
    qof = np.repeat(np.arange(count.size), count.astype(np.int64))
    for name, exp in (("vocab_id", evocab), ("via", evia), ("dist_score", edist), ("freq_score", efreq)):
        bad = np.nonzero(~(got[name] == exp))[0]
        assert bad.size == 0, (what, b.params, name, "query", int(qof[bad[0]]), "rows", int(b.counts[qof[bad[0]]]), "ranked row",
                               int(bad[0] - np.concatenate([[0], np.cumsum(count)])[qof[bad[0]]]), got[name][bad[0]], exp[bad[0]])


@pytest.mark.parametrize("group", sorted(R.main_groups()), ids=lambda g: "freq%d-variants%d-fw%g" % g)
def test_crossed_parameters(group):
    """max_matches x cutoff_threshold for one (have_freq, any_variants, freq_weight): every list length, quadruple and population"""
    for P in R.main_groups()[group]:
        b = R.main_batch(P)
        check(b, *rank_raw(b), "main")


def test_partly_filled_wave_and_block():
    for b in R.small_nq_batches():
        check(b, *rank_raw(b), "nq %d" % b.counts.size)


def test_2000_equal_rows_rank_query_all():
    for b in R.equal2000_batches():
        check(b, *rank_raw(b), "2000 equal rows")


def test_lists_beyond_65535_rows():
    """quickselect on lists of 65 535 / 65 536 / 65 537 / 70 000 rows whose best rows lie at the highest physical indices: the rows that
    come out are fetched back by their source index, which has to reach beyond 65 535"""
    for b in R.long_batches():
        check(b, *rank_raw(b), "long lists")


@pytest.mark.parametrize("have_freq", [0, 1])
def test_segments_equal_row_buffer(have_freq):
    """rows i < C in per-query segment records + entry records, the surplus in the row buffer: byte for byte what seg_cap 0 gives"""
    for P in R.segment_params():
        if P.have_freq != have_freq:
            continue
        b = R.main_batch(P)
        count, rows = rank_raw(b)
        check(b, count, rows, "seg_cap 0")
        for C in R.SEG_CAPS:
            assert (b.counts < C).any() and (b.counts == C).any() and (b.counts > C).any()
            c2, r2 = rank_raw(b, seg_cap=C)
            assert c2.tobytes() == count.tobytes() and r2.tobytes() == rows.tobytes(), (P, C)


def test_early_return_writes_nothing():
    b = R.main_batch(R.Params(10, 2.0, 0.0, 1, 0))
    total = b.score.size
    for kw in (dict(row_cap=total - 1), dict(overflow=1), dict(overflow=0x80000000)):
        count, rows = rank_raw(b, **kw)
        assert (count.view(np.uint8) == 0xFF).all() and (rows.view(np.uint8) == 0xFF).all(), kw
    count, rows = rank_raw(b, row_cap=total)  # exactly full: runs
    check(b, count, rows, "row_cap == total")


def test_hook_rejects_what_segments_cannot_hold():
    b = R.main_batch(R.Params(10, 2.0, 0.0, 1, 1))
    with pytest.raises(AssertionError):
        rank_raw(b, seg_cap=16)
