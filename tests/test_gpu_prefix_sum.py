"""The exclusive prefix sum of the run and of the fetch / export paths (kernels_prefix.hpp) by itself, through anx_debug_exclusive_scan,
against numpy.cumsum.  Up to 1024 blocks of 2048 elements two kernels do it (k_scan_add adds up the block totals in front of its block,
block 0 all of them for out[n]); above that the three-kernel form with k_scan_sums runs.  Sizes: one element, one block minus one /
exactly / plus one element, 257 blocks (the pass over the block totals goes round its loop of 256 threads a second time) and 1026
blocks (beyond the two-kernel form)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from analiticcl_amd import _lib as L

TILE = 2048


def _scan(v, want_copy=True):
    n = v.size
    out = np.full(n + 1, 0xDEADBEEF, dtype=np.uint32)
    copy = np.full(max(n, 1), 0xDEADBEEF, dtype=np.uint32)
    rc = L.lib().anx_debug_exclusive_scan(0, v.ctypes.data if n else None, n, out.ctypes.data, copy.ctypes.data if want_copy else None)
    assert rc == 0, L.last_error()
    return out, copy[:n]


@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 256 * TILE + 1, 1025 * TILE + 1])
def test_prefix_sum_equals_cumsum(n):
    rng = np.random.default_rng(n)
    v = rng.integers(0, 1000, n, dtype=np.uint32)
    exp = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(v, dtype=np.uint64, out=exp[1:])
    assert exp[-1] < 2**32
    out, copy = _scan(v)
    assert int(out[n]) == int(exp[n])
    assert np.array_equal(out, exp.astype(np.uint32))
    assert np.array_equal(copy, out[:n])
    out2, _ = _scan(v, want_copy=False)
    assert np.array_equal(out2, out)


def test_prefix_sum_of_nothing():
    out, _ = _scan(np.zeros(0, dtype=np.uint32))
    assert out.tolist() == [0]
