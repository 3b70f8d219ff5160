"""The entry points of the compact records with `via` answer ANX_EINVAL to NULL arguments, without a device."""
import ctypes as C

from analiticcl_amd import _lib as L


def test_null_arguments_are_refused():
    lib = L.lib()
    rows, offs, via, n = C.c_void_p(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_size_t()
    assert lib.anx_batch_fetch_compact_via(None, C.byref(rows), C.byref(offs), C.byref(via)) == L.ANX_EINVAL
    assert "NULL" in L.last_error()
    assert lib.anx_pipeline_next_via(None, C.byref(rows), C.byref(offs), C.byref(via), C.byref(n)) == L.ANX_EINVAL
    assert "NULL" in L.last_error()
    assert not rows.value and not offs and not via
    out = (L.Result * 1)()
    out[0].vocab_id = 7
    lib.anx_compact_to_results_via(None, None, 1, out)   # (void: nothing is written)
    assert out[0].vocab_id == 7
