"""Python mirror of analiticcl's Python API for the variant-query path, on top of the anx C ABI.

Same class / method / keyword names as the reference's pyo3 binding
(/root/reference/bindings/python/src/lib.rs:591-812, typed in /root/reference/analiticcl.pyi):
`VariantModel`, `SearchParameters`, `Weights`, `VocabParams`; `find_variants`, `find_variants_par`.
All scoring runs on the GPU through libanx.so; nothing is computed in Python.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

from . import _lib as L


def _threshold(v) -> L.Threshold:
    """int -> Absolute, float in [0,1] -> Ratio, (float, int) -> RatioWithLimit
    (bindings/python/src/lib.rs extract_distance_threshold; src/types.rs:85-108)."""
    if isinstance(v, bool):
        raise ValueError("distance threshold must be int, float or (float, int)")
    if isinstance(v, int):
        if not 0 <= v <= 255:
            raise ValueError("absolute distance threshold must fit in u8")
        return L.Threshold(0, v, 0.0)
    if isinstance(v, float):
        if not 0.0 <= v <= 1.0:
            raise ValueError("ratio must be in range 0.0-1.0")
        return L.Threshold(1, 0, v)
    if isinstance(v, (tuple, list)) and len(v) == 2:
        return L.Threshold(2, int(v[1]), float(v[0]))
    raise ValueError("distance threshold must be int, float or (float, int)")


class Weights:
    """Weights of the score components (src/types.rs:40-73)."""

    _names = ("ld", "lcs", "prefix", "suffix", "case")

    def __init__(self, **kwargs):
        self.ld, self.lcs, self.prefix, self.suffix, self.case = 0.5, 0.125, 0.125, 0.125, 0.125
        for k, v in kwargs.items():
            if k not in self._names:
                raise ValueError(f"Unknown parameter for Weights: {k}")
            setattr(self, k, float(v))

    def _c(self) -> L.Weights:
        return L.Weights(self.ld, self.lcs, self.prefix, self.suffix, self.case)

    def to_dict(self) -> dict:
        return {k: getattr(self, k) for k in self._names}

    def get_ld(self): return self.ld
    def get_lcs(self): return self.lcs
    def get_prefix(self): return self.prefix
    def get_suffix(self): return self.suffix
    def get_case(self): return self.case
    def set_ld(self, value): self.ld = float(value)
    def set_lcs(self, value): self.lcs = float(value)
    def set_prefix(self, value): self.prefix = float(value)
    def set_suffix(self, value): self.suffix = float(value)
    def set_case(self, value): self.case = float(value)


class SearchParameters:
    """SearchParameters (src/types.rs:112-192); defaults are the library defaults (k=3, d=3, n=20)."""

    _defaults = dict(max_anagram_distance=3, max_edit_distance=3, max_matches=20, score_threshold=0.25,
                     cutoff_threshold=2.0, stop_criterion=False, max_ngram=3, lm_order=3, max_seq=250,
                     single_thread=False, context_weight=0.0, variantmodel_weight=3.0, lm_weight=1.0,
                     contextrules_weight=1.0, freq_weight=0.0, consolidate_matches=True, unicodeoffsets=False)

    def __init__(self, **kwargs):
        self.__dict__.update(self._defaults)
        for k, v in kwargs.items():
            if k not in self._defaults:
                raise ValueError(f"Unknown parameter for SearchParameters: {k}")
            setattr(self, k, v)

    def _c(self) -> L.Params:
        return L.Params(_threshold(self.max_anagram_distance), _threshold(self.max_edit_distance),
                        int(self.max_matches), float(self.score_threshold), float(self.cutoff_threshold),
                        1 if self.stop_criterion else 0, float(self.freq_weight))

    def _c_search(self) -> L.SearchParams:
        return L.SearchParams(self._c(), int(self.max_ngram), int(self.max_seq), float(self.lm_weight),
                              float(self.variantmodel_weight), float(self.contextrules_weight),
                              1 if self.unicodeoffsets else 0)

    def to_dict(self) -> dict:
        return {k: getattr(self, k) for k in self._defaults}

    # getters of the pyo3 class (bindings/python/src/lib.rs:261-345, analiticcl.pyi:75-137)
    @staticmethod
    def _threshold_value(v):
        """Absolute -> int, Ratio -> float, RatioWithLimit -> {"ratio", "limit"} (bindings/python/src/lib.rs:261-292)."""
        if isinstance(v, (tuple, list)):
            return {"ratio": float(v[0]), "limit": int(v[1])}
        return v

    def get_max_anagram_distance(self): return self._threshold_value(self.max_anagram_distance)
    def get_max_edit_distance(self): return self._threshold_value(self.max_edit_distance)
    def get_edit_distance(self): return self.get_max_edit_distance()  # the name analiticcl.pyi:81 documents
    def get_max_matches(self) -> int: return int(self.max_matches)
    def get_score_threshold(self) -> float: return float(self.score_threshold)
    def get_cutoff_threshold(self) -> float: return float(self.cutoff_threshold)
    def get_stop_criterion(self) -> bool: return bool(self.stop_criterion)
    def get_max_ngram(self) -> int: return int(self.max_ngram)
    def get_lm_order(self) -> int: return int(self.lm_order)
    def get_max_seq(self) -> int: return int(self.max_seq)
    def get_single_thread(self) -> bool: return bool(self.single_thread)
    def get_context_weight(self) -> float: return float(self.context_weight)
    def get_variantmodel_weight(self) -> float: return float(self.variantmodel_weight)
    def get_lm_weight(self) -> float: return float(self.lm_weight)
    def get_contextrules_weight(self) -> float: return float(self.contextrules_weight)
    def get_freq_weight(self) -> float: return float(self.freq_weight)
    def get_consolidate_matches(self) -> bool: return bool(self.consolidate_matches)
    def get_unicodeoffsets(self) -> bool: return bool(self.unicodeoffsets)


class VocabParams:
    """VocabParams (src/vocab.rs:108-143)."""

    _fh = {"sum": 0, "max": 1, "min": 2, "replace": 3}
    _vt = {"NONE": 0, "INDEXED": 1, "LM": 2, "TRANSPARENT": 4}

    def __init__(self, **kwargs):
        self.text_column, self.freq_column, self.freq_handling, self.vocabtype = 0, 1, "max", "INDEXED"
        for k, v in kwargs.items():
            if k not in ("text_column", "freq_column", "freq_handling", "vocabtype"):
                raise ValueError(f"Unknown parameter for VocabParams: {k}")
            setattr(self, k, v)

    def _c(self) -> L.VocabParams:
        vt = self.vocabtype
        vtv = vt if isinstance(vt, int) else sum(self._vt[x.strip().upper()] for x in vt.split("|"))
        return L.VocabParams(int(self.text_column), -1 if self.freq_column is None else int(self.freq_column),
                             self._fh[self.freq_handling.lower()], vtv)


def _b(s) -> bytes:
    return s if isinstance(s, bytes) else s.encode("utf-8")


def _pack(inputs: Sequence) -> bytes:
    """n inputs -> one buffer, each terminated by a NUL byte; an input with an embedded NUL is cut there, exactly as the
    char* entry points would."""
    if not len(inputs):
        return b""
    try:
        blob = ("\0".join(inputs) + "\0").encode("utf-8")          # all str: one join, one encode
    except TypeError:
        blob = b"\0".join(_b(t) for t in inputs) + b"\0"
    if blob.count(b"\0") != len(inputs):
        blob = b"\0".join(_b(t).split(b"\0", 1)[0] for t in inputs) + b"\0"
    return blob


def edit_script(source: str, target: str) -> str:
    """sesdiff::shortest_edit_script(source, target) in sesdiff notation (anx_edit_script)."""
    buf = C.create_string_buffer(4 * (len(_b(source)) + len(_b(target))) + 64)
    L.check(min(0, L.lib().anx_edit_script(_b(source), _b(target), buf, len(buf))))
    return buf.value.decode("utf-8")


def _result_columns(rows, total: int):
    """anx_result[total] -> (vocab_id, dist_score, freq_score, via) as Python lists, converted in bulk (element-wise
    ctypes access costs about a microsecond per field)."""
    import numpy as np
    if total == 0:
        return [], [], [], []
    dt = np.dtype([("vocab_id", "<u8"), ("dist", "<f8"), ("freq", "<f8"), ("via", "<u8")])
    a = np.frombuffer((C.c_char * (total * dt.itemsize)).from_address(C.addressof(rows.contents)), dtype=dt)
    return a["vocab_id"].tolist(), a["dist"].tolist(), a["freq"].tolist(), a["via"].tolist()


def _offsets(offs, n: int) -> List[int]:
    import numpy as np
    return np.ctypeslib.as_array(offs, shape=(n + 1,)).tolist()


def _compact_views(rows, offs, via, n: int):
    """numpy views of one block of compact records ([rows | offsets] or [rows | via | offsets]): ONE owner for the whole block, which
    every view keeps alive through .base and whose collection releases the block (anx_compact_free)."""
    import weakref

    import numpy as np
    dt = np.dtype([("vocab_id", "<u4"), ("freq_score", "<f4"), ("dist_score", "<f8")])
    off_addr = C.addressof(offs.contents)
    owner = (C.c_char * (off_addr - rows.value + (n + 1) * 4)).from_address(rows.value)
    weakref.finalize(owner, L.lib().anx_compact_free, rows, offs)
    off = np.frombuffer(owner, dtype="<u4", count=n + 1, offset=off_addr - rows.value)
    total = int(off[-1])
    rec = np.frombuffer(owner, dtype=dt, count=total)
    if via is None:
        return off, rec
    return off, rec, np.frombuffer(owner, dtype="<u4", count=total, offset=C.addressof(via.contents) - rows.value)


class Batch:
    """A batch of queries encoded and resident in HBM (anx_batch_*): encode once, run many times."""

    def __init__(self, model: "VariantModel", inputs: Sequence[str], params: SearchParameters, packed: Optional[bytes] = None,
                 n: Optional[int] = None, device_ptr: Optional[int] = None, nbytes: int = 0, src_stream: Optional[int] = None):
        """inputs: the query strings; or packed + n: the same as ONE bytes object, every input followed by a NUL byte (what a
        caller that reads its queries from a file or a socket already has: the buffer goes to the device as it is)."""
        self.model = model
        cp = params._c()
        # one NUL-terminated buffer instead of a pointer array (anx_batch_encode_packed)
        if device_ptr is not None:   # the packed buffer already sits in HBM (anx_batch_encode_packed_device)
            self.n = int(n)
            if src_stream is None:   # the buffer is complete (its producer has been waited for)
                self.h = L.lib().anx_batch_encode_packed_device(model.h, C.c_void_p(device_ptr), int(nbytes), self.n, C.byref(cp))
            else:                    # ordered behind what the stream holds now (anx_batch_encode_packed_device_on)
                self.h = L.lib().anx_batch_encode_packed_device_on(model.h, C.c_void_p(device_ptr), int(nbytes), self.n, C.byref(cp), C.c_void_p(src_stream))
        else:
            blob = _pack(inputs) if packed is None else packed
            self.n = len(inputs) if packed is None else int(n)
            self.h = L.lib().anx_batch_encode_packed(model.h, blob, len(blob), self.n, C.byref(cp))
        if not self.h:
            raise L.AnxError(L.ANX_ENODEVICE if "device" in L.last_error() else L.ANX_EINVAL, L.last_error())
        self.freq_weight = float(params.freq_weight)

    def run(self, stream: int = 0):
        L.check(L.lib().anx_batch_run(self.model.h, self.h, C.c_void_p(stream)))

    def run_async(self, stream: int = 0):
        """Enqueue the run on `stream` and return (anx_batch_run_async); wait() completes it."""
        L.check(L.lib().anx_batch_run_async(self.model.h, self.h, C.c_void_p(stream)))

    def wait(self):
        L.check(L.lib().anx_batch_wait(self.model.h, self.h))

    def shards(self) -> List[tuple]:
        """[(device, first_input, n_inputs)]: the replicas of a multi-device model this batch is spread over."""
        out = []
        for g in range(L.lib().anx_batch_num_shards(self.h)):
            dev, lo, cnt = C.c_int(), C.c_size_t(), C.c_size_t()
            L.check(L.lib().anx_batch_shard_info(self.h, g, C.byref(dev), C.byref(lo), C.byref(cnt)))
            out.append((dev.value, lo.value, cnt.value))
        return out

    def shard_inputs(self, shard: int):
        """Indices (ascending) of the inputs shard `shard` holds under the length-partitioned split, None for a consecutive range."""
        import numpy as np
        dev, lo, cnt = C.c_int(), C.c_size_t(), C.c_size_t()
        L.check(L.lib().anx_batch_shard_info(self.h, shard, C.byref(dev), C.byref(lo), C.byref(cnt)))
        ix = C.POINTER(C.c_uint32)()
        L.check(L.lib().anx_batch_shard_inputs(self.h, shard, C.byref(ix)))
        return np.ctypeslib.as_array(ix, shape=(cnt.value,)).copy() if ix else None

    def stats(self) -> dict:
        s = L.BatchStats()
        L.check(L.lib().anx_batch_get_stats(self.h, C.byref(s), C.sizeof(s)))
        return {k: (list(getattr(s, k)) if k == "n_tests_kind" else getattr(s, k)) for k, _ in L.BatchStats._fields_}

    def fetch(self) -> List[List[tuple]]:
        """-> per query, ranked [(vocab_id, dist_score, freq_score)]"""
        rows = C.POINTER(L.Result)()
        offs = C.POINTER(C.c_size_t)()
        L.check(L.lib().anx_batch_fetch(self.h, C.byref(rows), C.byref(offs)))
        try:
            off = _offsets(offs, self.n)
            v, d, f, _via = _result_columns(rows, off[-1])
            return [list(zip(v[off[i]:off[i + 1]], d[off[i]:off[i + 1]], f[off[i]:off[i + 1]])) for i in range(self.n)]
        finally:
            L.lib().anx_results_free(rows, offs)

    def fetch_arrays(self):
        """-> (offsets[n+1], vocab_id[R], dist_score[R], freq_score[R]) as numpy arrays (CSR, batch order).  The three
        row arrays are strided VIEWS of the library's result buffer (32-byte anx_result records), which is released when
        the last of them is garbage collected: no second copy of the rows (141 MB per million queries of config 2)."""
        import weakref

        import numpy as np
        rows = C.POINTER(L.Result)()
        offs = C.POINTER(C.c_size_t)()
        L.check(L.lib().anx_batch_fetch(self.h, C.byref(rows), C.byref(offs)))
        release = True
        try:
            off = np.ctypeslib.as_array(offs, shape=(self.n + 1,)).astype(np.int64)
            total = int(off[-1])
            if total == 0:
                z = np.zeros(0)
                return off, z.astype(np.uint64), z, z
            dt = np.dtype([("vocab_id", "<u8"), ("dist", "<f8"), ("freq", "<f8"), ("via", "<u8")])
            owner = (C.c_char * (total * dt.itemsize)).from_address(C.addressof(rows.contents))
            weakref.finalize(owner, L.lib().anx_results_free, rows, offs)  # the views keep `owner` alive through .base
            release = False
            a = np.frombuffer(owner, dtype=dt)
            return off, a["vocab_id"], a["dist"], a["freq"]
        finally:
            if release:
                L.lib().anx_results_free(rows, offs)

    def fetch_compact(self, with_via: bool = False):
        """-> (offsets[n+1] uint32, rows) with rows a structured array of 16-byte records (vocab_id u32, freq_score f32, dist_score
        f64): anx_batch_fetch_compact, half the bytes of fetch_arrays over PCIe.  Views of the library's pinned block, which is
        released when the last of them is garbage collected.  Not for models with variant lists or confusables.
        with_via: -> (offsets, rows, via) through anx_batch_fetch_compact_via, for every model, variant lists included: via[r] is
        the vocabulary id of the variant row r was reached through, 0xFFFFFFFF = none (uint32, one word per row)."""
        rows = C.c_void_p()
        offs = C.POINTER(C.c_uint32)()
        via = C.POINTER(C.c_uint32)()
        if with_via:
            L.check(L.lib().anx_batch_fetch_compact_via(self.h, C.byref(rows), C.byref(offs), C.byref(via)))
        else:
            L.check(L.lib().anx_batch_fetch_compact(self.h, C.byref(rows), C.byref(offs)))
        return _compact_views(rows, offs, via if with_via else None, self.n)

    MEASURES_DTYPE = [("score", "<f8"), ("ld", "u1"), ("lcs", "u1"), ("prefixlen", "u1"), ("suffixlen", "u1"), ("len_input", "u1"),
                      ("len_entry", "u1"), ("anagram_distance", "u1"), ("flags", "u1")]

    def fetch_measures(self):
        """-> (offsets[n+1] uint32, measures): anx_batch_fetch_measures, why every ranked row got its score.  measures is a structured
        array of 16-byte records (MEASURES_DTYPE); record r describes row r of fetch_compact(with_via=True) on this batch: the
        unrestricted edit distance, common substring / prefix / suffix, the lengths in symbols, the anagram distance, flags (bit 0
        samecase, bit 1 the row has a via: the scored entry is the via item) and the unweighted distance score of (input, scored
        entry).  Views of the library's pinned block, which is released when the last of them is garbage collected."""
        import weakref

        import numpy as np
        rows = C.c_void_p()
        offs = C.POINTER(C.c_uint32)()
        L.check(L.lib().anx_batch_fetch_measures(self.h, C.byref(rows), C.byref(offs)))
        off_addr = C.addressof(offs.contents)
        owner = (C.c_char * (off_addr - rows.value + (self.n + 1) * 4)).from_address(rows.value)
        weakref.finalize(owner, L.lib().anx_measures_free, rows, offs)
        off = np.frombuffer(owner, dtype="<u4", count=self.n + 1, offset=off_addr - rows.value)
        return off, np.frombuffer(owner, dtype=np.dtype(self.MEASURES_DTYPE), count=int(off[-1]))

    def fetch_pairs(self) -> List[tuple]:
        """-> every scored pair (query, vocab_id, ld|-1, lcs, prefixlen, suffixlen, samecase, score)"""
        pairs = C.POINTER(L.Pair)()
        n = C.c_size_t()
        L.check(L.lib().anx_batch_fetch_pairs(self.h, C.byref(pairs), C.byref(n)))
        try:
            return [(pairs[i].query, pairs[i].vocab_id, pairs[i].ld, pairs[i].lcs, pairs[i].prefixlen,
                     pairs[i].suffixlen, pairs[i].samecase, pairs[i].score) for i in range(n.value)]
        finally:
            L.lib().anx_pairs_free(pairs)

    def pair_counts(self):
        """Scored pairs per input, counted by the scan of a production run (anx_batch_pair_counts) -> numpy uint32[n]."""
        import numpy as np
        out = C.POINTER(C.c_uint32)()
        L.check(L.lib().anx_batch_pair_counts(self.h, C.byref(out)))
        try:
            return np.ctypeslib.as_array(out, shape=(max(self.n, 1),))[:self.n].copy()
        finally:
            L.lib().anx_counts_free(out)

    def export_topk(self, device_ptr: int, stride: int, stream: int = 0, via_ptr: Optional[int] = None):
        """`stride` records per input into a device buffer of n * stride * 16 bytes.  via_ptr: a second device buffer of n * stride
        uint32 that receives the `via` of every slot (anx_batch_export_topk_via; 0xFFFFFFFF = none / unused slot), for every model."""
        if via_ptr is None:
            L.check(L.lib().anx_batch_export_topk(self.h, C.c_void_p(device_ptr), stride, C.c_void_p(stream)))
        else:
            L.check(L.lib().anx_batch_export_topk_via(self.h, C.c_void_p(device_ptr), C.c_void_p(via_ptr), stride, C.c_void_p(stream)))

    def export_compact(self, device_ptr: int, capacity: int, stream: int = 0, with_via: bool = False) -> int:
        """offsets[n+1] (u32, padded to 16 bytes) + unpadded records into a device buffer; returns the bytes used.
        with_via: followed by one uint32 `via` per record (anx_batch_export_compact_via: every model, variant lists included)."""
        used = C.c_size_t(0)
        fn = L.lib().anx_batch_export_compact_via if with_via else L.lib().anx_batch_export_compact
        L.check(fn(self.h, C.c_void_p(device_ptr), capacity, C.c_void_p(stream), C.byref(used)))
        return used.value

    def gather_compact(self, dst_device: int, device_ptr: int, capacity: int, with_via: bool = False):
        """anx_batch_gather_compact: every shard's compact export in one buffer on device dst_device (the shards' own devices copy
        their sections over) -> (section offsets [shards + 1], bytes used).  with_via: every section in export_compact(with_via=True)'s
        layout (anx_batch_gather_compact_via)."""
        import numpy as np
        ns = L.lib().anx_batch_num_shards(self.h)
        offs = (C.c_size_t * (ns + 1))()
        used = C.c_size_t(0)
        fn = L.lib().anx_batch_gather_compact_via if with_via else L.lib().anx_batch_gather_compact
        L.check(fn(self.h, dst_device, C.c_void_p(device_ptr), capacity, offs, C.byref(used)))
        return np.array(list(offs), dtype=np.int64), used.value

    def free(self):
        if getattr(self, "h", None):
            L.lib().anx_batch_free(self.h)
            self.h = None

    def __del__(self):
        self.free()


class Pipeline:
    """anx_pipeline: encode / run / fetch of consecutive packed batches overlapped for one caller thread.  submit() hands over a
    bytes object (every input followed by a NUL byte) and returns at once (or blocks while `depth` jobs are in flight); next()
    returns the oldest job's (offsets, rows) as Batch.fetch_compact does."""

    def __init__(self, model: "VariantModel", depth: int = 6):
        self.model = model
        self.h = L.lib().anx_pipeline_new(model.h, depth)
        if not self.h:
            raise L.AnxError(L.lib().anx_last_error_code(), L.lib().anx_last_error().decode("utf-8", "replace"))
        self._keep = []  # the submitted buffers stay alive until their results were returned

    def submit(self, packed: bytes, n: int, params: "SearchParameters"):
        """Raises AnxError (ANX_ELIMIT) when `depth` jobs are in flight: take a result with next() first."""
        L.check(L.lib().anx_pipeline_submit_packed(self.h, packed, len(packed), n, C.byref(params._c())))
        self._keep.append(packed)

    def pending(self) -> int:
        return L.lib().anx_pipeline_pending(self.h)

    def next(self, with_via: bool = False):
        """with_via: -> (offsets, rows, via) through anx_pipeline_next_via, as Batch.fetch_compact(with_via=True): what a model with
        variant lists needs (next() without it raises ANX_EINVAL for such a model's jobs)."""
        rows = C.c_void_p()
        offs = C.POINTER(C.c_uint32)()
        via = C.POINTER(C.c_uint32)()
        n = C.c_size_t()
        if with_via:
            L.check(L.lib().anx_pipeline_next_via(self.h, C.byref(rows), C.byref(offs), C.byref(via), C.byref(n)))
        else:
            L.check(L.lib().anx_pipeline_next(self.h, C.byref(rows), C.byref(offs), C.byref(n)))
        self._keep.pop(0)
        return _compact_views(rows, offs, via if with_via else None, n.value)

    def close(self):
        if self.h:
            L.lib().anx_pipeline_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


class VariantModel:
    """VariantModel (src/lib.rs:50-100) for the query path; `device` = HIP device ordinal
    (default: $LOCAL_RANK or 0; -1 = host index only).  `devices` = a list of ordinals: one process drives a replica of the
    lexicon on each of them (anx_model_to_devices) and every batch call shards its inputs over the replicas."""

    def __init__(self, alphabet_file: str, weights: Optional[Weights] = None, debug: int = 0,
                 device: Optional[int] = None, alphabet_text: Optional[str] = None, devices: Optional[List[int]] = None):
        w = (weights or Weights())._c()
        lib = L.lib()
        if alphabet_text is not None:
            self.h = lib.anx_model_new_with_alphabet(_b(alphabet_text), C.byref(w), debug)
        else:
            self.h = lib.anx_model_new(_b(alphabet_file), C.byref(w), debug)
        if not self.h:
            raise L.AnxError(L.ANX_EIO, L.last_error())
        self.devices = list(devices) if devices else None
        self.device = self.devices[0] if self.devices else (int(os.environ.get("LOCAL_RANK", "0")) if device is None else device)
        self.lexicons: List[str] = []

    def __del__(self):
        try:
            if getattr(self, "h", None):
                L.lib().anx_model_free(self.h)
                self.h = None
        except Exception:  # interpreter shutdown: the module globals are already gone
            pass

    # -- loading -----------------------------------------------------------------------------------
    def read_vocabulary(self, filename: str, params: Optional[VocabParams] = None):
        self.__dict__.pop("_vocab_cache", None)
        p = (params or VocabParams())._c()
        L.check(L.lib().anx_model_read_vocabulary(self.h, _b(filename), C.byref(p)))
        self.lexicons.append(filename)

    def read_lexicon(self, filename: str):
        self.__dict__.pop("_vocab_cache", None)
        self.read_vocabulary(filename, VocabParams())

    def add_to_vocabulary(self, text: str, frequency: Optional[int] = None, params: Optional[VocabParams] = None):
        self.__dict__.pop("_vocab_cache", None)
        p = (params or VocabParams())._c()
        return L.lib().anx_model_add_to_vocabulary(self.h, _b(text), 0 if frequency is None else 1,
                                                   frequency or 0, C.byref(p))

    def add_variant(self, ref_id: int, variant: str, score: float, frequency: Optional[int] = None,
                    params: Optional[VocabParams] = None) -> bool:
        """add_variant (src/lib.rs:460): link `variant` to the reference item `ref_id` with a score"""
        self.__dict__.pop("_vocab_cache", None)
        p = (params or VocabParams())._c()
        rc = L.lib().anx_model_add_variant(self.h, ref_id, _b(variant), float(score), 0 if frequency is None else 1,
                                           frequency or 0, C.byref(p))
        if rc < 0:
            L.check(rc)
        return bool(rc)

    def read_variants(self, filename: str, transparent: bool = False):
        """Load a weighted variant list; transparent=True for error lists whose items are never returned themselves
        (bindings/python/src/lib.rs:671-681)"""
        self.__dict__.pop("_vocab_cache", None)
        p = VocabParams()._c()
        L.check(L.lib().anx_model_read_variants(self.h, _b(filename), C.byref(p), 1 if transparent else 0))
        self.lexicons.append(filename)

    def build(self):
        self.__dict__.pop("_vocab_cache", None)
        if self.devices and len(self.devices) > 1:
            L.check(L.lib().anx_model_build(self.h, -1))
            self.to_devices(self.devices)
        else:
            L.check(L.lib().anx_model_build(self.h, self.device))

    def set_index_tag(self, tag: str):
        """Stored in the image save_index writes: what the model was built from (see index_tag_of)."""
        L.check(L.lib().anx_model_set_index_tag(self.h, _b(tag)))

    @staticmethod
    def index_tag_of(filename: str) -> Optional[str]:
        """The tag of an index image without loading it; None if the file is not an image of this library version."""
        p = L.lib().anx_index_read_tag(_b(filename))
        if not p:
            return None
        try:
            return C.string_at(p).decode("utf-8", "replace")
        finally:
            L.lib().anx_string_free(p)

    def save_index(self, filename: str):
        """Write the built model (vocabulary + the lexicon image the GPU consumes) to disk (anx_model_save_index)."""
        L.check(L.lib().anx_model_save_index(self.h, _b(filename)))

    def load_index(self, filename: str):
        """Instead of read_lexicon / read_variants / build: load an image written by save_index for the same alphabet."""
        self.__dict__.pop("_vocab_cache", None)
        multi = bool(self.devices and len(self.devices) > 1)
        L.check(L.lib().anx_model_load_index(self.h, _b(filename), -1 if multi else self.device))
        if multi:
            self.to_devices(self.devices)
        n = L.lib().anx_model_num_lexicons(self.h) if hasattr(L.lib(), "anx_model_num_lexicons") else 0
        self.lexicons = [L.lib().anx_model_lexicon_name(self.h, i).decode("utf-8") for i in range(n)]

    def to_device(self, device: int):
        self.device = device
        self.devices = None
        L.check(L.lib().anx_model_to_device(self.h, device))

    def to_devices(self, devices: List[int]):
        """One replica of the built lexicon per listed HIP device (an ordinal may repeat); batch calls then shard their inputs
        over the replicas inside this one process (anx_model_to_devices)."""
        arr = (C.c_int * len(devices))(*devices)
        L.check(L.lib().anx_model_to_devices(self.h, arr, len(devices)))
        self.devices = list(devices)
        self.device = self.devices[0]

    @property
    def num_replicas(self) -> int:
        return L.lib().anx_model_num_replicas(self.h)

    def small_replica_stats(self) -> List[int]:
        """Per replica: the small calls (find_variants of at most 4096 short inputs) it has answered since the model went to its
        devices (anx_debug_small_replica_stats) -- a multi-device model spreads such calls over its replicas, each call on one."""
        n = L.lib().anx_model_num_replicas(self.h)
        out = (C.c_uint64 * max(n, 1))()
        got = L.lib().anx_debug_small_replica_stats(self.h, out, n)
        if got < 0:
            L.check(got)
        return [int(out[i]) for i in range(min(n, got))]

    # -- introspection ------------------------------------------------------------------------------
    def __contains__(self, text: str) -> bool:
        return bool(L.lib().anx_model_has(self.h, _b(text)))

    def vocab_text(self, vocab_id: int) -> str:
        return L.lib().anx_model_vocab_text(self.h, vocab_id).decode("utf-8")

    def num_instances(self) -> int:
        return L.lib().anx_model_num_instances(self.h)

    def num_classes(self) -> int:
        return L.lib().anx_model_num_classes(self.h)

    def bucket_size(self, charcount: int) -> int:
        return L.lib().anx_model_bucket_size(self.h, charcount)

    def normalize(self, text: str) -> List[int]:
        buf = C.create_string_buffer(256)
        n = L.lib().anx_model_normalize(self.h, _b(text), buf, 255)
        if n < 0:
            L.check(n)
        return list(buf.raw[:n])

    def anahash(self, text: str) -> int:
        buf = C.create_string_buffer(4096)
        n = L.lib().anx_model_anahash(self.h, _b(text), buf, len(buf))
        if n < 0:
            L.check(n)
        return int(buf.value)

    def length_split(self, inputs: Sequence[str], params: "SearchParameters", n_shards: int, learn_ms=None):
        """Which of n_shards replicas each input would go to under the length-partitioned split of a multi-device model
        (anx_debug_length_split; needs no device): a numpy uint8 array.  learn_ms: measured device times of those shares, fed to
        the split's cost corrections (the next call then returns the corrected split)."""
        import numpy as np
        arr = (C.c_char_p * len(inputs))(*[_b(t) for t in inputs])
        out = np.zeros(len(inputs), dtype=np.uint8)
        ms = np.ascontiguousarray(learn_ms, dtype=np.float64) if learn_ms is not None else None
        L.check(L.lib().anx_debug_length_split(self.h, arr, len(inputs), C.byref(params._c()), n_shards, out.ctypes.data,
                                               ms.ctypes.data if ms is not None else None))
        return out

    # -- the hot path ---------------------------------------------------------------------------------
    def encode_packed(self, packed: bytes, n: int, params: SearchParameters) -> Batch:
        """encode_batch for n inputs already packed into one bytes object, each followed by a NUL byte."""
        return Batch(self, (), params, packed=packed, n=n)

    def encode_packed_device(self, device_ptr: int, nbytes: int, n: int, params: SearchParameters, stream: Optional[int] = None) -> Batch:
        """encode_packed for a packed buffer in device memory (e.g. a torch uint8 tensor's data_ptr()): nothing crosses PCIe.
        stream = None: the buffer must be complete (synchronised) when the call is made; stream = a hipStream_t handle (0 = the default
        stream): the encoder is ordered behind what that stream holds now (the kernel or copy that fills the buffer)."""
        return Batch(self, (), params, n=n, device_ptr=device_ptr, nbytes=nbytes, src_stream=stream)

    def encode_batch(self, inputs: Sequence[str], params: SearchParameters) -> Batch:
        return Batch(self, inputs, params)

    def find_variants_ids(self, inputs: Sequence[str], params: SearchParameters, with_via: bool = False
                          ) -> List[List[tuple]]:
        """anx_find_variants_batch: -> per input, ranked [(vocab_id, dist_score, freq_score[, via | None])]"""
        n = len(inputs)
        arr = (C.c_char_p * max(n, 1))(*[_b(t) for t in inputs])
        cp = params._c()
        rows = C.POINTER(L.Result)()
        offs = C.POINTER(C.c_size_t)()
        L.check(L.lib().anx_find_variants_batch(self.h, arr, n, C.byref(cp), C.byref(rows), C.byref(offs)))
        try:
            off = _offsets(offs, n)
            v, d, f, via = _result_columns(rows, off[-1])
            if with_via:
                via = [None if x == L.ANX_NO_VIA else x for x in via]
                return [list(zip(v[off[i]:off[i + 1]], d[off[i]:off[i + 1]], f[off[i]:off[i + 1]], via[off[i]:off[i + 1]]))
                        for i in range(n)]
            return [list(zip(v[off[i]:off[i + 1]], d[off[i]:off[i + 1]], f[off[i]:off[i + 1]])) for i in range(n)]
        finally:
            L.lib().anx_results_free(rows, offs)

    # -- caller-chosen pairs ----------------------------------------------------------------------------
    PAIR_KEYS = ("score", "ld", "lcs", "prefixlen", "suffixlen", "samecase", "len_a", "len_b", "status")

    def score_pairs_arrays(self, a: Sequence[str], b: Sequence[str], packed: bool = True, weighted: bool = False) -> dict:
        """anx_score_pairs: the model's measures for the pairs (a[i], b[i]) as numpy columns -- score (f64; the dist_score
        find_variants would give the pair, input = a[i]), ld (unrestricted Damerau-Levenshtein, no distance bound), lcs, prefixlen,
        suffixlen (u16), len_a, len_b (symbols), samecase (u8) and status (i8: 0, ANX_EEMPTY for an empty side, ANX_ELIMIT beyond 255
        symbols; score, ld, lcs, prefixlen, suffixlen and samecase of such a pair are 0, len_a / len_b hold the symbols of a side that
        could be normalised and 0 otherwise).  packed = False: the pointer form of the call instead of the packed one.
        weighted = True (anx_score_pairs_weighted): one more column, weight (f64) -- compute_confusable_weight(a[i], b[i]) under the
        model's confusable list, 1.0 without one and for a pair with a status; score * weight is the dist_score of the row
        find_variants ranks on such a model.  The other columns do not change."""
        import numpy as np
        n = len(a)
        if len(b) != n:
            raise ValueError("score_pairs: a and b differ in length")
        dt = np.dtype([("score", "<f8"), ("ld", "<u2"), ("lcs", "<u2"), ("prefixlen", "<u2"), ("suffixlen", "<u2"),
                       ("len_a", "u1"), ("len_b", "u1"), ("samecase", "u1"), ("status", "i1"), ("_pad", "<u4")])
        assert dt.itemsize == C.sizeof(L.PairScore)
        out = np.zeros(max(n, 1), dtype=dt)
        optr = out.ctypes.data_as(C.POINTER(L.PairScore))
        weight = np.ones(max(n, 1), dtype=np.float64) if weighted else None
        wptr = weight.ctypes.data_as(C.POINTER(C.c_double)) if weighted else None
        if packed:
            ba, bb = _pack(a), _pack(b)
            if weighted:
                L.check(L.lib().anx_score_pairs_weighted_packed(self.h, ba, len(ba), bb, len(bb), n, optr, wptr))
            else:
                L.check(L.lib().anx_score_pairs_packed(self.h, ba, len(ba), bb, len(bb), n, optr))
        else:
            aa = (C.c_char_p * max(n, 1))(*[_b(t) for t in a])
            ab = (C.c_char_p * max(n, 1))(*[_b(t) for t in b])
            if weighted:
                L.check(L.lib().anx_score_pairs_weighted(self.h, aa, ab, n, optr, wptr))
            else:
                L.check(L.lib().anx_score_pairs(self.h, aa, ab, n, optr))
        out = out[:n]
        cols = {k: out[k].copy() for k in self.PAIR_KEYS}
        if weighted:
            cols["weight"] = weight[:n]
        return cols

    def score_pairs(self, a: Sequence[str], b: Sequence[str], weighted: bool = False) -> List[dict]:
        """score_pairs_arrays as one dict per pair (keys: score, ld, lcs, prefixlen, suffixlen, samecase, len_a, len_b, status;
        samecase is a bool).  weighted = True adds weight and weighted_score = score * weight (one f64 multiply: the dist_score
        of the ranked row on a model with confusables)."""
        cols = self.score_pairs_arrays(a, b, weighted=weighted)
        lists = {k: cols[k].tolist() for k in self.PAIR_KEYS}
        lists["samecase"] = [bool(x) for x in lists["samecase"]]
        keys = self.PAIR_KEYS
        if weighted:
            lists["weight"] = cols["weight"].tolist()
            lists["weighted_score"] = (cols["score"] * cols["weight"]).tolist()
            keys = keys + ("weight", "weighted_score")
        return [{k: lists[k][i] for k in keys} for i in range(len(a))]

    def confusable_weight_text(self, a: str, b: str) -> float:
        """anx_model_confusable_weight_text: compute_confusable_weight (src/lib.rs:1733-1756) of two strings on the host -- the
        product of the weights of the confusable patterns found in the edit script a -> b.  Needs no device and no build()."""
        w = C.c_double(1.0)
        L.check(L.lib().anx_model_confusable_weight_text(self.h, _b(a), _b(b), C.byref(w)))
        return w.value

    @staticmethod
    def pairs_conf_stats() -> dict:
        """anx_debug_pairs_conf_stats: running totals of the weighted pair calls."""
        out = (C.c_uint64 * 4)()
        L.check(L.lib().anx_debug_pairs_conf_stats(out))
        return {"pairs": int(out[0]), "screened": int(out[1]), "device_scripts": int(out[2]), "host_pairs": int(out[3])}

    # -- confusable mining --------------------------------------------------------------------------------
    MINE_SITE_DTYPE = [("pair", "<u4"), ("a_pos", "<u4"), ("a_len", "<u4"), ("b_pos", "<u4"), ("b_len", "<u4"), ("pattern", "<u4"),
                       ("flags", "<u4"), ("_pad", "<u4")]

    def _mine_call(self, a, b, counts, context, anchors, sites, packed, n=None):
        import numpy as np
        if n is None:
            n = len(a)
            if len(b) != n:
                raise ValueError("mine_confusables: a, b and counts differ in length")
        if counts is not None and len(counts) != n:
            raise ValueError("mine_confusables: a, b and counts differ in length")
        mp = L.MineParams()
        L.lib().anx_default_mine_params(C.byref(mp))
        mp.context, mp.anchors, mp.no_sites = int(context), 1 if anchors else 0, 0 if sites else 1
        cnt = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
        cptr = None if cnt is None else cnt.ctypes.data_as(C.POINTER(C.c_uint32))
        res = C.POINTER(L.MineResult)()
        if packed:
            ba, bb = (a, b) if packed == "blobs" else (_pack(a), _pack(b))
            L.check(L.lib().anx_mine_confusables_packed(self.h, ba, len(ba), bb, len(bb), cptr, n, C.byref(mp), C.byref(res)))
        else:
            aa = (C.c_char_p * max(n, 1))(*[_b(t) for t in a])
            ab = (C.c_char_p * max(n, 1))(*[_b(t) for t in b])
            L.check(L.lib().anx_mine_confusables(self.h, aa, ab, cptr, n, C.byref(mp), C.byref(res)))
        return res

    def mine_confusables_arrays(self, a: Sequence[str], b: Sequence[str], counts=None, context: int = 0, anchors: bool = False,
                                sites: bool = False, packed: bool = True, as_confusables: Optional[tuple] = None,
                                n: Optional[int] = None) -> dict:
        """anx_mine_confusables: the change sites of shortest_edit_script(a[i], b[i]) of every pair and the table of distinct sites in
        confusable-list notation, as numpy arrays -- text (bytes: the patterns back to back), text_off (u64 [D + 1]), count, sites
        (u64 [D]), flags (u32 [D]; bit 0: the pattern holds `[`, `]` or `|` and no list can carry it); rows by count descending, sites
        descending, pattern bytes ascending.  counts: per-pair counts (u32; None: 1 each).  context: 0..8 code points of the
        neighbouring identities; anchors: `^` / `$` where the site begins / ends the script.  sites = True adds site_off (u64 [n + 1])
        and site (a structured array: pair, a_pos, a_len, b_pos, b_len, pattern, flags with bit 0 first / bit 1 last), pair i's sites
        left to right at site[site_off[i]:site_off[i + 1]].  as_confusables = (weight, min_count): one more key, "confusables", the
        list `read_confusablelist` reads (anx_format_confusable_list).  packed = "blobs": a and b are the two NUL-separated byte
        strings anx_mine_confusables_packed takes and n the number of pairs in them."""
        import numpy as np
        res = self._mine_call(a, b, counts, context, anchors, sites, packed, n if packed == "blobs" else None)
        try:
            r = res.contents
            D, n = r.n_patterns, r.n_pairs
            text_off = np.ctypeslib.as_array(r.text_off, shape=(D + 1,)).copy()
            out = {"text": C.string_at(r.text, int(text_off[D])) if D else b"", "text_off": text_off,
                   "count": np.ctypeslib.as_array(r.count, shape=(D,)).copy() if D else np.zeros(0, np.uint64),
                   "sites": np.ctypeslib.as_array(r.sites, shape=(D,)).copy() if D else np.zeros(0, np.uint64),
                   "flags": np.ctypeslib.as_array(r.flags, shape=(D,)).copy() if D else np.zeros(0, np.uint32),
                   "n_sites": int(r.n_sites)}
            if sites:
                out["site_off"] = np.ctypeslib.as_array(r.site_off, shape=(n + 1,)).copy()
                dt = np.dtype(self.MINE_SITE_DTYPE)
                assert dt.itemsize == C.sizeof(L.MineSite)
                out["site"] = (np.frombuffer(C.string_at(r.site, r.n_sites * dt.itemsize), dtype=dt).copy() if r.n_sites
                               else np.zeros(0, dtype=dt))
            if as_confusables is not None:
                txt = C.c_void_p()
                L.check(L.lib().anx_format_confusable_list(res, float(as_confusables[0]), int(as_confusables[1]), C.byref(txt)))
                try:
                    out["confusables"] = C.string_at(txt.value).decode("utf-8", "surrogateescape")
                finally:
                    L.lib().anx_string_free(txt)
            return out
        finally:
            L.lib().anx_mine_result_free(res)

    def mine_confusables(self, a: Sequence[str], b: Sequence[str], counts=None, context: int = 0, anchors: bool = False,
                         sites: bool = False):
        """mine_confusables_arrays as a list of dicts (pattern, count, sites, representable) in table order; with sites = True a pair
        (table, per-pair site lists), a site being a dict (a_pos, a_len, b_pos, b_len, pattern = row of the table, first, last)."""
        r = self.mine_confusables_arrays(a, b, counts, context, anchors, sites)
        off, text = r["text_off"].tolist(), r["text"]
        table = [{"pattern": text[off[k]:off[k + 1]].decode("utf-8", "surrogateescape"), "count": c, "sites": s,
                  "representable": not (f & L.ANX_MINE_UNREPRESENTABLE)}
                 for k, (c, s, f) in enumerate(zip(r["count"].tolist(), r["sites"].tolist(), r["flags"].tolist()))]
        if not sites:
            return table
        so, st = r["site_off"].tolist(), r["site"]
        cols = {k: st[k].tolist() for k in ("a_pos", "a_len", "b_pos", "b_len", "pattern", "flags")}
        recs = [{"a_pos": cols["a_pos"][j], "a_len": cols["a_len"][j], "b_pos": cols["b_pos"][j], "b_len": cols["b_len"][j],
                 "pattern": cols["pattern"][j], "first": bool(cols["flags"][j] & L.ANX_MINE_SITE_FIRST),
                 "last": bool(cols["flags"][j] & L.ANX_MINE_SITE_LAST)} for j in range(len(st))]
        return table, [recs[so[i]:so[i + 1]] for i in range(len(a))]

    @staticmethod
    def mine_stats() -> dict:
        """anx_debug_mine_stats: running totals of the mine calls."""
        out = (C.c_uint64 * 8)()
        L.check(L.lib().anx_debug_mine_stats(out))
        keys = ("device_pairs", "host_pairs", "sites", "patterns", "collision_runs", "odd_shape_pairs", "bytes_up", "bytes_down")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    @staticmethod
    def mine_chunk(chunk: int) -> None:
        """anx_debug_mine_chunk (test hook): pairs per chunk of the mine calls that follow; 0 = the default."""
        L.check(L.lib().anx_debug_mine_chunk(int(chunk)))

    # -- gold evaluation ---------------------------------------------------------------------------------
    GOLD_DTYPE = [("gold_vocab_id", "<u4"), ("rank", "<i4"), ("n_results", "<u4"), ("top_vocab_id", "<u4"), ("gold_score", "<f8"),
                  ("ld", "<u2"), ("k", "u1"), ("d", "u1"), ("status", "i1"), ("reason", "u1"), ("_pad", "<u2")]
    PAIR_DTYPE = [("score", "<f8"), ("ld", "<u2"), ("lcs", "<u2"), ("prefixlen", "<u2"), ("suffixlen", "<u2"),
                  ("len_a", "u1"), ("len_b", "u1"), ("samecase", "u1"), ("status", "i1"), ("_pad", "<u4")]
    GOLD_KEYS = ("gold_vocab_id", "rank", "n_results", "top_vocab_id", "gold_score", "ld", "k", "d", "status", "reason")

    def evaluate_arrays(self, inputs: Sequence[str], gold: Sequence[str], params: SearchParameters, with_pairs: bool = False,
                        packed: bool = True, chunk: Optional[int] = None):
        """anx_evaluate_gold: one record per pair (inputs[i], gold[i]) as a numpy structured array (anx_gold_eval: gold_vocab_id,
        rank, n_results, top_vocab_id, gold_score, ld, k, d, status, reason) -- where gold[i] stands in what find_variants(inputs[i],
        params) returns on this model (rank, -1 = not there) and, if it is not there, the first stage of the pipeline that lost it
        (reason, an index into GOLD_REASONS).  The ranked rows never leave the device.  with_pairs: returns (records, pairs), pairs =
        the anx_pair_score records anx_score_pairs writes for the same pairs.  packed = False: the pointer form of the call; chunk:
        the test hook with a caller-chosen chunk size (pointer form)."""
        import numpy as np
        n = len(inputs)
        if len(gold) != n:
            raise ValueError("evaluate: inputs and gold differ in length")
        dt = np.dtype(self.GOLD_DTYPE)
        assert dt.itemsize == C.sizeof(L.GoldEval)
        out = np.zeros(max(n, 1), dtype=dt)
        optr = out.ctypes.data_as(C.POINTER(L.GoldEval))
        pairs = np.zeros(max(n, 1), dtype=np.dtype(self.PAIR_DTYPE)) if with_pairs else None
        pptr = pairs.ctypes.data_as(C.POINTER(L.PairScore)) if with_pairs else None
        cp = params._c()
        if packed and chunk is None:
            ba, bg = _pack(inputs), _pack(gold)
            L.check(L.lib().anx_evaluate_gold_packed(self.h, ba, len(ba), bg, len(bg), n, C.byref(cp), optr, pptr))
        else:
            aa = (C.c_char_p * max(n, 1))(*[_b(t) for t in inputs])
            ag = (C.c_char_p * max(n, 1))(*[_b(t) for t in gold])
            if chunk is None:
                L.check(L.lib().anx_evaluate_gold(self.h, aa, ag, n, C.byref(cp), optr, pptr))
            else:
                L.check(L.lib().anx_debug_evaluate_gold_chunk(self.h, aa, ag, n, C.byref(cp), optr, pptr, int(chunk)))
        return (out[:n], pairs[:n]) if with_pairs else out[:n]

    def evaluate(self, inputs: Sequence[str], gold: Sequence[str], params: SearchParameters) -> List[dict]:
        """evaluate_arrays as one dict per pair: the record's fields, rank None when gold is not among the rows, gold_vocab_id /
        top_vocab_id None when there is none, and reason as its name (GOLD_REASONS)."""
        rec = self.evaluate_arrays(inputs, gold, params)
        lists = {k: rec[k].tolist() for k in self.GOLD_KEYS}
        out = []
        for i in range(len(inputs)):
            d = {k: lists[k][i] for k in self.GOLD_KEYS}
            d["rank"] = None if d["rank"] < 0 else d["rank"]
            for k in ("gold_vocab_id", "top_vocab_id"):
                d[k] = None if d[k] == 0xFFFFFFFF else d[k]
            d["reason"] = L.GOLD_REASONS[d["reason"]]
            out.append(d)
        return out

    @staticmethod
    def evaluate_summary(records) -> dict:
        """What a tuning run reads off evaluate_arrays' records, computed on the host: n, gold_known (pairs whose gold text is a
        vocabulary item), accuracy_at_1 (gold at rank 0), ranked_share (gold anywhere in the rows), mrr (mean of 1 / (rank + 1), 0 for
        a gold that is not ranked) -- all three over n -- and the count per reason."""
        import numpy as np
        n = int(len(records))
        rank = np.asarray(records["rank"], dtype=np.int64)
        ranked = rank >= 0
        rr = np.zeros(n, dtype=np.float64)
        rr[ranked] = 1.0 / (rank[ranked] + 1.0)
        counts = np.bincount(np.asarray(records["reason"], dtype=np.int64), minlength=len(L.GOLD_REASONS))
        return {"n": n,
                "gold_known": int(np.count_nonzero(np.asarray(records["gold_vocab_id"]) != 0xFFFFFFFF)),
                "accuracy_at_1": float(np.count_nonzero(rank == 0)) / n if n else 0.0,
                "ranked_share": float(np.count_nonzero(ranked)) / n if n else 0.0,
                "mrr": float(rr.sum()) / n if n else 0.0,
                "reasons": {name: int(counts[i]) for i, name in enumerate(L.GOLD_REASONS)}}

    # -- parameter sweep ---------------------------------------------------------------------------------
    SUMMARY_DTYPE = [("n", "<u8"), ("gold_known", "<u8"), ("reasons", "<u8", (8,)), ("rank_hist", "<u8", (L.GOLD_RANK_BINS,)),
                     ("rr_fixed", "<u8"), ("n_results", "<u8"), ("gained_at_1", "<u8"), ("lost_at_1", "<u8")]

    def evaluate_sweep_arrays(self, inputs: Sequence[str], gold: Sequence[str], params_list: Sequence[SearchParameters],
                              with_records: bool = False, with_pairs: bool = False, packed: bool = True, chunk: Optional[int] = None):
        """anx_evaluate_sweep: evaluate_arrays' question for every parameter set of params_list over the same pairs, answered per
        set as a summary the device reduced -- a numpy structured array (SUMMARY_DTYPE = anx_gold_summary: n, gold_known, reasons[8],
        rank_hist[64] with every rank >= 63 in the last bin, rr_fixed = sum of floor(2^32 / (rank + 1)), n_results, gained_at_1 /
        lost_at_1 against params_list[0]) with one element per set.  What does not depend on the set (upload, encoder, pair
        measures, gold lookup) runs once per chunk.  with_records: also the (P, n) array of the records evaluate_arrays returns per
        set; with_pairs: also the anx_pair_score records.  Returns the summaries alone, or a tuple (summaries[, records][, pairs]).
        packed = False: the pointer form of the call; chunk: the test hook with a caller-chosen chunk size (pointer form)."""
        import numpy as np
        n, P = len(inputs), len(params_list)
        if len(gold) != n:
            raise ValueError("evaluate_sweep: inputs and gold differ in length")
        dt = np.dtype(self.SUMMARY_DTYPE)
        assert dt.itemsize == C.sizeof(L.GoldSummary)
        sums = np.zeros(max(P, 1), dtype=dt)
        sptr = sums.ctypes.data_as(C.POINTER(L.GoldSummary))
        sets = (L.Params * max(P, 1))(*[p._c() for p in params_list])
        rec = np.zeros((max(P, 1), max(n, 1)), dtype=np.dtype(self.GOLD_DTYPE)) if with_records else None   # [P][n] set-major (n == 0: untouched)
        optr = rec.ctypes.data_as(C.POINTER(L.GoldEval)) if with_records else None
        pairs = np.zeros(max(n, 1), dtype=np.dtype(self.PAIR_DTYPE)) if with_pairs else None
        pptr = pairs.ctypes.data_as(C.POINTER(L.PairScore)) if with_pairs else None
        if packed and chunk is None:
            ba, bg = _pack(inputs), _pack(gold)
            L.check(L.lib().anx_evaluate_sweep_packed(self.h, ba, len(ba), bg, len(bg), n, sets, P, sptr, optr, pptr))
        else:
            aa = (C.c_char_p * max(n, 1))(*[_b(t) for t in inputs])
            ag = (C.c_char_p * max(n, 1))(*[_b(t) for t in gold])
            if chunk is None:
                L.check(L.lib().anx_evaluate_sweep(self.h, aa, ag, n, sets, P, sptr, optr, pptr))
            else:
                L.check(L.lib().anx_debug_evaluate_sweep_chunk(self.h, aa, ag, n, sets, P, sptr, optr, pptr, int(chunk)))
        res = (sums[:P],) + ((rec[:P, :n],) if with_records else ()) + ((pairs[:n],) if with_pairs else ())
        return res if len(res) > 1 else res[0]

    @staticmethod
    def sweep_summary(s) -> dict:
        """One element of evaluate_sweep_arrays' summaries as a dict: evaluate_summary's keys (accuracy_at_1 = rank_hist[0] / n,
        ranked_share = reasons[RANKED] / n, mrr = rr_fixed / 2^32 / n) plus rank_hist, n_results, gained_at_1 and lost_at_1."""
        n = int(s["n"])
        reasons = [int(x) for x in s["reasons"]]
        hist = [int(x) for x in s["rank_hist"]]
        return {"n": n, "gold_known": int(s["gold_known"]),
                "accuracy_at_1": hist[0] / n if n else 0.0,
                "ranked_share": reasons[L.ANX_GOLD_RANKED] / n if n else 0.0,
                "mrr": int(s["rr_fixed"]) / 4294967296.0 / n if n else 0.0,
                "reasons": {name: reasons[i] for i, name in enumerate(L.GOLD_REASONS)},
                "rank_hist": hist, "n_results": int(s["n_results"]), "gained_at_1": int(s["gained_at_1"]), "lost_at_1": int(s["lost_at_1"])}

    def evaluate_sweep(self, inputs: Sequence[str], gold: Sequence[str], params_list: Sequence[SearchParameters]) -> List[dict]:
        """evaluate_sweep_arrays as one dict per parameter set (sweep_summary)."""
        return [self.sweep_summary(s) for s in self.evaluate_sweep_arrays(inputs, gold, params_list)]

    @staticmethod
    def sweep_stats() -> dict:
        """anx_debug_sweep_stats: running totals of the sweep calls since process start."""
        keys = ("calls", "chunks", "sets", "pair_passes", "lookups", "batch_runs", "bytes_down")
        out = (C.c_uint64 * len(keys))()
        L.check(L.lib().anx_debug_sweep_stats(out, len(keys)))
        return {k: int(out[i]) for i, k in enumerate(keys)}

    # -- weight sweep ------------------------------------------------------------------------------------
    def evaluate_sweep_weights_arrays(self, inputs: Sequence[str], gold: Sequence[str], params_list: Sequence[SearchParameters],
                                      weights_list: Sequence[Weights], with_records: bool = False, packed: bool = True,
                                      chunk: Optional[int] = None):
        """anx_evaluate_sweep_weights: evaluate_sweep_arrays for sets that also differ in the score weights -- set s is
        (params_list[s], weights_list[s]) and its summary is what evaluate_arrays gives on a model created with weights_list[s].
        One batch run per distinct (max_anagram_distance, max_edit_distance, stop_criterion) serves every set; the model's own
        weights play no part.  Plain models only (no variant list, no confusable list).  Returns the summaries (SUMMARY_DTYPE), or
        (summaries, records[P][n]) with with_records.  packed = False: the pointer form; chunk: the test hook (pointer form)."""
        import numpy as np
        n, P = len(inputs), len(params_list)
        if len(gold) != n:
            raise ValueError("evaluate_sweep_weights: inputs and gold differ in length")
        if len(weights_list) != P:
            raise ValueError("evaluate_sweep_weights: params_list and weights_list differ in length")
        dt = np.dtype(self.SUMMARY_DTYPE)
        sums = np.zeros(max(P, 1), dtype=dt)
        sptr = sums.ctypes.data_as(C.POINTER(L.GoldSummary))
        sets = (L.Params * max(P, 1))(*[p._c() for p in params_list])
        ws = (L.Weights * max(P, 1))(*[w._c() for w in weights_list])
        rec = np.zeros((max(P, 1), max(n, 1)), dtype=np.dtype(self.GOLD_DTYPE)) if with_records else None   # [P][n] set-major (n == 0: untouched)
        optr = rec.ctypes.data_as(C.POINTER(L.GoldEval)) if with_records else None
        if packed and chunk is None:
            ba, bg = _pack(inputs), _pack(gold)
            L.check(L.lib().anx_evaluate_sweep_weights_packed(self.h, ba, len(ba), bg, len(bg), n, sets, ws, P, sptr, optr))
        else:
            aa = (C.c_char_p * max(n, 1))(*[_b(t) for t in inputs])
            ag = (C.c_char_p * max(n, 1))(*[_b(t) for t in gold])
            if chunk is None:
                L.check(L.lib().anx_evaluate_sweep_weights(self.h, aa, ag, n, sets, ws, P, sptr, optr))
            else:
                L.check(L.lib().anx_debug_evaluate_sweep_weights_chunk(self.h, aa, ag, n, sets, ws, P, sptr, optr, int(chunk)))
        return (sums[:P], rec[:P, :n]) if with_records else sums[:P]

    def evaluate_sweep_weights(self, inputs: Sequence[str], gold: Sequence[str], params_list: Sequence[SearchParameters],
                               weights_list: Sequence[Weights]) -> List[dict]:
        """evaluate_sweep_weights_arrays as one dict per set (sweep_summary), the set's weights under "weights"."""
        sums = self.evaluate_sweep_weights_arrays(inputs, gold, params_list, weights_list)
        return [dict(self.sweep_summary(s), weights=w.to_dict()) for s, w in zip(sums, weights_list)]

    @staticmethod
    def weight_sweep_stats() -> dict:
        """anx_debug_weight_sweep_stats: running totals of the weight-sweep calls since process start."""
        keys = ("calls", "chunks", "groups", "sets", "pair_passes", "batch_runs", "rows_rescored", "bytes_down")
        out = (C.c_uint64 * len(keys))()
        L.check(L.lib().anx_debug_weight_sweep_stats(out, len(keys)))
        return {k: int(out[i]) for i, k in enumerate(keys)}

    # -- confusable sweep --------------------------------------------------------------------------------
    CONF_SWEEP_MAX_PATTERNS = 64

    def evaluate_sweep_confusables_arrays(self, inputs: Sequence[str], gold: Sequence[str], patterns: Sequence[str],
                                          params_list: Sequence[SearchParameters], weights_list: Sequence[Sequence[float]],
                                          early_list: Optional[Sequence[bool]] = None, with_records: bool = False, packed: bool = True,
                                          chunk: Optional[int] = None):
        """anx_evaluate_sweep_confusables: evaluate_sweep_arrays for candidate confusable patterns -- set s is (params_list[s],
        weights_list[s] = one weight per pattern, early_list[s]) and its summary is what evaluate_arrays gives on a model with the
        same alphabet, lexicons and score weights whose confusable list is patterns[j] with weight weights_list[s][j], with
        set_confusables_before_pruning() iff early_list[s] (None: every set is late).  A weight of exactly 1.0 switches a pattern
        off.  One batch run and one edit-script pass per distinct (max_anagram_distance, max_edit_distance, stop_criterion) serve
        every set.  Models without a variant list and without a confusable list of their own; at most 64 patterns, 256 sets.
        Returns the summaries (SUMMARY_DTYPE), or (summaries, records[P][n]) with with_records.  packed = False: the pointer form;
        chunk: the test hook (pointer form)."""
        import numpy as np
        n, P, J = len(inputs), len(params_list), len(patterns)
        if len(gold) != n:
            raise ValueError("evaluate_sweep_confusables: inputs and gold differ in length")
        if len(weights_list) != P:
            raise ValueError("evaluate_sweep_confusables: params_list and weights_list differ in length")
        if early_list is not None and len(early_list) != P:
            raise ValueError("evaluate_sweep_confusables: params_list and early_list differ in length")
        if any(len(w) != J for w in weights_list):
            raise ValueError("evaluate_sweep_confusables: every set needs one weight per pattern")
        sums = np.zeros(max(P, 1), dtype=np.dtype(self.SUMMARY_DTYPE))
        sptr = sums.ctypes.data_as(C.POINTER(L.GoldSummary))
        sets = (L.Params * max(P, 1))(*[p._c() for p in params_list])
        pats = (C.c_char_p * max(J, 1))(*[_b(t) for t in patterns])
        ws = np.ascontiguousarray(np.asarray([[float(x) for x in w] for w in weights_list], dtype=np.float64).reshape(P, J))
        wptr = ws.ctypes.data_as(C.POINTER(C.c_double)) if ws.size else (C.c_double * 1)(1.0)
        early = None if early_list is None else (C.c_uint8 * max(P, 1))(*[1 if e else 0 for e in early_list])
        rec = np.zeros((max(P, 1), max(n, 1)), dtype=np.dtype(self.GOLD_DTYPE)) if with_records else None   # [P][n] set-major (n == 0: untouched)
        optr = rec.ctypes.data_as(C.POINTER(L.GoldEval)) if with_records else None
        if packed and chunk is None:
            ba, bg = _pack(inputs), _pack(gold)
            L.check(L.lib().anx_evaluate_sweep_confusables_packed(self.h, ba, len(ba), bg, len(bg), n, pats, J, sets, wptr, early, P, sptr, optr))
        else:
            aa = (C.c_char_p * max(n, 1))(*[_b(t) for t in inputs])
            ag = (C.c_char_p * max(n, 1))(*[_b(t) for t in gold])
            if chunk is None:
                L.check(L.lib().anx_evaluate_sweep_confusables(self.h, aa, ag, n, pats, J, sets, wptr, early, P, sptr, optr))
            else:
                L.check(L.lib().anx_debug_evaluate_sweep_confusables_chunk(self.h, aa, ag, n, pats, J, sets, wptr, early, P, sptr, optr, int(chunk)))
        return (sums[:P], rec[:P, :n]) if with_records else sums[:P]

    def evaluate_sweep_confusables(self, inputs: Sequence[str], gold: Sequence[str], patterns: Sequence[str],
                                   params_list: Sequence[SearchParameters], weights_list: Sequence[Sequence[float]],
                                   early_list: Optional[Sequence[bool]] = None, records: bool = False):
        """evaluate_sweep_confusables_arrays as one dict per set (sweep_summary), the set's weights under "confusable_weights" (pattern ->
        weight, the patterns at 1.0 left out) and its mode under "early".  records: returns (dicts, records[P][n])."""
        got = self.evaluate_sweep_confusables_arrays(inputs, gold, patterns, params_list, weights_list, early_list, with_records=records)
        sums = got[0] if records else got
        out = [dict(self.sweep_summary(s), confusable_weights={p: float(x) for p, x in zip(patterns, w) if float(x) != 1.0},
                    early=bool(early_list[i]) if early_list is not None else False)
               for i, (s, w) in enumerate(zip(sums, weights_list))]
        return (out, got[1]) if records else out

    def sweep_conf_masks(self, inputs: Sequence[str], patterns: Sequence[str], params: SearchParameters):
        """anx_debug_sweep_conf_masks (test hook): the base rows of `inputs` under params' k / d / stop criterion as three numpy arrays
        (input index, vocabulary id, mask): bit j of the mask = patterns[j] is found in the edit script of (input, vocabulary item)."""
        import numpy as np
        n, J = len(inputs), len(patterns)
        aa = (C.c_char_p * max(n, 1))(*[_b(t) for t in inputs])
        pats = (C.c_char_p * max(J, 1))(*[_b(t) for t in patterns])
        pp, pv, pm, rows = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)(), C.c_size_t(0)
        cp = params._c()
        L.check(L.lib().anx_debug_sweep_conf_masks(self.h, aa, n, pats, J, C.byref(cp), C.byref(pp), C.byref(pv), C.byref(pm), C.byref(rows)))
        try:
            r = rows.value
            return (np.array(pp[:r], dtype=np.uint32), np.array(pv[:r], dtype=np.uint32), np.array(pm[:r], dtype=np.uint64))
        finally:
            for p in (pp, pv, pm):
                L.lib().anx_string_free(C.cast(p, C.c_void_p))

    @staticmethod
    def conf_mask_text(patterns: Sequence[str], a: str, b: str) -> int:
        """anx_debug_conf_mask_text: the host body of the mask kernel -- bit j = patterns[j] is found in the edit script of (a -> b)."""
        J = len(patterns)
        pats = (C.c_char_p * max(J, 1))(*[_b(t) for t in patterns])
        out = C.c_uint64(0)
        L.check(L.lib().anx_debug_conf_mask_text(pats, J, _b(a), _b(b), C.byref(out)))
        return int(out.value)

    @staticmethod
    def conf_sweep_stats() -> dict:
        """anx_debug_conf_sweep_stats: running totals of the confusable-sweep calls since process start."""
        keys = ("calls", "chunks", "groups", "sets", "pair_passes", "batch_runs", "base_rows", "rows_listed", "rows_patched", "rows_host_mode",
                "bytes_down")
        out = (C.c_uint64 * len(keys))()
        L.check(L.lib().anx_debug_conf_sweep_stats(out, len(keys)))
        return {k: int(out[i]) for i, k in enumerate(keys)}

    # -- confusable fit ----------------------------------------------------------------------------------
    FIT_COUNTS_DTYPE = [("at1", "<u8"), ("ranked", "<u8"), ("rr_fixed", "<u8")]
    FIT_ROUND_DTYPE = [("pattern", "<u4"), ("grid_index", "<u4"), ("weight", "<f8"), ("counts", FIT_COUNTS_DTYPE)]
    FIT_RESULT_DTYPE = [("n_rounds", "<u4"), ("n_trial_rounds", "<u4"), ("stop", "<u4"), ("_pad", "<u4"), ("start", FIT_COUNTS_DTYPE),
                        ("final", FIT_COUNTS_DTYPE)]

    @staticmethod
    def fit_min_gain(objective: str, min_gain) -> int:
        """min_gain in the units of the objective's first key component: pairs for "acc1", reciprocal rank as 32.32 fixed point for "mrr"."""
        if objective not in L.FIT_OBJECTIVES:
            raise ValueError("fit_confusables: objective is 'acc1' or 'mrr'")
        if not (float(min_gain) >= 0.0) or float(min_gain) == float("inf"):
            raise ValueError("fit_confusables: min_gain is a number >= 0")
        if objective == "mrr":
            return int(round(float(min_gain) * 4294967296.0))
        if int(min_gain) != min_gain:
            raise ValueError("fit_confusables: for objective 'acc1' min_gain counts pairs: an integer")
        return int(min_gain)

    def fit_confusables_arrays(self, inputs: Sequence[str], gold: Sequence[str], patterns: Sequence[str], params: SearchParameters,
                               grid: Sequence[float], start: Optional[Sequence[float]] = None, objective: str = "acc1", max_rounds: int = 16,
                               min_gain=1, with_trials: bool = False, packed: bool = True, chunk: Optional[int] = None):
        """anx_fit_confusable_weights: a greedy coordinate ascent over the weights of the candidate patterns (late mode), on the
        device.  A round tries every (pattern, grid weight) that differs from the current weights; the best trial by (at1, rr_fixed)
        -- "mrr": (rr_fixed, at1) -- is accepted when it improves the key and gains at least min_gain in its first component
        (pairs; "mrr": reciprocal rank, a float); the fit ends when none is accepted (stop 0) or after max_rounds accepted rounds
        (stop 1).  Every count equals what evaluate_sweep_confusables_arrays gives for the same weights.  Returns (weights[J] f64,
        rounds (FIT_ROUND_DTYPE, the accepted ones), result (FIT_RESULT_DTYPE, one element)[, trials[n_trial_rounds][J][G]
        (FIT_COUNTS_DTYPE)]).  packed = False: the pointer form; chunk: the test hook (pointer form)."""
        import numpy as np
        n, J, G = len(inputs), len(patterns), len(grid)
        if len(gold) != n:
            raise ValueError("fit_confusables: inputs and gold differ in length")
        if start is not None and len(start) != J:
            raise ValueError("fit_confusables: start needs one weight per pattern")
        gain = self.fit_min_gain(objective, min_gain)
        max_rounds = int(max_rounds)
        room = min(max(max_rounds, 1), L.FIT_MAX_ROUNDS)   # (a max_rounds outside 1 .. 256 is the library's to refuse)
        ga = np.ascontiguousarray(np.asarray([float(x) for x in grid], dtype=np.float64))
        sa = None if start is None else np.ascontiguousarray(np.asarray([float(x) for x in start], dtype=np.float64))
        dp = C.POINTER(C.c_double)
        fp = L.FitParams(ga.ctypes.data_as(dp) if G else (C.c_double * 1)(1.0), G, 0, sa.ctypes.data_as(dp) if sa is not None and J else None,
                         L.FIT_OBJECTIVES[objective], max_rounds & 0xFFFFFFFF, gain)
        weights = np.zeros(max(J, 1), dtype=np.float64)
        rounds = np.zeros(room, dtype=np.dtype(self.FIT_ROUND_DTYPE))
        result = np.zeros(1, dtype=np.dtype(self.FIT_RESULT_DTYPE))
        trials = np.zeros((room, max(J, 1), max(G, 1)), dtype=np.dtype(self.FIT_COUNTS_DTYPE)) if with_trials else None
        assert rounds.dtype.itemsize == C.sizeof(L.FitRound) and result.dtype.itemsize == C.sizeof(L.FitResult)
        tail = (C.byref(fp), weights.ctypes.data_as(dp), rounds.ctypes.data_as(C.POINTER(L.FitRound)),
                trials.ctypes.data_as(C.POINTER(L.FitCounts)) if with_trials else None, result.ctypes.data_as(C.POINTER(L.FitResult)))
        pats = (C.c_char_p * max(J, 1))(*[_b(t) for t in patterns])
        cp = params._c()
        if packed and chunk is None:
            ba, bg = _pack(inputs), _pack(gold)
            L.check(L.lib().anx_fit_confusable_weights_packed(self.h, ba, len(ba), bg, len(bg), n, pats, J, C.byref(cp), *tail))
        else:
            aa = (C.c_char_p * max(n, 1))(*[_b(t) for t in inputs])
            ag = (C.c_char_p * max(n, 1))(*[_b(t) for t in gold])
            if chunk is None:
                L.check(L.lib().anx_fit_confusable_weights(self.h, aa, ag, n, pats, J, C.byref(cp), *tail))
            else:
                L.check(L.lib().anx_debug_fit_confusable_weights_chunk(self.h, aa, ag, n, pats, J, C.byref(cp), *tail, int(chunk)))
        res = (weights[:J], rounds[:int(result[0]["n_rounds"])], result)
        return res + (trials[:int(result[0]["n_trial_rounds"]), :J, :G],) if with_trials else res

    @staticmethod
    def fit_counts_summary(c, n: int) -> dict:
        """An anx_fit_counts as a dict, accuracy_at_1, ranked_share and mrr derived as sweep_summary derives them."""
        at1, ranked, rr = int(c["at1"]), int(c["ranked"]), int(c["rr_fixed"])
        return {"at1": at1, "ranked": ranked, "rr_fixed": rr, "accuracy_at_1": at1 / n if n else 0.0, "ranked_share": ranked / n if n else 0.0,
                "mrr": rr / 4294967296.0 / n if n else 0.0}

    def fit_confusables(self, inputs: Sequence[str], gold: Sequence[str], patterns: Sequence[str], params: SearchParameters,
                        grid: Sequence[float], start: Optional[Sequence[float]] = None, objective: str = "acc1", max_rounds: int = 16,
                        min_gain=1) -> dict:
        """fit_confusables_arrays as a dict: "weights" (pattern -> weight, the patterns at 1.0 left out), "rounds" (one dict per
        accepted round: pattern, grid_index, weight and the counts after it), "start" and "final" (fit_counts_summary), "stop"
        ("converged": no trial was accepted; "max_rounds"), "n_trial_rounds"."""
        n = len(inputs)
        weights, rounds, result = self.fit_confusables_arrays(inputs, gold, patterns, params, grid, start, objective, max_rounds, min_gain)
        r = result[0]
        return {"weights": {p: float(w) for p, w in zip(patterns, weights) if float(w) != 1.0},
                "rounds": [dict(self.fit_counts_summary(x["counts"], n), pattern=patterns[int(x["pattern"])], grid_index=int(x["grid_index"]),
                                weight=float(x["weight"])) for x in rounds],
                "start": self.fit_counts_summary(r["start"], n), "final": self.fit_counts_summary(r["final"], n),
                "stop": "max_rounds" if int(r["stop"]) else "converged", "n_trial_rounds": int(r["n_trial_rounds"])}

    @staticmethod
    def fit_select(trials, cur: Sequence[float], grid: Sequence[float], cur_counts, objective: str = "acc1", min_gain: int = 1):
        """anx_debug_fit_select (host only): the selection of one round.  trials[J][G] and cur_counts are (at1, ranked, rr_fixed)
        triples; min_gain in the key's own units.  Returns (pattern, grid_index), (-1, -1) when no trial is accepted."""
        J, G = len(cur), len(grid)
        flat = [t for row in trials for t in row]
        if len(trials) != J or len(flat) != J * G:
            raise ValueError("fit_select: trials is [patterns][grid]")
        tt = (L.FitCounts * max(J * G, 1))(*[L.FitCounts(*[int(x) for x in t]) for t in flat])
        cc = L.FitCounts(*[int(x) for x in cur_counts])
        pj, pg = C.c_int32(0), C.c_int32(0)
        L.check(L.lib().anx_debug_fit_select(tt, (C.c_double * max(J, 1))(*[float(x) for x in cur]), J, (C.c_double * max(G, 1))(*[float(x) for x in grid]), G,
                                             C.byref(cc), L.FIT_OBJECTIVES[objective], int(min_gain), C.byref(pj), C.byref(pg)))
        return int(pj.value), int(pg.value)

    @staticmethod
    def fit_stats() -> dict:
        """anx_debug_fit_stats: running totals of the fit calls since process start."""
        keys = ("calls", "chunks", "rounds", "trial_launches", "state_pairs", "state_slots", "bytes_down")
        out = (C.c_uint64 * len(keys))()
        L.check(L.lib().anx_debug_fit_stats(out, len(keys)))
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def query_output(self, inputs: Sequence[str], params: SearchParameters, json: bool = False,
                     output_lexmatch: bool = False, first_seqnr: int = 1) -> str:
        """One device batch + the text `analiticcl query` prints for it (anx_format_query_output: the TSV lines or JSON
        items of src/bin/analiticcl.rs:21-187, formatted natively)."""
        n = len(inputs)
        arr = (C.c_char_p * max(n, 1))(*[_b(t) for t in inputs])
        cp = params._c()
        rows = C.POINTER(L.Result)()
        offs = C.POINTER(C.c_size_t)()
        L.check(L.lib().anx_find_variants_batch(self.h, arr, n, C.byref(cp), C.byref(rows), C.byref(offs)))
        try:
            buf, ln = C.c_void_p(), C.c_size_t(0)
            L.check(L.lib().anx_format_query_output(self.h, arr, n, rows, offs, float(params.freq_weight), int(bool(json)),
                                                    int(bool(output_lexmatch)), first_seqnr, C.byref(buf), C.byref(ln)))
            try:
                return C.string_at(buf, ln.value).decode("utf-8")
            finally:
                L.lib().anx_string_free(buf)
        finally:
            L.lib().anx_results_free(rows, offs)

    def _to_dict(self, vid: int, dist: float, freq: float, freq_weight: float, via: Optional[int] = None) -> Dict:
        # variantresult_to_dict, bindings/python/src/lib.rs:554-588
        fw = float(freq_weight)
        score = dist if fw == 0.0 else (dist + fw * freq) / (1.0 + fw)
        cache = self.__dict__.setdefault("_vocab_cache", {})  # vocabulary items do not change after build()
        hit = cache.get(vid)
        if hit is None:
            lexindex = L.lib().anx_model_vocab_lexindex(self.h, vid)
            hit = cache[vid] = (self.vocab_text(vid), [name for i, name in enumerate(self.lexicons) if lexindex & (1 << i)])
        d = {"text": hit[0], "score": score, "dist_score": dist, "freq_score": freq}
        if via is not None:
            d["via"] = self.vocab_text(via)
        d["lexicons"] = list(hit[1])
        return d

    def find_variants(self, input: str, params: SearchParameters) -> List[dict]:
        res = self.find_variants_ids([input], params, with_via=True)[0]
        return [self._to_dict(v, d, f, params.freq_weight, via) for v, d, f, via in res]

    def find_variants_par(self, input: List[str], params: SearchParameters) -> List[dict]:
        res = self.find_variants_ids(input, params, with_via=True)
        return [{"input": t, "variants": [self._to_dict(v, d, f, params.freq_weight, via) for v, d, f, via in r]}
                for t, r in zip(input, res)]

    EXPLAIN_KEYS = ("ld", "lcs", "prefixlen", "suffixlen", "samecase", "anagram_distance", "len_input", "len_entry", "unweighted_score")

    def explain_variants(self, input: List[str], params: SearchParameters) -> List[dict]:
        """find_variants_par with the reason for every score: each variant dict also has ld, lcs, prefixlen, suffixlen, samecase,
        anagram_distance, len_input, len_entry (symbols), unweighted_score (the distance score of the input and the scored entry
        without confusable weight and variant score) and, when the row has a `via`, scored: the text of the entry that was scored.
        Always the staged batch path (the small call keeps no resident batch): Batch.run + anx_batch_fetch + Batch.fetch_measures."""
        b = Batch(self, input, params)
        try:
            b.run()
            rows = C.POINTER(L.Result)()
            offs = C.POINTER(C.c_size_t)()
            L.check(L.lib().anx_batch_fetch(b.h, C.byref(rows), C.byref(offs)))
            try:
                off = _offsets(offs, b.n)
                v, d, f, via = _result_columns(rows, off[-1])
            finally:
                L.lib().anx_results_free(rows, offs)
            moff, m = b.fetch_measures()
            if moff.tolist() != off:
                raise L.AnxError(L.ANX_EINVAL, "explain_variants: the measures do not describe the fetched rows")
            cols = {k: m[k].tolist() for k, _t in Batch.MEASURES_DTYPE}
        finally:
            b.free()
        out = []
        for i, t in enumerate(input):
            vs = []
            for r in range(off[i], off[i + 1]):
                has_via = via[r] != L.ANX_NO_VIA
                e = self._to_dict(v[r], d[r], f[r], params.freq_weight, via[r] if has_via else None)
                for k in ("ld", "lcs", "prefixlen", "suffixlen", "anagram_distance", "len_input", "len_entry"):
                    e[k] = cols[k][r]
                e["samecase"] = bool(cols["flags"][r] & 1)
                e["unweighted_score"] = cols["score"][r]
                if has_via:
                    e["scored"] = e["via"]
                vs.append(e)
            out.append({"input": t, "variants": vs})
        return out

    # -- search mode: the caller of the hot path ---------------------------
    def find_all_matches_ids(self, texts: Sequence[str], params: SearchParameters) -> List[List[dict]]:
        """anx_find_all_matches_batch over many texts: every segment of one n-gram order, over all texts, is one
        device batch. Per text: [{begin, end, n, selected, variants: [(vocab_id, dist, freq, via|None)]}]."""
        n = len(texts)
        enc = [_b(t) for t in texts]
        arr = (C.c_char_p * max(n, 1))(*enc)
        sp = params._c_search()
        ms, offs, rows = C.POINTER(L.Match)(), C.POINTER(C.c_size_t)(), C.POINTER(L.Result)()
        tags = C.POINTER(L.MatchTag)()
        nrows = C.c_size_t(0)
        L.check(L.lib().anx_find_all_matches_batch(self.h, arr, n, C.byref(sp), C.byref(ms), C.byref(offs),
                                                   C.byref(rows), C.byref(nrows), C.byref(tags)))
        try:
            import numpy as np
            off = _offsets(offs, n)
            v, d, f, via = _result_columns(rows, nrows.value)
            via = [None if x == L.ANX_NO_VIA else x for x in via]
            out = [[] for _ in range(n)]
            if off[-1]:
                mdt = np.dtype([("begin", "<u8"), ("end", "<u8"), ("n", "<u4"), ("selected", "<i4"), ("vb", "<u8"), ("ve", "<u8"),
                                ("tb", "<u4"), ("te", "<u4")])
                ma = np.frombuffer((C.c_char * (off[-1] * mdt.itemsize)).from_address(C.addressof(ms.contents)), dtype=mdt)
                cols = [ma[k].tolist() for k in ("begin", "end", "n", "selected", "vb", "ve", "tb", "te")]
                ntags = max(cols[7]) if cols[7] else 0
                tg = sq = []
                if ntags:
                    tdt = np.dtype([("tag", "<u2"), ("seqnr", "u1"), ("pad", "u1")])
                    ta = np.frombuffer((C.c_char * (ntags * tdt.itemsize)).from_address(C.addressof(tags.contents)), dtype=tdt)
                    tg, sq = ta["tag"].tolist(), ta["seqnr"].tolist()
                for i in range(n):
                    cur = out[i]
                    for j in range(off[i], off[i + 1]):
                        vb, ve, tb, te = cols[4][j], cols[5][j], cols[6][j], cols[7][j]
                        cur.append({"begin": cols[0][j], "end": cols[1][j], "n": cols[2][j],
                                    "selected": None if cols[3][j] < 0 else cols[3][j],
                                    "variants": list(zip(v[vb:ve], d[vb:ve], f[vb:ve], via[vb:ve])),
                                    "tag": tg[tb:te], "seqnr": sq[tb:te]})
            return out
        finally:
            L.lib().anx_matches_free(ms, offs, rows, tags)

    def find_all_matches_arrays(self, texts: Sequence[str], params: SearchParameters):
        """Bulk form of find_all_matches_ids: numpy copies of what anx_find_all_matches_batch returns, no per-match Python
        objects.  -> (offs[n+1], matches (structured: begin, end, n, selected, vb, ve, tb, te), rows (structured:
        vocab_id, dist, freq, via)); the matches of text i are matches[offs[i]:offs[i+1]], the variants of a match
        rows[vb:ve] (selected = index into them, -1 = none)."""
        import numpy as np
        n = len(texts)
        arr = (C.c_char_p * max(n, 1))(*[_b(t) for t in texts])
        sp = params._c_search()
        ms, offs, rows = C.POINTER(L.Match)(), C.POINTER(C.c_size_t)(), C.POINTER(L.Result)()
        nrows = C.c_size_t(0)
        L.check(L.lib().anx_find_all_matches_batch(self.h, arr, n, C.byref(sp), C.byref(ms), C.byref(offs),
                                                   C.byref(rows), C.byref(nrows), None))
        try:
            off = np.ctypeslib.as_array(offs, shape=(n + 1,)).astype(np.int64)
            mdt = np.dtype([("begin", "<u8"), ("end", "<u8"), ("n", "<u4"), ("selected", "<i4"), ("vb", "<u8"), ("ve", "<u8"),
                            ("tb", "<u4"), ("te", "<u4")])
            rdt = np.dtype([("vocab_id", "<u8"), ("dist", "<f8"), ("freq", "<f8"), ("via", "<u8")])
            nm = int(off[-1])
            ma = np.frombuffer((C.c_char * (nm * mdt.itemsize)).from_address(C.addressof(ms.contents)), dtype=mdt).copy() \
                if nm else np.zeros(0, dtype=mdt)
            ra = np.frombuffer((C.c_char * (nrows.value * rdt.itemsize)).from_address(C.addressof(rows.contents)), dtype=rdt).copy() \
                if nrows.value else np.zeros(0, dtype=rdt)
            return off, ma, ra
        finally:
            L.lib().anx_matches_free(ms, offs, rows, None)

    def search_output(self, texts: Sequence[str], params: SearchParameters, json: bool = False,
                      output_lexmatch: bool = False, first_seqnr: int = 1):
        """find_all_matches over the texts + the text `analiticcl search` prints for the matches
        (anx_format_search_output) -> (text, number of matches)."""
        if params.unicodeoffsets:
            raise ValueError("search_output needs byte offsets (unicodeoffsets=False)")
        n = len(texts)
        arr = (C.c_char_p * max(n, 1))(*[_b(t) for t in texts])
        sp = params._c_search()
        ms, offs, rows = C.POINTER(L.Match)(), C.POINTER(C.c_size_t)(), C.POINTER(L.Result)()
        tags = C.POINTER(L.MatchTag)()
        nrows = C.c_size_t(0)
        L.check(L.lib().anx_find_all_matches_batch(self.h, arr, n, C.byref(sp), C.byref(ms), C.byref(offs),
                                                   C.byref(rows), C.byref(nrows), C.byref(tags)))
        try:
            buf, ln = C.c_void_p(), C.c_size_t(0)
            L.check(L.lib().anx_format_search_output(self.h, arr, n, ms, offs, rows, tags, float(params.freq_weight),
                                                     int(bool(json)), int(bool(output_lexmatch)), first_seqnr,
                                                     C.byref(buf), C.byref(ln)))
            try:
                return C.string_at(buf, ln.value).decode("utf-8"), int(offs[n])
            finally:
                L.lib().anx_string_free(buf)
        finally:
            L.lib().anx_matches_free(ms, offs, rows, tags)

    def find_all_matches(self, text: str, params: SearchParameters) -> List[dict]:
        """find_all_matches of the pyo3 binding (bindings/python/src/lib.rs:752-805): the selected variant first."""
        res = self.find_all_matches_ids([text], params)[0]
        raw = _b(text)
        out = []
        for m in res:
            inp = text[m["begin"]:m["end"]] if params.unicodeoffsets else raw[m["begin"]:m["end"]].decode("utf-8")
            order = list(range(len(m["variants"])))
            if m["selected"] is not None and m["selected"] < len(order):
                order.remove(m["selected"])
                order.insert(0, m["selected"])
            item = {"input": inp, "offset": {"begin": m["begin"], "end": m["end"]}}
            if m["tag"]:  # bindings/python/src/lib.rs:768-782
                item["tag"] = [self.tag_name(t) for t in m["tag"]]
                item["seqnr"] = list(m["seqnr"])
            item["variants"] = [self._to_dict(*m["variants"][k][:3], params.freq_weight, m["variants"][k][3])
                                for k in order]
            out.append(item)
        return out

    # -- context rules of search mode (src/lib.rs:570-765; bindings/python/src/lib.rs:630-700) -------------
    # -- learn mode (src/lib.rs:1029-1139) ----------------------------------------------------------------------------------------
    def learn_variants(self, inputs: Sequence[str], params: SearchParameters, strict: bool = True, auto_build: bool = True) -> int:
        """learn_variants: query every input against the model as it is now, fold the ranked rows into the model (new input strings
        become TRANSPARENT entries that build() does not index; ReferenceFor links on the results, first mention wins) and return the
        number of rows whose result was not the input itself.  strict=False: each input is a text, its rows are the selected variants
        of find_all_matches paired with the matched text.  auto_build: build() and the upload to the model's devices again."""
        self.__dict__.pop("_vocab_cache", None)
        n = len(inputs)
        arr = (C.c_char_p * max(n, 1))(*[_b(t) for t in inputs])
        count = C.c_uint64(0)
        if strict:
            L.check(L.lib().anx_learn_variants(self.h, arr, n, C.byref(params._c()), int(bool(auto_build)), C.byref(count)))
        else:
            L.check(L.lib().anx_learn_variants_search(self.h, arr, n, C.byref(params._c_search()), int(bool(auto_build)),
                                                      C.byref(count)))
        return count.value

    def learn_apply_rows(self, inputs: Sequence[str], rows: Sequence[Sequence[tuple]]) -> int:
        """The fold of learn_variants over caller-provided ranked rows (per input: [(vocab_id, dist_score, ...)]), on the host; no
        build.  -> the count learn_variants would return."""
        return self._learn_rows(inputs, rows, None)

    def learn_fold_rows_device(self, inputs: Sequence[str], rows: Sequence[Sequence[tuple]], n_sections: int = 1,
                               by_index: bool = False) -> int:
        """The same fold through learn.hip on replica 0's device (anx_debug_learn_fold_rows, a test hook): the rows are packed into
        n_sections compact export sections, contiguous input ranges or (by_index) index-listed round-robin ones; no build."""
        return self._learn_rows(inputs, rows, (int(n_sections), int(bool(by_index))))

    def _learn_rows(self, inputs, rows, device_sections) -> int:
        self.__dict__.pop("_vocab_cache", None)
        n = len(inputs)
        if len(rows) != n:
            raise ValueError("one list of rows per input")
        arr = (C.c_char_p * max(n, 1))(*[_b(t) for t in inputs])
        off = [0]
        for r in rows:
            off.append(off[-1] + len(r))
        res = (L.Result * max(off[-1], 1))()
        k = 0
        for r in rows:
            for row in r:
                res[k].vocab_id, res[k].dist_score = int(row[0]), float(row[1])
                res[k].freq_score = float(row[2]) if len(row) > 2 else 0.0
                res[k].via = L.ANX_NO_VIA
                k += 1
        offs = (C.c_size_t * (n + 1))(*off)
        count = C.c_uint64(0)
        if device_sections is None:
            L.check(L.lib().anx_learn_apply_rows(self.h, arr, n, res, offs, C.byref(count)))
        else:
            L.check(L.lib().anx_debug_learn_fold_rows(self.h, arr, n, res, offs, device_sections[0], device_sections[1], C.byref(count)))
        return count.value

    def variants(self, vocab_id: int) -> List[tuple]:
        """The item's variant references in order: [("ReferenceFor" | "VariantOf", vocab_id, score)]."""
        lib = L.lib()
        k = lib.anx_model_variants(self.h, vocab_id, None, None, None, 0)
        if k < 0:
            L.check(int(k))
        if k == 0:
            return []
        kinds, ids, scores = (C.c_uint8 * k)(), (C.c_uint64 * k)(), (C.c_double * k)()
        lib.anx_model_variants(self.h, vocab_id, kinds, ids, scores, k)
        return [("VariantOf" if kinds[i] else "ReferenceFor", ids[i], scores[i]) for i in range(k)]

    def vocab_size(self) -> int:
        return L.lib().anx_model_vocab_size(self.h)

    def vocab_frequency(self, vocab_id: int) -> int:
        return L.lib().anx_model_vocab_frequency(self.h, vocab_id)

    def vocab_lexindex(self, vocab_id: int) -> int:
        return L.lib().anx_model_vocab_lexindex(self.h, vocab_id)

    def vocabtype(self, vocab_id: int) -> int:
        """VocabType bits of the item: 1 INDEXED, 2 LM, 4 TRANSPARENT (include/anx.h ANX_VOCAB_*)."""
        return L.lib().anx_model_vocab_type(self.h, vocab_id)

    def variant_list_output(self, json: bool = False) -> str:
        """The weighted variant list `analiticcl learn` prints (ReferenceFor links of every item in vocabulary order), as TSV or as
        the reference's JSON (trailing commas included)."""
        buf = C.c_void_p()
        L.check(L.lib().anx_format_variant_list(self.h, int(bool(json)), C.byref(buf)))
        try:
            return C.string_at(buf).decode("utf-8")
        finally:
            L.lib().anx_string_free(buf)

    @staticmethod
    def learn_stats() -> dict:
        """anx_debug_learn_stats: folds that ran on the device / on the host, rows folded, ReferenceFor links added (process totals)."""
        out = (C.c_uint64 * 4)()
        L.check(L.lib().anx_debug_learn_stats(out))
        return {"device_folds": out[0], "host_folds": out[1], "rows": out[2], "links": out[3]}

    @staticmethod
    def learn_times() -> dict:
        """The last learn call's phases in ms (anx_debug_learn_times)."""
        out = (C.c_double * 6)()
        L.check(L.lib().anx_debug_learn_times(out))
        return dict(zip(("batch", "device_fold", "host_fold", "host_apply", "build", "upload"), list(out)))

    @staticmethod
    def search_lattice_stats() -> dict:
        """anx_debug_search_lattice_stats: lattices decoded on the device / by the host decoder / on the device with context rules
        scored, and parts of search calls that completed as one pass (process totals)."""
        out = (C.c_uint64 * 4)()
        L.check(L.lib().anx_debug_search_lattice_stats(out))
        return {"device": out[0], "host": out[1], "device_rules": out[2], "onepass_parts": out[3]}

    @staticmethod
    def portable_log(x):
        """Test hook (anx_debug_portable_log): the host build of the library's logarithm over a float64 array."""
        import numpy as np
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        L.check(L.lib().anx_debug_portable_log(x.ctypes.data, x.size, out.ctypes.data))
        return out

    def debug_lattice_decode(self, params: SearchParameters, lattices: Sequence[dict], first: int = 0, count: Optional[int] = None,
                             budget_nodes: int = 0, pools: bool = True) -> dict:
        """Test hook (anx_debug_lattice_decode): the device lattice decoder alone on the caller's lattices, through the product's
        lattice_decode.  A lattice is a dict of nstates, in_off [nstates + 2], arcs [(cost, src, sym)] (sym 0xFFFFFFFF = epsilon),
        syms [(vocab_id, boundary)], btok_off [nstates], btok, best_cost_init.  Returns out_n / out_syms / out_cover (per lattice
        of the view; out_cover stays the fill without rules) and, with pools, the device pools of the sub-range's stretches over a 0xFF
        fill: per stretch cnts [states], nodes [states, K, 3], lm [states, K, 3], marks [states, MK], ctxval [K], launch, width,
        lds; plus lds_limit and n_launches.  A refusal raises AnxError before anything is launched."""
        import numpy as np
        n = len(lattices)
        count = n - first if count is None else count
        K = max(1, int(params.max_seq))
        ns = np.array([int(l["nstates"]) for l in lattices], dtype=np.uint32)
        for l in lattices:  # the lengths the C side cannot see
            if len(l["in_off"]) != int(l["nstates"]) + 2 or len(l["btok_off"]) != max(int(l["nstates"]), 1):
                raise ValueError("in_off needs nstates + 2 entries and btok_off nstates")
            if int(l["in_off"][-1]) != len(l["arcs"]) or int(l["btok_off"][-1]) != len(l["btok"]):
                raise ValueError("the last offset is not the length of its array")
        cat = lambda key, dt: np.ascontiguousarray(np.concatenate([np.asarray(l[key], dtype=dt).reshape(-1) for l in lattices] + [np.zeros(0, dt)]))
        in_off, btok_off, btok = cat("in_off", np.uint32), cat("btok_off", np.uint32), cat("btok", np.int32)
        arcs = np.zeros((sum(len(l["arcs"]) for l in lattices), 3), dtype=np.uint32)
        syms = np.zeros((sum(len(l["syms"]) for l in lattices), 2), dtype=np.uint32)
        ai = si = 0
        for l in lattices:
            if len(l["arcs"]):
                a = l["arcs"]
                arcs[ai:ai + len(a), 0] = np.array([x[0] for x in a], dtype=np.float32).view(np.uint32)
                arcs[ai:ai + len(a), 1] = [x[1] for x in a]
                arcs[ai:ai + len(a), 2] = [x[2] for x in a]
                ai += len(a)
            if len(l["syms"]):
                syms[si:si + len(l["syms"])] = np.asarray(l["syms"], dtype=np.uint32).reshape(-1, 2)
                si += len(l["syms"])
        nsyms = np.array([len(l["syms"]) for l in lattices], dtype=np.uint32)
        bci = np.array([l["best_cost_init"] for l in lattices], dtype=np.float32)
        out_total = int(ns.sum())
        out_n = np.zeros(n, dtype=np.uint32)
        out_syms = np.zeros(max(out_total, 1), dtype=np.uint32)
        out_cover = np.zeros(max(out_total, 1), dtype=np.uint32)  # (stays the fill for a model without rules)
        dbg = L.LatticeDebug()
        dbg.budget_nodes = int(budget_nodes)
        sub = ns[first:first + count].astype(np.int64) + 1 if 0 <= first <= n and 0 <= count <= n - first else np.zeros(0, np.int64)
        states = int(sub.sum())
        MK = (K + 3) & ~3
        arrs = {}
        if pools and states * K <= 1 << 24:
            arrs = dict(launch_of=np.full(max(len(sub), 1), 0xFFFFFFFF, np.uint32), width_of=np.full(max(len(sub), 1), 0xFFFFFFFF, np.uint32),
                        lds_of=np.full(max(len(sub), 1), 0xFFFFFFFF, np.uint32), nodes=np.full((max(states, 1), K, 3), 0xFFFFFFFF, np.uint32),
                        lm=np.full((max(states, 1), K, 3), 0xFFFFFFFF, np.uint32), marks=np.full((max(states, 1), MK), 0xFF, np.uint8),
                        cnts=np.full(max(states, 1), 0xFFFF, np.uint16), ctxval=np.full((max(len(sub), 1), K), 0xFFFFFFFFFFFFFFFF, np.uint64))
            for k, v in arrs.items():
                setattr(dbg, k, v.ctypes.data)
        cs = params._c_search()
        L.check(L.lib().anx_debug_lattice_decode(self.h, C.byref(cs), n, ns.ctypes.data, in_off.ctypes.data, arcs.ctypes.data, nsyms.ctypes.data,
                                                 syms.ctypes.data, btok_off.ctypes.data, btok.ctypes.data, bci.ctypes.data, first, count,
                                                 out_n.ctypes.data, out_syms.ctypes.data, out_cover.ctypes.data,
                                                 C.byref(dbg)))
        o0 = np.concatenate([[0], np.cumsum(ns.astype(np.int64))])
        res = {"out_n": out_n, "out_syms": [out_syms[o0[i]:o0[i + 1]] for i in range(n)],
               "out_cover": [out_cover[o0[i]:o0[i + 1]] for i in range(n)],
               "lds_limit": int(dbg.lds_limit), "n_launches": int(dbg.n_launches), "stretches": []}
        if arrs:
            s0 = np.concatenate([[0], np.cumsum(sub)])
            for j in range(len(sub)):
                a, b = int(s0[j]), int(s0[j + 1])
                res["stretches"].append(dict(cnts=arrs["cnts"][a:b], nodes=arrs["nodes"][a:b], lm=arrs["lm"][a:b], marks=arrs["marks"][a:b],
                                             ctxval=arrs["ctxval"][j], launch=int(arrs["launch_of"][j]), width=int(arrs["width_of"][j]),
                                             lds=int(arrs["lds_of"][j])))
        return res

    def debug_scan_pairs(self, batch: Optional["Batch"] = None, inputs: Optional[Sequence[str]] = None, params: Optional[SearchParameters] = None,
                         region_shift: int = 12, chunk: int = 256, chunk_fused: int = 128, chunk_first: int = 32, fuse: bool = True,
                         twins: bool = True, drop_len: bool = True, want_exact: bool = False, count_pairs: bool = False, slots: int = 32) -> dict:
        """Test hook (anx_debug_scan_pairs): the scan stage alone.  With `batch`: the batch's own tiles through a run's three launches;
        with `inputs` and `params`: the small call's encoder (slots tile slots per query) and k_scan_small.  Returns the tiles as launched
        [tiles, 15], nadj / nbits / nsad, per query of the sorted order q_orig / kind / meta (len | k << 8 | d << 16) / qpairs, the whole
        pair list raw [64, slots per region, 2] (0xFEFEFEFE = never touched), rctr [64, 32] and guard (slots written behind the pair
        list).  A refusal raises AnxError before anything is launched."""
        import numpy as np
        o = L.ScanOpts(region_shift, chunk, chunk_fused, chunk_first, int(fuse), int(twins), int(drop_len), int(want_exact), int(count_pairs), slots)
        if batch is not None:
            n, arr, cp = batch.n, None, None
        else:
            n = len(inputs)
            arr = (C.c_char_p * max(n, 1))(*[_b(s) for s in inputs])
            cp = C.byref(params._c())
        if not 10 <= region_shift <= 25:
            raw = np.zeros((64, 1, 2), np.uint32)   # (refused below; the output is sized by the shift)
        else:
            raw = np.zeros((64, 1 << region_shift, 2), np.uint32)
        counts, query, rctr = np.zeros(6, np.uint32), np.zeros((4, max(n, 1)), np.uint32), np.zeros((64, 32), np.uint32)
        pt = C.POINTER(C.c_uint32)()
        L.check(L.lib().anx_debug_scan_pairs(self.h, batch.h if batch is not None else None, arr, n, cp, C.byref(o), counts.ctypes.data, C.byref(pt),
                                             query.ctypes.data, raw.ctypes.data, rctr.ctypes.data))
        nt, nq = int(counts[0]), int(counts[4])
        tiles = np.ctypeslib.as_array(pt, shape=(max(nt, 1), 15)).copy()[:nt]
        L.lib().anx_counts_free(pt)
        return dict(tiles=tiles, nadj=int(counts[1]), nbits=int(counts[2]), nsad=int(counts[3]), nq=nq, guard=int(counts[5]),
                    q_orig=query[0, :nq], kind=query[1, :nq], meta=query[2, :nq], qpairs=query[3, :nq], raw=raw, rctr=rctr)

    def contextrule_element_matches(self, rule: int, position: int, vocab_id: int, lexindex: int, flat: bool = False) -> bool:
        """Test hook (anx_debug_contextrule_match): element `position` of context rule `rule` on (vocab_id, lexindex), evaluated as
        the parsed pattern (flat=False) or as the flattened element the device decoder reads (flat=True)."""
        out = C.c_int(0)
        L.check(L.lib().anx_debug_contextrule_match(self.h, rule, position, vocab_id, lexindex, 1 if flat else 0, C.byref(out)))
        return bool(out.value)

    def add_contextrule(self, pattern: str, score: float, tag: Sequence[str] = (), tagoffset: Sequence[str] = ()):
        t = (C.c_char_p * max(1, len(tag)))(*[_b(x) for x in tag])
        o = (C.c_char_p * max(1, len(tagoffset)))(*[_b(x) for x in tagoffset])
        L.check(L.lib().anx_model_add_contextrule(self.h, _b(pattern), float(score), t, len(tag), o, len(tagoffset)))

    def read_contextrules(self, filename: str):
        L.check(L.lib().anx_model_read_contextrules(self.h, _b(filename)))

    @property
    def tags(self) -> List[str]:
        return [self.tag_name(i) for i in range(L.lib().anx_model_num_tags(self.h))]

    def tag_name(self, index: int) -> str:
        s = L.lib().anx_model_tag_name(self.h, index)
        if s is None:
            raise IndexError("tag %d" % index)
        return s.decode("utf-8")

    # -- confusables: host-side rescoring of the ranked lists ---------------
    def read_lm(self, filename: str):
        """Language-model n-gram counts: read_vocabulary with VocabType::LM (bindings/python/src/lib.rs:659-667)."""
        self.read_vocabulary(filename, VocabParams(vocabtype="LM"))

    def read_confusiblelist(self, filename: str):
        """The spelling the reference's Python API uses (analiticcl.pyi:283, bindings/python/src/lib.rs read_confusiblelist)."""
        self.read_confusablelist(filename)

    def read_confusablelist(self, filename: str):
        L.check(L.lib().anx_model_read_confusablelist(self.h, _b(filename)))

    def add_to_confusables(self, editscript: str, weight: float):
        L.check(L.lib().anx_model_add_to_confusables(self.h, _b(editscript), float(weight)))

    def compute_confusable_weight(self, input: str, vocab_id: int) -> float:
        """compute_confusable_weight (src/lib.rs:1733-1756): product of the weights of the confusable patterns found in the edit
        script input -> vocabulary item."""
        w = C.c_double(1.0)
        L.check(L.lib().anx_model_confusable_weight(self.h, _b(input), int(vocab_id), C.byref(w)))
        return w.value

    def set_confusables_before_pruning(self):
        L.lib().anx_model_set_confusables_before_pruning(self.h)
