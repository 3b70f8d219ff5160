"""Conditions on the inputs of tests/test_gpu_scan_door.py, checked without a GPU.

(a) The reference of tests/scan_cases.py -- the set the header of kernels_scan.hpp states, computed from count vectors -- equals the C
    oracle's n_pairs for every query of every case, and the twin's find_nearest_anahashes + index for every distinct (length, kind, k).
(b) band_bound_rejects never rejects a pair whose Damerau-Levenshtein distance is within d, on the cases' own pairs.
(c) The reference-side classes the GPU test relies on are populated.  (The tile-side classes are asserted by the GPU test itself, from
    the tiles the door returns.)"""
from collections import Counter

import numpy as np
import pytest

import scan_cases as S
from oracle import cwrap as O
from oracle import twin as T

ALL = S.BATCH_CASES + S.STOP_CASES + S.SMALL_CASES
_ORACLES = {}


def _oracle(m):
    if m.name not in _ORACLES:
        o = O.OracleModel(alphabet_text=m.alphabet_text())
        for w in m.texts:
            o.add(w)
        o.build()
        _ORACLES[m.name] = o
    return _ORACLES[m.name]


def test_every_case_is_listed():
    assert sorted(ALL) == sorted(S.cases()) and len(set(ALL)) == len(ALL)


@pytest.mark.parametrize("name", ALL)
def test_reference_counts_equal_the_c_oracle(name):
    c = S.case(name)
    o = _oracle(c.model)
    p = O.make_params(c.kth, c.dth, 10, 0.25, 2.0)
    seen = set()
    for q, r in zip(c.queries, c.ref):
        assert r is not None, q
        if q in seen:
            continue
        seen.add(q)
        _, _, npairs, _ = o.find_variants(q, p, want_pairs=True, cap=1 << 14)
        assert npairs == len(r.ents), (name, q, npairs, len(r.ents))


def test_stop_counts_equal_the_c_oracle():
    """StopAtExactMatch: the narrowed per-query count (the exact class alone where the lexicon has it) is the oracle's n_pairs"""
    c = S.case("five-stop")
    o = _oracle(c.model)
    p = O.make_params(c.kth, c.dth, 10, 0.25, 2.0, stop_at_exact_match=True)
    have = Counter()
    for q, r in zip(c.queries, c.ref):
        ex = S.expected(c.model, r, False, False, True)
        _, _, npairs, _ = o.find_variants(q, p, want_pairs=True, cap=1 << 14)
        assert npairs == ex.n_counted, (q, npairs, ex.n_counted)
        have["exact" if r.exact_cls >= 0 else "none"] += 1
        assert sum(1 for (_, f) in ex.written if f & 2) == (ex.n_counted if r.exact_cls >= 0 else 0)
    assert have["exact"] > 20 and have["none"] > 20


@pytest.mark.parametrize("name", ["lex-many", "five-k3d2", "five-k2d2", "five-k1d1", "five-k0d0", "five1-run", "wide"])
def test_reference_equals_the_twin(name):
    """one query of every distinct (length, kind, k) of the case: the same entries as find_nearest_anahashes + index[av][0]"""
    c = S.case(name)
    m = c.model
    done = set()
    for q, r in zip(c.queries, c.ref):
        key = (r.lq, r.kind, r.k)
        if key in done:
            continue
        done.add(key)
        near = m.twin.find_nearest_anahashes(T.anahash(q, m.alphabet), r.k)
        ents = sorted(v - 3 for av in near for v in m.twin.index[av][0])
        assert ents == r.ents.tolist(), (name, q, key)
    assert len(done) >= 4


def test_band_bound_never_rejects_a_pair_within_d():
    n = 0
    for name in ("five-k3d2", "five-k3d3", "five-k1d1", "lex-many", "five1-run"):
        c = S.case(name)
        m = c.model
        for r in {id(r): r for r in c.ref}.values():
            if not S.fuses(r, True):
                continue
            for e in r.ents.tolist():
                if abs(int(m.lens[e]) - r.lq) <= r.d and m.lens[e] <= 16 and S.band_rejects(m, r, e):
                    assert T.damerau_levenshtein(r.norm, m.norm[e], r.d) is None, (name, r.text, m.texts[e])
                    n += 1
    assert n > 1000


def _census():
    have = Counter()
    for name in ALL:
        c = S.case(name)
        m = c.model
        have["nq=%d" % len(c.queries)] += 1
        for r in {id(r): r for r in c.ref}.values():
            have["k=%d" % r.k] += 1
            have["kind=%d" % r.kind] += 1
            have["d<k" if r.d < r.k else "d=k" if r.d == r.k else "d>k"] += 1
            if r.lq <= 3 or r.lq in (16, 17):
                have["lq=%d" % r.lq] += 1
            ex = S.expected(m, r, True, True, False)
            if ex.n_lendrop:
                have["length-dropped"] += 1
            if ex.n_bandrej:
                have["band-rejected"] += 1
            if not r.ents.size:
                have["no pair"] += 1
            if r.kind and len(r.ents) > S.SCAN_PBUF:
                have["ring wraps"] += 1
            if r.kind and len(r.ents) > 2 * S.SCAN_HITS:
                have["hit list flushed twice"] += 1
            if r.kind == 0 and len(set(m.cls[r.ents].tolist())) > S.SCAN_HITS - 64:   # (a count-vector tile expands its list when a chunk of 64 could overflow it)
                have["count-vector list flushed"] += 1
            if r.kind == 0 and (r.lq + m.lens[np.abs(m.lens - r.lq) <= r.k] - 1 < r.k).any():   # (an entry inside the length window)
                have["thr from share"] += 1
            if S.fuses(r, True):
                lcs = m.lens[r.ents]
                ok = np.abs(lcs - r.lq) <= r.d
                if (ok & (lcs == 17)).any():
                    have["17-symbol entry in a fused tile"] += 1
                for lo, hi, nm in ((0, 8, "band ml<=8"), (9, 12, "band ml 9..12"), (13, 16, "band ml 13..16")):
                    ml = np.maximum(lcs[ok & (lcs <= 16)], r.lq)
                    if ((ml >= lo) & (ml <= hi)).any():
                        have[nm] += 1
            elif r.kind and r.lq > 16:
                have["bit-plane tile that does not fuse"] += 1
    return have


def test_reference_side_classes_are_populated():
    have = _census()
    need = ["nq=1", "nq=31", "nq=32", "nq=33", "nq=40", "nq=64", "nq=129", "nq=600", "k=0", "k=1", "k=2", "k=3", "kind=0", "kind=1", "kind=2", "kind=3", "kind=4",
            "d<k", "d=k", "lq=1", "lq=2", "lq=3", "lq=16", "lq=17", "length-dropped", "band-rejected", "no pair", "ring wraps", "hit list flushed twice",
            "count-vector list flushed", "thr from share", "17-symbol entry in a fused tile", "band ml<=8", "band ml 9..12", "band ml 13..16", "bit-plane tile that does not fuse"]
    missing = [k for k in need if not have[k]]
    assert not missing, (missing, dict(have))
    m = S.model("five")
    assert 255 in m.lens and 17 in m.lens
    assert int((S.model("five1").lens == 7).sum()) > S.SCAN_MASKW
