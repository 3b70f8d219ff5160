"""Models with variant lists for the GPU tests of the small call and of the compact records with `via`: the golden English lexicon plus
(a) a hand-made weighted variant list and (b) a list the product itself learned (learn_variants -> variant_list_output -> read_variants),
each with the C oracle holding the same files.  A lexicon only has variant lists when an INDEXED entry holds a VariantOf link, so
every builder asserts that the old fetch_compact() refuses the model."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import synth
from oracle import cwrap as O

# queries whose rows carry a `via` on model (a)
HAND_QUERIES = ["recieve", "seperate", "definately", "thier", "occurence", "neccessary", "recieves", "desperate", "qwertyx", "releive"]


def hand_made_lists(tmp_path, words):
    """-> [(path, transparent)].  List 1 (its variants are returned themselves): `recieve` has three references, `desperate` and
    `there` are indexed words of the lexicon that become variants, `qwertyx` has 150 references (more rows than a call of one input
    has room for).  List 2 is an error list (TRANSPARENT variants: only their references are returned)."""
    rng = random.Random(11)
    many = rng.sample([w for w in words if 5 <= len(w) <= 9 and w.isalpha()], 150)
    one = ["receive\trecieve\t0.9\treceeve\t0.8", "relieve\trecieve\t0.7\treleive\t0.9", "reprieve\trecieve\t0.6",
           "separate\tseperate\t1.0\tdesperate\t0.5", "their\tthere\t0.8\tthier\t0.9"]
    one += [f"{w}\tqwertyx\t{0.5 + 0.003 * i}" for i, w in enumerate(many)]
    two = ["definitely\tdefinately\t1.0\tdefinatly\t0.9", "occurrence\toccurence\t1.0\tocurrence\t0.8", "necessary\tneccessary\t1.0\tnecesary\t0.9"]
    f1, f2 = tmp_path / "hand1.variants.tsv", tmp_path / "hand2.variants.tsv"
    f1.write_text("\n".join(one) + "\n", encoding="utf-8")
    f2.write_text("\n".join(two) + "\n", encoding="utf-8")
    return [(str(f1), False), (str(f2), True)]


def build_pair(data_dir, lists, device=0, devices=None, want_oracle=True):
    """The device model and the oracle with eng.aspell and the given variant lists."""
    alphabet, lexicon = os.path.join(data_dir, "simple.alphabet.tsv"), os.path.join(data_dir, "eng.aspell.lexicon")
    g = A.VariantModel(alphabet, A.Weights(), device=device)
    g.read_lexicon(lexicon)
    for f, transparent in lists:
        g.read_variants(f, transparent)
    g.build()
    if devices:
        g.to_devices(devices)
    o = None
    if want_oracle:
        o = O.OracleModel(alphabet_path=alphabet)
        o.read_lexicon(lexicon)
        for f, transparent in lists:
            o.read_variants(f, transparent)
        o.build()
    assert_has_variant_lists(g)
    return g, o


def assert_has_variant_lists(g):
    b = g.encode_batch(["recieve"], A.SearchParameters())
    b.run()
    with pytest.raises(A.AnxError, match="variant lists"):
        b.fetch_compact()
    b.free()


def learn_inputs(words, n_words=400, n_typos=1200, seed=21):
    """Words of the lexicon itself (they gain links to their neighbours: INDEXED entries with VariantOf links) beside misspellings
    (learned strings are TRANSPARENT and not indexed: alone they would not make a variant-list model)."""
    rng = random.Random(seed)
    pool = [w for w in words if 4 <= len(w) <= 12 and w.isalpha()]
    return rng.sample(pool, n_words) + synth.make_queries(words, n_typos, max_len=14, min_len=4, seed=seed)


def learned_list(data_dir, tmp_path, words):
    """The variant list the product learns from learn_inputs (max_matches 3), written out: -> [(path, transparent)].  It is read back
    as an error list (transparent: a learned misspelling is never returned itself, only its references are, each with a `via`), so
    that rows with a `via` also survive a crop to max_matches = 1; words of the lexicon that the list names as variants stay
    ordinary entries (an existing item does not become TRANSPARENT)."""
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    g.build()
    g.learn_variants(learn_inputs(words), A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=3), strict=True, auto_build=False)
    f = tmp_path / "learned.variants.tsv"
    f.write_text(g.variant_list_output(), encoding="utf-8")
    return [(str(f), True)]


def listed_variants(lists):
    """variant strings of the list files (querying one finds the entry itself, whose rows are its references with `via` = the entry)"""
    out = []
    for f, _t in lists:
        for line in open(f, encoding="utf-8").read().split("\n")[:400]:
            fields = line.split("\t")
            out += [x for x in fields[1:] if x and not x.replace(".", "").isdigit()][:2]
    return [x for x in out if len(x.encode("utf-8")) <= 64]


def queries_for(words, lists, n, seed):
    """n inputs: the hand-made misspellings and strings of the lists themselves (their rows carry a `via`) among synthetic queries."""
    listed = listed_variants(lists)
    rng = random.Random(seed)
    qs = HAND_QUERIES[:3] + rng.sample(listed, min(len(listed), max(1, n // 8))) + HAND_QUERIES[3:]
    qs += synth.make_queries(words, max(0, n - len(qs)), max_len=16, seed=seed)
    qs = qs[:n]
    if n > 2:
        rng.shuffle(qs)
    return qs


def small_stats():
    out = (C.c_uint64 * 2)()
    assert L.lib().anx_debug_small_stats(out) == 0
    return out[0], out[1]


def via_batch_path(model, qs, params):
    A.set_switch("ANX_SMALL", "0")
    try:
        return model.find_variants_ids(qs, params, with_via=True)
    finally:
        A.set_switch("ANX_SMALL", None)


def fetch_columns(batch):
    """anx_batch_fetch of a run batch -> (offsets i64[n + 1], vocab_id u64, dist f64, freq f64, via u64) as numpy copies"""
    rows = C.POINTER(L.Result)()
    offs = C.POINTER(C.c_size_t)()
    L.check(L.lib().anx_batch_fetch(batch.h, C.byref(rows), C.byref(offs)))
    try:
        off = np.ctypeslib.as_array(offs, shape=(batch.n + 1,)).astype(np.int64)
        total = int(off[-1])
        dt = np.dtype([("vocab_id", "<u8"), ("dist", "<f8"), ("freq", "<f8"), ("via", "<u8")])
        if total == 0:
            z = np.zeros(0, dtype=dt)
            return off, z["vocab_id"], z["dist"], z["freq"], z["via"]
        a = np.frombuffer((C.c_char * (total * dt.itemsize)).from_address(C.addressof(rows.contents)), dtype=dt).copy()
        return off, a["vocab_id"], a["dist"], a["freq"], a["via"]
    finally:
        L.lib().anx_results_free(rows, offs)


def assert_compact_equals_fetch(batch, coff, rec, via):
    """offsets, ids, `via` and dist_score equal; freq_score equal after rounding fetch()'s to float32; at least one row has a via"""
    off, vid, dist, freq, fvia = fetch_columns(batch)
    assert coff.dtype == np.uint32 and np.array_equal(coff, off)
    assert np.array_equal(rec["vocab_id"], vid) and np.array_equal(rec["dist_score"], dist)
    assert np.array_equal(rec["freq_score"], freq.astype(np.float32))
    assert via.dtype == np.uint32 and via.shape == vid.shape
    assert np.array_equal(np.where(via == 0xFFFFFFFF, np.uint64(0xFFFFFFFFFFFFFFFF), via.astype(np.uint64)), fvia)
    return int((via != 0xFFFFFFFF).sum())
