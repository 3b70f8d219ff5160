"""What a run reports of its ranked lists: their total (n_results) and the longest of them (the stride a fixed-stride export needs) come
from k_run_summary, and everything batch_finish reads -- the scan's, the scoring's and the slot lists' fills, the counters, the survivor
total, the confusable counters -- comes down in ONE copy of the run's control block.  Batches of 1, 2049 and 5000 queries (one block of
the summary kernel, one block plus one query, two blocks), a batch without any candidate and an empty one: rows against the oracle,
n_results against the fetched rows, the stride check on both sides of the longest list, and the same rows after every capacity overflowed
(ANX_CAP_DIV=64: the repeated run goes through the same single read-back).  A model with variant lists (its mid-run synchronisation
reads the control block) and a batch with a confusable list (cf_ctr travels in the control block) return the oracle's rows."""
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import synth
from oracle import cwrap as O
from oracle import twin as T

TEST_ALPHABET_TSV = "\n".join(f"{c}\t{c.upper()}" for c in "abcdefghijklmnopqrstuvwxyz") + "\n.\t,\n"
CONF10 = os.path.join(synth.GOLDEN_DATA, "confusables10.tsv")
KW = dict(max_anagram_distance=3, max_edit_distance=2, max_matches=10, score_threshold=0.25, cutoff_threshold=2.0)


@pytest.fixture(scope="module")
def small(data_dir, tmp_path_factory):
    """3000 words of the English lexicon: the device model, the oracle, the words"""
    words = [w for w in synth.load_lexicon_words(os.path.join(data_dir, "eng.aspell.lexicon")) if w.isascii() and w.isalpha()][::37][:3000]
    f = tmp_path_factory.mktemp("summary") / "small.lexicon"
    f.write_text("\n".join(words) + "\n", encoding="utf-8")
    alphabet = os.path.join(data_dir, "simple.alphabet.tsv")
    g = A.VariantModel(alphabet, A.Weights(), device=0)
    g.read_lexicon(str(f))
    g.build()
    o = O.OracleModel(alphabet_path=alphabet)
    o.read_lexicon(str(f))
    o.build()
    return g, o, words, str(f)


def _run(g, qs, p):
    b = g.encode_batch(qs, p)
    b.run()
    return b, b.fetch_arrays(), b.stats()


def _check_stride(b, n, longest):
    import torch
    buf = torch.zeros(max(n, 1) * max(longest, 1) * 16, dtype=torch.uint8, device="cuda:0")
    b.export_topk(buf.data_ptr(), max(longest, 1))      # a stride equal to the longest list is accepted
    torch.cuda.synchronize()
    if longest > 1:
        with pytest.raises(A.AnxError, match="longest result list"):
            b.export_topk(buf.data_ptr(), longest - 1)
    return buf


@pytest.mark.parametrize("nq", [1, 2049, 5000])
def test_totals_and_longest_list(small, nq):
    g, o, words, _ = small
    qs = [words[5]] if nq == 1 else synth.make_queries(words, nq, max_len=16, seed=nq)
    p = A.SearchParameters(**KW)
    b, (off, vid, dist, freq), st = _run(g, qs, p)
    try:
        counts, ovid, odist, ofreq, _tp, _tc = O.batch_rows(o, qs, O.make_params(("abs", 3), ("abs", 2), 10, 0.25, 2.0))
        rows = O.assert_rows_equal(off, vid, dist, freq, np.arange(nq), counts, ovid, odist, ofreq, what=lambda i: qs[i])
        assert st["n_results"] == rows == int(off[-1]) == vid.size and rows >= nq // 2
        longest = int(np.diff(off).max())
        assert nq == 1 or longest > 1
        buf = _check_stride(b, nq, longest)
        rec = np.frombuffer(buf.cpu().numpy().tobytes(), dtype=np.dtype([("vocab_id", "<u4"), ("freq", "<f4"), ("dist", "<f8")])).reshape(nq, max(longest, 1))
        i = int(np.argmax(np.diff(off)))                 # the longest list came through whole
        assert rec[i]["vocab_id"].tolist() == vid[off[i]:off[i + 1]].tolist()
    finally:
        b.free()
    A.set_switch("ANX_CAP_DIV", 64)
    try:
        b, got, st2 = _run(g, qs, p)
        b.free()
    finally:
        A.set_switch("ANX_CAP_DIV", None)
    for x, y in zip((off, vid, dist, freq), got):
        assert np.array_equal(x, y)
    for k in ("n_pairs", "n_results", "n_survivors"):
        assert st[k] == st2[k], k


def test_no_candidates_and_empty_batch(small):
    g, _o, _words, _ = small
    p = A.SearchParameters(**KW)
    qs = ["qqqqqqqqqqqqqq", "zzzzzzzzzzzzzzzzzzzzzzzzzzzzzz", "xxxxxxxxxxjjjjjjjjjj"] * 40
    for cap_div in (None, 64):
        A.set_switch("ANX_CAP_DIV", cap_div)
        try:
            b, (off, vid, _d, _f), st = _run(g, qs, p)
            assert st["n_queries"] == len(qs) and st["n_results"] == 0 == vid.size and not off.any()
            _check_stride(b, len(qs), 0)
            b.free()
            b, (off, vid, _d, _f), st = _run(g, [], p)
            assert off.tolist() == [0] and vid.size == 0 and st["n_results"] == 0
            b.free()
        finally:
            A.set_switch("ANX_CAP_DIV", None)


def test_variant_lists_through_the_control_block(small, data_dir, tmp_path):
    """a model with variant lists keeps one synchronisation in the middle of the run (the row buffer is sized from the survivor total and the
    survivor regions' fills, both read from the control block): rows and `via` against the oracle, also after every capacity overflowed"""
    _g, _o, words, lexfile = small
    rng = random.Random(5)
    refs = rng.sample(words, 60)
    lines = []
    for i, w in enumerate(refs):
        v1 = w[:1] + w[2:] + "x" if len(w) > 3 else w + "xx"
        lines.append(f"{w}\t{v1}\t{0.5 + 0.005 * i}\t{rng.choice(words)}\t0.7")
    lines.append("\t".join([refs[0]] + [x for w in rng.sample(words, 40) for x in (w, "0.6")][:80]))
    vf = tmp_path / "v.variants.tsv"
    vf.write_text("\n".join(lines) + "\n", encoding="utf-8")
    alphabet = os.path.join(data_dir, "simple.alphabet.tsv")
    g = A.VariantModel(alphabet, A.Weights(), device=0)
    o = O.OracleModel(alphabet_path=alphabet)
    for m in (g, o):
        m.read_lexicon(lexfile)
        m.read_variants(str(vf), False)
        m.build()
    qs = [ln.split("\t")[1] for ln in lines[:30]] + synth.make_queries(words, 2100, max_len=16, seed=9)
    p, op = A.SearchParameters(**KW), O.make_params(("abs", 3), ("abs", 2), 10, 0.25, 2.0)
    exp = [o.find_variants_via(q, op) for q in qs]
    assert sum(1 for r in exp for row in r if row[3] is not None) > 20
    for cap_div in (None, 64):
        A.set_switch("ANX_SMALL", "0")
        A.set_switch("ANX_CAP_DIV", cap_div)
        try:
            got = g.find_variants_ids(qs, p, with_via=True)
        finally:
            A.set_switch("ANX_SMALL", None)
            A.set_switch("ANX_CAP_DIV", None)
        for q, r, e in zip(qs, got, exp):
            assert r == e, (cap_div, q)


@pytest.mark.parametrize("early", [False, True])
def test_confusable_list_through_the_control_block(small, early):
    """confusables weighted on the device: the number of edit scripts and the fallback flag (cf_ctr) come down with the control block"""
    _g, _o, words, _ = small
    rng = random.Random(3)
    tw = T.VariantModel(T.TEST_ALPHABET)
    g = A.VariantModel("", alphabet_text=TEST_ALPHABET_TSV, device=0)
    for w in words[:2000]:
        f = rng.randrange(1, 30)
        tw.add_to_vocabulary(w, f)
        g.add_to_vocabulary(w, f)
    for m in (tw, g):
        m.read_confusablelist(CONF10)
        if early:
            m.set_confusables_before_pruning()
        m.build()
    qs = synth.make_queries(words[:2000], 300, max_len=16, seed=21)
    gp = A.SearchParameters(max_anagram_distance=2, max_edit_distance=2, max_matches=5, score_threshold=0.3, cutoff_threshold=2.0)
    tp = T.SearchParameters(("abs", 2), ("abs", 2), 5, 0.3, 2.0, False, 0.0)
    b = g.encode_batch(qs, gp)
    b.run()
    got, st = b.fetch(), b.stats()
    b.free()
    assert st["n_conf_scripts"] > 0 and st["n_results"] == sum(len(r) for r in got)
    changed = 0
    for q, r in zip(qs, got):
        exp = tw.find_variants(q, tp)
        assert [v for v, _d, _f in r] == [x.vocab_id for x in exp], q
        for (v, d, f), x in zip(r, exp):
            assert abs(d - x.dist_score) < 1e-6 and abs(f - x.freq_score) < 1e-6
        changed += any(tw.compute_confusable_weight(q, x.vocab_id) != 1.0 for x in exp)
    assert changed >= 1   # (by the twin) the list did re-weight some query's rows: the comparison above is not vacuous
