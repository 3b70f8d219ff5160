"""Learn mode on the MI355X: learn_variants with the fold on the device (learn.hip) against the restatement in tests/learn_twin.py
over C-oracle rows, the host fold (ANX_LEARN_FOLD=host), the non-strict mode, a multi-replica model and the `learn` command."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import synth
from oracle import cwrap as O
from oracle import twin as T

import learn_twin as LT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _paths(data_dir):
    return os.path.join(data_dir, "simple.alphabet.tsv"), os.path.join(data_dir, "eng.aspell.lexicon")


def _product(data_dir, **kw):
    alpha, lex = _paths(data_dir)
    g = A.VariantModel(alpha, A.Weights(), **kw)
    g.read_lexicon(lex)
    g.build()
    return g


def _twin(data_dir):
    alpha, lex = _paths(data_dir)
    m = T.VariantModel(T.read_alphabet(alpha))
    m.read_vocabulary(lex)
    return m


def _params(max_matches=1):
    return A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=max_matches)


def _queries(data_dir, n, seed):
    words = synth.load_lexicon_words(_paths(data_dir)[1])
    return synth.make_queries(words, n, max_len=16, seed=seed)


def test_learn_strict_device_fold(data_dir):
    qs = _queries(data_dir, 20000, seed=21)
    qs[500:503] = ["seperate", "seperate", "recieve"]
    alpha, lex = _paths(data_dir)
    o = O.OracleModel(alphabet_path=alpha)
    o.read_lexicon(lex)
    o.build()
    counts, vid, dist, _f, _, _ = O.batch_rows(o, qs, O.make_params(("abs", 3), ("abs", 2), 1, 0.25, 2.0), stride=4)
    rows = [[(int(vid[i, k]), float(dist[i, k])) for k in range(int(counts[i]))] for i in range(len(qs))]
    m = _twin(data_dir)
    g = _product(data_dir, device=0)
    before = A.VariantModel.learn_stats()
    c1 = g.learn_variants(qs, _params())
    assert A.VariantModel.learn_stats()["device_folds"] == before["device_folds"] + 1
    assert c1 == LT.learn_fold(m, qs, rows) and c1 > 0
    LT.assert_same_state(g, m)
    assert g.vocabtype(m.encoder["seperate"]) == LT.VOCAB_TRANSPARENT
    s1 = LT.product_state(g)
    c2 = g.learn_variants(qs, _params())
    s2 = LT.product_state(g)
    # the same two iterations with the host fold
    L.set_switch("ANX_LEARN_FOLD", "host")
    try:
        h = _product(data_dir, device=0)
        hb = A.VariantModel.learn_stats()
        assert h.learn_variants(qs, _params()) == c1
        assert LT.product_state(h) == s1
        assert h.learn_variants(qs, _params()) == c2
        assert LT.product_state(h) == s2
        assert A.VariantModel.learn_stats()["host_folds"] == hb["host_folds"] + 2
    finally:
        L.set_switch("ANX_LEARN_FOLD", "device")


def test_learn_non_strict(data_dir):
    words = synth.load_lexicon_words(_paths(data_dir)[1])
    texts = synth.make_running_text(words, 0.08, seed=9)[:50]
    sp = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=5)
    g = _product(data_dir, device=0)
    off, ma, ra = g.find_all_matches_arrays(texts, sp)
    inputs, rows = [], []
    for i, t in enumerate(texts):
        b = t.encode("utf-8")
        for x in ma[off[i]:off[i + 1]]:
            if x["selected"] >= 0:
                inputs.append(b[x["begin"]:x["end"]].decode("utf-8"))
                r = ra[int(x["vb"]) + int(x["selected"])]
                rows.append([(int(r["vocab_id"]), float(r["dist"]))])
    assert len(inputs) > 100
    m = _twin(data_dir)
    exp = LT.learn_fold(m, inputs, rows)
    assert g.learn_variants(texts, sp, strict=False) == exp
    LT.assert_same_state(g, m)


def test_learn_replicas_match_one(data_dir):
    qs = _queries(data_dir, 30000, seed=33)
    one = _product(data_dir, device=0)
    three = _product(data_dir, devices=[0, 0, 0])
    assert three.num_replicas == 3
    before = A.VariantModel.learn_stats()
    assert three.learn_variants(qs, _params(3)) == one.learn_variants(qs, _params(3))
    assert A.VariantModel.learn_stats()["device_folds"] == before["device_folds"] + 2
    assert three.num_replicas == 3
    assert LT.product_state(three) == LT.product_state(one)


def test_learn_cli_round_trip(data_dir, tmp_path):
    alpha, lex = _paths(data_dir)
    qs = _queries(data_dir, 3000, seed=5)
    inp = tmp_path / "learn.txt"
    inp.write_text("\n".join(qs) + "\n", encoding="utf-8")
    r = subprocess.run([sys.executable, "-m", "analiticcl_amd", "learn", "--strict", "-I", "2", "--alphabet", alpha, "--lexicon", lex,
                        "-n", "2", "--device", "0", str(inp)], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    # the restatement: each iteration folds the rows the model gives at its start (CLI defaults k=3 d=2), then rebuilds
    p = _product(data_dir, device=0)
    m = _twin(data_dir)
    params = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=2)
    msgs = []
    for it in range(2):
        rows = p.find_variants_ids(qs, params)
        c = LT.learn_fold(m, qs, rows)
        assert p.learn_apply_rows(qs, rows) == c
        p.build()
        msgs.append(f"(Iteration #{it + 1}: learned {c} variants (out of a total of {len(qs)} input strings)")
    assert r.stdout == LT.variant_list_tsv(m)
    assert [x for x in r.stderr.splitlines() if x.startswith("(Iteration")] == msgs
    # the list read back with --variants gives the same ReferenceFor structure
    vl = tmp_path / "learned.tsv"
    vl.write_text(r.stdout, encoding="utf-8")
    back = A.VariantModel(alpha, A.Weights(), device=-1)
    back.read_lexicon(lex)
    back.read_variants(str(vl))

    def refs_of(texts_and_refs):
        return {t: v for t, v in texts_and_refs if v}

    got = refs_of((back.vocab_text(i), [(back.vocab_text(y), s) for k, y, s in back.variants(i) if k == "ReferenceFor"])
                  for i in range(back.vocab_size()))
    exp = refs_of((v.text, [(m.decoder[y].text, s) for k, y, s in (v.variants or []) if k == "ref_for"]) for v in m.decoder)
    assert got == exp and exp
