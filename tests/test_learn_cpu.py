"""Learn mode without a device: the fold of learn_variants over C-oracle rows (anx_learn_apply_rows, the host fold) and the weighted
variant list writers, against the restatement in tests/learn_twin.py; the `learn` subcommand's options."""
import io
import os
import subprocess
import sys

import pytest

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli, synth
from oracle import cwrap as O
from oracle import twin as T

import learn_twin as LT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _models(data_dir):
    alpha = os.path.join(data_dir, "simple.alphabet.tsv")
    lex = os.path.join(data_dir, "eng.aspell.lexicon")
    g = A.VariantModel(alpha, A.Weights(), device=-1)
    g.read_lexicon(lex)
    m = T.VariantModel(T.read_alphabet(alpha))
    m.read_vocabulary(lex)
    return alpha, lex, g, m


def test_learn_fold_matches_restatement(data_dir):
    alpha, lex, g, m = _models(data_dir)
    o = O.OracleModel(alphabet_path=alpha)
    o.read_lexicon(lex)
    o.build()
    words = synth.load_lexicon_words(lex)
    special = ["seperate", "seperate", "recieve", "xqzxqzxqzjjj", "recieve", "separate", "horse", "seperate"]
    qs = synth.make_queries(words, 292, max_len=16, seed=3)
    qs = qs[:100] + special + qs[100:]
    op = O.make_params(("abs", 3), ("abs", 2), 10, 0.25, 2.0)
    counts, vid, dist, _freq, _, _ = O.batch_rows(o, qs, op, stride=16)
    rows = [[(int(vid[i, k]), float(dist[i, k])) for k in range(int(counts[i]))] for i in range(len(qs))]
    assert rows[103] == [], "the separator must have no rows"
    horse = m.encoder["horse"]
    assert rows[106][0][0] == horse, "an exact match"
    # a link that exists before the call: the learned rows of "horse" name its first neighbour again (first mention wins)
    house = rows[106][1][0]
    assert g.add_variant(house, "horse", 0.5) and m.add_variant(house, "horse", 0.5, lexicon_index=len(m.lexicons))
    assert any(r[0] == m.encoder["separate"] for r in rows[105])
    V = g.vocab_size()
    freq_separate = g.vocab_frequency(m.encoder["separate"])
    for _ in range(2):  # the second call meets the links and entries of the first
        assert g.learn_apply_rows(qs, rows) == LT.learn_fold(m, qs, rows)
        LT.assert_same_state(g, m)
    seperate, recieve = m.encoder["seperate"], m.encoder["recieve"]
    assert seperate >= V and recieve >= V
    # two runs of "seperate" per call (the third mention follows other inputs); "recieve" is one run across the row-less input
    assert g.vocab_frequency(seperate) == 4 and g.vocab_frequency(recieve) == 2
    assert g.vocabtype(seperate) == LT.VOCAB_TRANSPARENT and g.vocab_lexindex(seperate) == 1
    assert g.vocab_frequency(m.encoder["separate"]) == freq_separate + 2
    assert [v for v in g.variants(house) if v[1] == horse] == [("ReferenceFor", horse, 0.5)]
    st = A.VariantModel.learn_stats()
    assert st["host_folds"] >= 2 and st["rows"] >= 2 * sum(len(r) for r in rows)


def test_learn_apply_rows_rejects_bad_ids(data_dir):
    _alpha, _lex, g, _m = _models(data_dir)
    with pytest.raises(A.AnxError) as e:
        g.learn_apply_rows(["huis"], [[(g.vocab_size() + 5, 0.5)]])
    assert e.value.code == L.ANX_EINVAL


def test_learn_strict_needs_a_device(data_dir):
    """There is no CPU fallback of strict learning: without a resident model it fails loudly."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _alpha, _lex, g, _m = _models(data_dir)
    g.build()
    with pytest.raises(A.AnxError) as e:
        g.learn_variants(["seperate"], A.SearchParameters())
    assert e.value.code == L.ANX_ENODEVICE


def _writer_models(data_dir, tmp_path):
    alpha = os.path.join(data_dir, "simple.alphabet.tsv")
    lex1, lex2 = str(tmp_path / "one.lexicon"), str(tmp_path / "two.lexicon")
    open(lex1, "w", encoding="utf-8").write("house\t10\nmouse\t5\nhorse\t3\n")
    open(lex2, "w", encoding="utf-8").write("mouse\t7\nhouses\t2\n")
    g = A.VariantModel(alpha, A.Weights(), device=-1)
    m = T.VariantModel(T.read_alphabet(alpha))
    for f in (lex1, lex2):
        g.read_lexicon(f)
        m.read_vocabulary(f)
    # (anx_model_add_variant gives a new variant the lexicon index of the next lexicon: the twin is told the same)
    links = [("house", "hous", 0.75), ("house", "mouse", 0.5), ("mouse", "house", 1.0), ("houses", 'hou"ses', 0.1 + 0.2),
             ("house", "hous", 0.3), ("horse", "hors", 1e-7)]
    for ref, var, score in links:
        rid = m.encoder[ref]
        assert g.add_variant(rid, var, score) == m.add_variant(rid, var, score, lexicon_index=len(m.lexicons))
    return g, m


def test_variant_list_writers(data_dir, tmp_path):
    g, m = _writer_models(data_dir, tmp_path)
    LT.assert_same_state(g, m)
    assert g.variant_list_output(json=False) == LT.variant_list_tsv(m)
    assert g.variant_list_output(json=True) == LT.variant_list_json(m)
    for json in (False, True):
        ext = "json" if json else "tsv"
        for f in m.lexicons:
            if os.path.exists(f"{f}.variants.{ext}"):
                os.remove(f"{f}.variants.{ext}")
        out = io.StringIO()
        cli.write_multi_output(g, json, out)
        exp_out, exp_files = LT.variant_list_multi(m, json)
        assert out.getvalue() == exp_out
        got_files = {i: open(f"{f}.variants.{ext}", encoding="utf-8").read()
                     for i, f in enumerate(m.lexicons) if os.path.exists(f"{f}.variants.{ext}")}
        assert got_files == exp_files and exp_files


def test_learn_help_lists_options():
    r = subprocess.run([sys.executable, "-m", "analiticcl_amd", "learn", "--help"], cwd=REPO, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--iterations", "-I", "--strict", "--multi-output", "-O", "--lexicon", "--max-anagram-distance", "--json"):
        assert opt in r.stdout, opt
