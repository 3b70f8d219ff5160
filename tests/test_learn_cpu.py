"""Learn mode without a device: the fold of learn_variants over C-oracle rows (anx_learn_apply_rows, the host fold) and the weighted
variant list writers, against the restatement in tests/learn_twin.py; the generated edge cases of tests/learn_cases.py through the host
fold; the `learn` subcommand's options."""
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

import learn_cases as LC
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


# ---- the generated cases of tests/learn_cases.py through the host fold ---------------------------------------------------------------
@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("case", LC.all_cases(seeds=(1, 2)), ids=repr)
def test_generated_cases_host_fold(data_dir, tmp_path, case, kind):
    """Every hand-made and random case, call after call: count and the whole state (text, frequency, type, lexicon index, links in
    order with their scores) of the host fold equal the restatement of the reference's loop.  What the device fold is compared with
    (tests/test_gpu_learn_fold.py) is thereby itself pinned."""
    g, m = LC.build_models(os.path.join(data_dir, "simple.alphabet.tsv"), tmp_path, kind)
    LT.assert_same_state(g, m)
    ncalls = 0
    for inputs, rows in case.calls(m):
        assert all(vid < len(m.decoder) for rs in rows for vid, _ in rs)
        assert g.learn_apply_rows(inputs, rows) == LT.learn_fold(m, inputs, rows)
        LT.assert_same_state(g, m)
        ncalls += 1
    assert ncalls >= 2


def test_hand_cases_say_what_they_claim(data_dir, tmp_path):
    """The outcomes the comments of the hand-made cases promise, read off the restatement (which the test above ties to the product)."""
    alpha = os.path.join(data_dir, "simple.alphabet.tsv")
    cases = {c.name: c for c in LC.HAND_CASES}

    def run(name, kind="plain", ncalls=1):
        _g, m = LC.build_models(alpha, tmp_path, kind)
        it = cases[name].calls(m)
        counts = [LT.learn_fold(m, *next(it)) for _ in range(ncalls)]
        return m, counts

    lex = dict(LC.LEXICON)
    m, c = run("duplicate_pairs")
    hauze, house = m.encoder["hauze"], m.encoder["house"]
    assert c == [7] and m.decoder[hauze].frequency == 2
    assert [v for v in m.decoder[house].variants if v[0] == "ref_for"] == [("ref_for", hauze, 0.9), ("ref_for", m.encoder["xx"], 0.7)]
    assert [s for k, y, s in m.decoder[hauze].variants if y == house] == [0.9, 0.5, 0.1, 0.2]
    m, c = run("own_id_between_links")
    assert c == [4] and m.decoder[m.encoder["house"]].variants == [("variant_of", m.encoder["mouse"], 0.5), ("variant_of", m.encoder["horse"], 0.4),
                                                                 ("variant_of", m.encoder["mouse"], 0.3)]
    m, _ = run("rowless_between_mentions")
    f = lambda t: m.decoder[m.encoder[t]].frequency
    assert (f("house"), f("recieve"), f("mouse"), f("teh")) == (lex["house"] + 1, 1, lex["mouse"] + 2, 2)
    assert "zzzz" not in m.encoder and "" not in m.encoder
    m, _ = run("runs_across_block_borders")
    f = lambda t: m.decoder[m.encoder[t]].frequency
    assert (f("house"), f("mouse"), f("qqq")) == (lex["house"] + 1, lex["mouse"] + 2, 2)
    m, _ = run("prefix_family")
    V = 3 + len(LC.LEXICON)
    assert [v.text for v in m.decoder[V:]] == ["abcde", "abcdef", "b", "ééé", LC.LONG[:66], LC.LONG]
    m, c = run("no_rows")
    assert c == [0] and len(m.decoder) == V
    m, c = run("second_call", ncalls=2)
    hauze, house = m.encoder["hauze"], m.encoder["house"]
    assert c == [3, 7] and m.decoder[hauze].frequency == 2 and m.decoder[m.encoder["mauze"]].frequency == 2
    assert [v for v in m.decoder[house].variants if v[1] == hauze] == [("ref_for", hauze, 0.9)]
    assert ("ref_for", m.encoder["hauzen"], 0.6) in m.decoder[hauze].variants
    m, _ = run("links_before_the_call", kind="variants")
    hous, house = m.encoder["hous"], m.encoder["house"]
    assert hous < len(m.decoder) - 1 and [v for v in m.decoder[house].variants if v[1] == hous] == [("ref_for", hous, 0.75)]
    assert [s for k, y, s in m.decoder[hous].variants if k == "variant_of" and y == house] == [0.75, 0.2, 0.3]


def test_learn_fold_rows_device_validates_like_apply_rows(data_dir, tmp_path):
    """The device fold's test hook checks its rows as anx_learn_apply_rows does, and there is no host fall-back behind it."""
    g, m = LC.build_models(os.path.join(data_dir, "simple.alphabet.tsv"), tmp_path, "plain")
    for bad in ([[(g.vocab_size(), 0.5)]], [[(0, 0.5), (g.vocab_size() + 5, 0.5)]]):
        for call in (g.learn_apply_rows, g.learn_fold_rows_device):
            with pytest.raises(A.AnxError) as e:
                call(["huis"], bad)
            assert e.value.code == L.ANX_EINVAL
    with pytest.raises(A.AnxError) as e:
        g.learn_fold_rows_device(["huis"], [[(3, 0.5)]], n_sections=0)
    assert e.value.code == L.ANX_EINVAL
    with pytest.raises(A.AnxError) as e:   # (the model is not resident on a device: it was never built for one)
        g.learn_fold_rows_device(["huis"], [[(3, 0.5)]])
    assert e.value.code == L.ANX_ENODEVICE
    LT.assert_same_state(g, m)
