"""anx_evaluate_gold on the device (analiticcl_amd/csrc/eval.hip) against the oracle side (tests/eval_twin.py: rows from the C oracle, measures
and reasons from the twin's stages).  Every record is compared field by field with `==`; gold_score bit for bit.  The shapes are the
smallest at which the pass can go wrong: one lane, the wave edge, more than one block, row lists that cross waves and blocks beside
inputs without rows, a chunk seam inside a call, three sections with an empty one."""
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli, synth
from oracle import cwrap as O
from oracle import twin as T

import eval_twin as E
from variant_models_common import build_pair, hand_made_lists, small_stats

CONF10 = os.path.join(synth.GOLDEN_DATA, "confusables10.tsv")
SEED = 1   # edited_pairs(eng.aspell, 257, SEED) under k = 3, d = 2, n = 10: 175 RANKED, 34 ANAGRAM, 44 EDIT, 4 CROPPED (counted with the oracle side alone)


def oracle_params(p):
    return O.make_params(p.max_anagram_distance, p.max_edit_distance, p.max_matches, p.score_threshold, p.cutoff_threshold,
                         p.stop_at_exact_match, p.freq_weight)


def product_params(p):
    def th(t):
        return int(t[1]) if t[0] == "abs" else float(t[1]) if t[0] == "ratio" else (float(t[1]), int(t[2]))
    return A.SearchParameters(max_anagram_distance=th(p.max_anagram_distance), max_edit_distance=th(p.max_edit_distance), max_matches=p.max_matches,
                              score_threshold=p.score_threshold, cutoff_threshold=p.cutoff_threshold, stop_criterion=bool(p.stop_at_exact_match),
                              freq_weight=p.freq_weight)


def bits(x):
    return struct.pack("<d", float(x))


def assert_records(rec, expected, pairs):
    assert len(rec) == len(expected) == len(pairs)
    for i, (e, (a, g)) in enumerate(zip(expected, pairs)):
        got = {k: rec[k][i].item() for k in E.FIELDS}
        what = (i, a[:40], g[:40], got, e)
        for k in E.FIELDS:
            if k != "gold_score":
                assert got[k] == e[k], (k,) + what
        assert bits(got["gold_score"]) == bits(e["gold_score"]), what
    assert not rec["_pad"].any()


def check(g, side, pairs, P, **kw):
    expected = [E.expected_record(side, a, b, P) for a, b in pairs]
    rec = g.evaluate_arrays([a for a, _ in pairs], [b for _, b in pairs], product_params(P), **kw)
    assert_records(rec, expected, pairs)
    return rec, expected


# ---- models ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand(data_dir, tmp_path_factory):
    alphabet = os.path.join(data_dir, "simple.alphabet.tsv")
    lex = tmp_path_factory.mktemp("evalhand") / "hand.lexicon"
    lex.write_text("\n".join(E.HAND_WORDS) + "\n")
    g = A.VariantModel(alphabet, A.Weights(), device=0)
    g.read_lexicon(str(lex))
    g.build()
    tw = T.VariantModel(T.read_alphabet(alphabet))
    o = O.OracleModel(alphabet_path=alphabet)
    for w in E.HAND_WORDS:
        assert tw.add_to_vocabulary(w) == o.add(w)
    tw.build()
    o.build()
    return g, E.twin_side(tw, lambda text, P: o.find_variants_via(text, oracle_params(P))), str(lex)


def eng_side(data_dir, o, words):
    encoder = {w: 3 + i for i, w in enumerate(words)}   # ids 0-2 are <bos>, <eos>, <unk>; every lexicon line is a new item
    return E.oracle_side(o, T.read_alphabet(os.path.join(data_dir, "simple.alphabet.tsv")), T.Weights(), encoder, lambda v: (v >= 3, False), oracle_params)


@pytest.fixture(scope="module")
def eng(data_dir):
    alphabet, lexicon = os.path.join(data_dir, "simple.alphabet.tsv"), os.path.join(data_dir, "eng.aspell.lexicon")
    g = A.VariantModel(alphabet, A.Weights(), device=0)
    g.read_lexicon(lexicon)
    g.build()
    o = O.OracleModel(alphabet_path=alphabet)
    o.read_lexicon(lexicon)
    o.build()
    words = synth.load_lexicon_words(lexicon)
    side = eng_side(data_dir, o, words)
    P = T.SearchParameters(("abs", 3), ("abs", 2), 10, 0.25, 2.0, False, 0.0)
    pairs = E.edited_pairs(words, 257, SEED)
    expected = [E.expected_record(side, a, b, P) for a, b in pairs]   # computed once, shared by the tests below
    for (a, b), e in zip(pairs, expected):
        assert o.text(e["gold_vocab_id"]) == b
    return g, o, words, side, P, pairs, expected


# ---- every reason ---------------------------------------------------------------------------------------------------------------------
def test_every_reason_on_the_hand_made_lexicon(hand):
    g, side, _lex = hand
    seen = set()
    for P, cases in ((E.hand_params(), E.HAND_PAIRS), (E.hand_params(stop_at_exact_match=True), E.HAND_PAIRS_STOP)):
        pairs = [(a, b) for a, b, _r, _k in cases]
        rec, expected = check(g, side, pairs, P)
        for (a, b, reason, rank), e in zip(cases, expected):
            assert (e["reason"], e["rank"]) == (reason, rank), (a, b[:10], e)
        seen |= set(rec["reason"].tolist())
        assert_records(g.evaluate_arrays([a for a, _ in pairs], [b for _, b in pairs], product_params(P), packed=False), expected, pairs)
    assert seen == set(range(8))
    d = g.evaluate(["abcdef", "abcdef"], ["xbcdef", "nothere"], product_params(E.hand_params()))
    assert d[0]["rank"] == 2 and d[0]["reason"] == "RANKED" and d[0]["gold_score"] == 0.75
    assert d[1]["rank"] is None and d[1]["gold_vocab_id"] is None and d[1]["reason"] == "NOT_A_RESULT"


# ---- wave and block edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_and_block_edges(eng, n):
    g, _o, _words, _side, P, pairs, expected = eng
    rec = g.evaluate_arrays([a for a, _ in pairs[:n]], [b for _, b in pairs[:n]], product_params(P))
    assert_records(rec, expected[:n], pairs[:n])
    if n == 257:
        reasons = set(rec["reason"].tolist())
        assert E.RANKED in reasons and E.CROPPED in reasons and (E.ANAGRAM in reasons or E.EDIT in reasons)
        s = A.VariantModel.evaluate_summary(rec)
        assert s["n"] == 257 and s["gold_known"] == 257 and s["reasons"]["RANKED"] == int((rec["rank"] >= 0).sum())


def test_row_lists_that_cross_waves(eng):
    """3-letter inputs with every candidate kept (hundreds of rows each: k = d = 3 by ratio, no crop, no thresholds) beside inputs with
    no rows at all; gold deep in the list, at its end, and absent.  Then one call whose inputs all have no rows."""
    g, o, _words, side, _P, _pairs, _expected = eng
    P = T.SearchParameters(("ratio", 1.0), ("ratio", 1.0), 0, 0.0, 0.0, False, 0.0)
    none = ["qqqqqqqqqqqqqqqqqqqqjjjjjjjjjj", "zzzzzzzzzzzzzzzzzzzzzzzzzzzzzzxxxxx"]
    pairs = []
    for a in ("cat", "teh", "dog", "the"):
        rows = o.find_variants_via(a, oracle_params(P))
        assert len(rows) > 200, (a, len(rows))
        pairs += [(none[0], "cat"), (a, o.text(rows[len(rows) // 2][0])), (a, o.text(rows[-1][0])), (a, o.text(rows[65][0])), (none[1], "nothere"),
                  (a, "incomprehensible")]
    rec, _ = check(g, side, pairs, P)
    assert rec["n_results"].max() > 200 and (rec["n_results"] == 0).sum() == 8 and rec["rank"].max() > 128
    rec, _ = check(g, side, [(none[0], "cat"), (none[1], "dog"), (none[0], none[0])] * 23, P)
    assert not rec["n_results"].any() and (rec["rank"] == -1).all() and (rec["top_vocab_id"] == 0xFFFFFFFF).all()


def test_chunk_seams(eng):
    g, _o, _words, _side, P, pairs, expected = eng
    a, b = [x for x, _ in pairs[:130]], [y for _, y in pairs[:130]]
    whole = g.evaluate_arrays(a, b, product_params(P))
    cut, cut_pairs = g.evaluate_arrays(a, b, product_params(P), chunk=64, with_pairs=True)
    assert whole.tobytes() == cut.tobytes()
    assert_records(cut, expected[:130], pairs[:130])
    _rec, whole_pairs = g.evaluate_arrays(a, b, product_params(P), with_pairs=True)
    assert whole_pairs.tobytes() == cut_pairs.tobytes()
    with pytest.raises(A.AnxError) as e:
        g.evaluate_arrays(a, b, product_params(P), chunk=0)
    assert e.value.code == L.ANX_EINVAL


def test_three_replicas(eng, data_dir):
    g1, _o, _words, _side, P, pairs, expected = eng
    g3 = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g3.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    g3.build()
    g3.to_devices([0, 0, 0])
    assert g3.num_replicas == 3
    for n in (2, 65):   # n = 2: three sections, one of them empty
        a, b = [x for x, _ in pairs[:n]], [y for _, y in pairs[:n]]
        rec = g3.evaluate_arrays(a, b, product_params(P))
        assert rec.tobytes() == g1.evaluate_arrays(a, b, product_params(P)).tobytes()
        assert_records(rec, expected[:n], pairs[:n])


# ---- variant lists and confusables ----------------------------------------------------------------------------------------------------
def test_variant_lists(eng, data_dir, tmp_path):
    _g, _o, words, _side, P, _pairs, _expected = eng
    lists = hand_made_lists(tmp_path, words)
    g, o = build_pair(data_dir, lists)
    alphabet = T.read_alphabet(os.path.join(data_dir, "simple.alphabet.tsv"))
    tw = E.light_twin(alphabet, [(w, None) for w in words])
    for f, transparent in lists:
        tw.read_variants(f, transparent)
    side = E.oracle_side(o, alphabet, T.Weights(), tw.encoder, lambda v: (tw.decoder[v].indexed, tw.decoder[v].transparent), oracle_params)
    pairs = [("recieve", "receive"), ("recieve", "reprieve"), ("definately", "definitely"), ("definately", "definately"), ("definatly", "definatly"),
             ("seperate", "separate"), ("desperate", "separate"), ("thier", "their"), ("thier", "there"), ("qwertyx", "qwertyx"), ("occurence", "occurrence"),
             ("releive", "relieve"), ("releive", "recieve"), ("neccessary", "necesary")]
    rec, expected = check(g, side, pairs, P)
    for (a, b), e in zip(pairs, expected):
        assert o.text(e["gold_vocab_id"]) == b, (a, b)
    by = {p: e for p, e in zip(pairs, expected)}
    assert by[("definately", "definitely")]["reason"] == E.RANKED      # a gold reached only through `via`
    assert by[("definately", "definately")]["reason"] == E.NOT_A_RESULT and by[("definately", "definately")]["gold_vocab_id"] != E.NONE   # a TRANSPARENT gold
    assert by[("recieve", "receive")]["reason"] == E.RANKED
    check(g, side, pairs, T.SearchParameters(("abs", 3), ("abs", 2), 1, 0.25, 2.0, False, 0.0))


@pytest.fixture(scope="module")
def nld(data_dir):
    alphabet, lexicon = os.path.join(data_dir, "simple.alphabet.tsv"), os.path.join(data_dir, "nld.aspell.lexicon")
    o = O.OracleModel(alphabet_path=alphabet)
    o.read_lexicon(lexicon)
    o.build()
    words = synth.load_lexicon_words(lexicon)
    return alphabet, lexicon, o, words


@pytest.mark.parametrize("early", [False, True])
def test_confusables_late_and_early(nld, early):
    alphabet, lexicon, o, words = nld
    g = A.VariantModel(alphabet, A.Weights(), device=0)
    g.read_lexicon(lexicon)
    g.read_confusablelist(CONF10)
    tw = E.light_twin(T.read_alphabet(alphabet), [(w, None) for w in words])
    tw.read_confusablelist(CONF10)
    if early:
        g.set_confusables_before_pruning()
        tw.set_confusables_before_pruning()
    g.build()
    side = E.oracle_side(o, tw.alphabet, T.Weights(), tw.encoder, lambda v: (v >= 3, False), oracle_params)
    side.rows = E.rows_by_twin_tail(o, tw, oracle_params)   # the C oracle's instances through the twin's tail: it weights confusables
    P = T.SearchParameters(("abs", 3), ("abs", 2), 10, 0.25, 2.0, False, 0.0)
    pairs = E.edited_pairs(words, 64, seed=3)
    rec, expected = check(g, side, pairs, P)
    weighted = sum(1 for (a, b), e in zip(pairs, expected) if e["rank"] >= 0 and tw.compute_confusable_weight(a, e["gold_vocab_id"]) != 1.0)
    assert weighted > 0, "no ranked gold carries a confusable weight: the case is not covered"
    if not early:
        A.set_switch("ANX_CONFUSABLES", "host")
        try:
            with pytest.raises(A.AnxError) as e:
                g.evaluate_arrays([a for a, _ in pairs], [b for _, b in pairs], product_params(P))
            assert e.value.code == L.ANX_EINVAL
        finally:
            A.set_switch("ANX_CONFUSABLES", None)


# ---- the call and its neighbours ------------------------------------------------------------------------------------------------------
def test_no_side_effect_and_pairs_output(eng):
    g, _o, _words, _side, P, pairs, expected = eng
    a, b = [x for x, _ in pairs[:100]], [y for _, y in pairs[:100]]
    before = g.find_variants_ids(a, product_params(P))
    t0 = small_stats()
    rec, got_pairs = g.evaluate_arrays(a, b, product_params(P), with_pairs=True)
    assert small_stats() == t0
    assert g.find_variants_ids(a, product_params(P)) == before
    assert_records(rec, expected[:100], pairs[:100])
    cols = g.score_pairs_arrays(a, b)
    for k in A.VariantModel.PAIR_KEYS:
        assert got_pairs[k].tobytes() == cols[k].tobytes(), k
    assert not got_pairs["_pad"].any()
    # the ranked row the record points at is the row find_variants returns
    for i, rows in enumerate(before):
        if rec["rank"][i] >= 0:
            assert rows[rec["rank"][i]][0] == rec["gold_vocab_id"][i] and bits(rows[rec["rank"][i]][1]) == bits(rec["gold_score"][i])
        assert len(rows) == rec["n_results"][i]


def test_cli_evaluate(hand, data_dir, tmp_path, capsys):
    _g, _side, lex = hand
    inp = tmp_path / "pairs.tsv"
    inp.write_text("abcdef\txbcdef\nabcdef\tabcdyz\nabcdef\t\n")
    summary = tmp_path / "summary.json"
    common = ["evaluate", "-a", os.path.join(data_dir, "simple.alphabet.tsv"), "-l", lex, "-k", "2", "-d", "1", "-n", "3", "-t", "0.71", "-T", "0", "--device", "0"]
    assert cli.main(common + [str(inp)]) == 0
    cap = capsys.readouterr()
    assert cap.out == "abcdef\txbcdef\t3\tabcdef\t0.75\t1\tRANKED\nabcdef\tabcdyz\t-\tabcdef\t0.625\t2\tANAGRAM\nabcdef\t\t-\tabcdef\t0\t0\tSTATUS\n"
    assert "pairs: 3\n" in cap.err and "accuracy@1: 0\n" in cap.err and "ANAGRAM: 1\n" in cap.err
    assert cli.main(common + ["--summary-json", str(summary), str(inp)]) == 0
    import json
    s = json.loads(summary.read_text())
    assert s["n"] == 3 and s["reasons"]["RANKED"] == 1 and s["mrr"] == (1 / 3) / 3
    assert capsys.readouterr().err == ""
