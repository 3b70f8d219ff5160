"""anx_evaluate_sweep on the device (analiticcl_amd/csrc/sweep.hip) against two independent sides: the oracle side's expected records
(tests/eval_twin.py) reduced by the helper (tests/sweep_twin.py), and the product's own evaluate_arrays per parameter set.  Every field
of every summary is compared with `==`, records byte for byte.  The shapes are the smallest at which the pass can go wrong: one lane,
the wave and block edges, more than two blocks, one counter under full contention, ranks beyond the last bin, chunk seams, three
sections with an empty one."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli, synth
from oracle import cwrap as O
from oracle import twin as T

import eval_twin as E
import sweep_twin as S
from variant_models_common import build_pair, hand_made_lists, small_stats

CONF10 = os.path.join(synth.GOLDEN_DATA, "confusables10.tsv")
NONE_INPUTS = ["qqqqqqqqqqqqqqqqqqqqjjjjjjjjjj", "zzzzzzzzzzzzzzzzzzzzzzzzzzzzzzxxxxx"]   # test_row_lists_that_cross_waves' inputs without rows


def oracle_params(p):
    return O.make_params(p.max_anagram_distance, p.max_edit_distance, p.max_matches, p.score_threshold, p.cutoff_threshold,
                         p.stop_at_exact_match, p.freq_weight)


def product_params(p):
    def th(t):
        return int(t[1]) if t[0] == "abs" else float(t[1]) if t[0] == "ratio" else (float(t[1]), int(t[2]))
    return A.SearchParameters(max_anagram_distance=th(p.max_anagram_distance), max_edit_distance=th(p.max_edit_distance), max_matches=p.max_matches,
                              score_threshold=p.score_threshold, cutoff_threshold=p.cutoff_threshold, stop_criterion=bool(p.stop_at_exact_match),
                              freq_weight=p.freq_weight)


def sweep(g, pairs, Ps, **kw):
    return g.evaluate_sweep_arrays([a for a, _ in pairs], [b for _, b in pairs], [product_params(P) for P in Ps], **kw)


def oracle_records(side, pairs, Ps):
    return [[E.expected_record(side, a, b, P) for a, b in pairs] for P in Ps]


def reduced(records_per_set):
    """the helper's summaries of per-set records (dict lists or arrays), the first set being the baseline"""
    return [S.summarize(r, baseline=records_per_set[0]) for r in records_per_set]


def assert_summaries(got, expected):
    assert len(got) == len(expected)
    for s, (g, e) in enumerate(zip(got, expected)):
        g = S.of_product(g)
        for k in S.KEYS:
            assert g[k] == e[k], (s, k, g[k], e[k])


def assert_against_evaluate(g, pairs, Ps, **kw):
    """summaries and records of one sweep against evaluate_arrays per set"""
    sums, rec = sweep(g, pairs, Ps, with_records=True, **kw)
    per_set = [g.evaluate_arrays([a for a, _ in pairs], [b for _, b in pairs], product_params(P)) for P in Ps]
    assert rec.shape == (len(Ps), len(pairs))
    for s, r in enumerate(per_set):
        assert rec[s].tobytes() == r.tobytes(), s
    assert_summaries(sums, reduced(per_set))
    return sums, rec


# ---- models ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand(data_dir, tmp_path_factory):
    alphabet = os.path.join(data_dir, "simple.alphabet.tsv")
    lex = tmp_path_factory.mktemp("sweephand") / "hand.lexicon"
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
    side = E.twin_side(tw, lambda text, P: o.find_variants_via(text, oracle_params(P)))
    pairs = [(a, b) for a, b, _r, _k in E.HAND_PAIRS + E.HAND_PAIRS_STOP]
    Ps = [E.hand_params(), E.hand_params(stop_at_exact_match=True), E.hand_params(max_edit_distance=("ratio", 0.34)),
          E.hand_params(max_matches=1, score_threshold=0.9)]
    expected = oracle_records(side, pairs, Ps)   # computed once, shared by the tests below
    return g, side, str(lex), pairs, Ps, expected


EDGE_SETS = [T.SearchParameters(("abs", 3), ("abs", 2), 10, 0.25, 2.0, False, 0.0), T.SearchParameters(("abs", 2), ("abs", 1), 1, 0.25, 2.0, False, 0.0)]


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
    encoder = {w: 3 + i for i, w in enumerate(words)}   # ids 0-2 are <bos>, <eos>, <unk>; every lexicon line is a new item
    side = E.oracle_side(o, T.read_alphabet(alphabet), T.Weights(), encoder, lambda v: (v >= 3, False), oracle_params)
    pairs = E.edited_pairs(words, 513, seed=1)
    expected = oracle_records(side, pairs, EDGE_SETS)   # computed once, shared by the tests below
    return g, o, words, side, pairs, expected


# ---- every reason, four sets ----------------------------------------------------------------------------------------------------------
def test_four_sets_on_the_hand_made_lexicon(hand):
    g, _side, _lex, pairs, Ps, expected = hand
    want = reduced(expected)
    assert (want[2]["reasons"], want[3]["reasons"]) != (want[0]["reasons"], want[0]["reasons"])   # the ratio for d and the crop to one row change something
    sums, rec = assert_against_evaluate(g, pairs, Ps)
    assert_summaries(sums, want)
    assert set(np.unique(rec["reason"]).tolist()) == set(range(8))
    assert sums["reasons"][0][E.EXACT_STOP] != sums["reasons"][1][E.EXACT_STOP]
    assert (sums["n"] == len(pairs)).all() and sums["gained_at_1"][0] == 0 and sums["lost_at_1"][0] == 0
    pointer = sweep(g, pairs, Ps, packed=False)
    assert pointer.tobytes() == sums.tobytes()
    d = g.evaluate_sweep([a for a, _ in pairs], [b for _, b in pairs], [product_params(P) for P in Ps])
    for s, e in enumerate(want):
        assert d[s]["reasons"] == dict(zip(E.REASONS, e["reasons"])) and d[s]["rank_hist"] == e["rank_hist"]
        assert d[s]["accuracy_at_1"] == e["rank_hist"][0] / len(pairs) and d[s]["mrr"] == e["rr_fixed"] / 2.0 ** 32 / len(pairs)
        assert (d[s]["n_results"], d[s]["gained_at_1"], d[s]["lost_at_1"]) == (e["n_results"], e["gained_at_1"], e["lost_at_1"])


# ---- wave and block edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_wave_and_block_edges(eng, n):
    g, _o, _words, _side, pairs, expected = eng
    sums, rec = sweep(g, pairs[:n], EDGE_SETS, with_records=True)
    want = reduced([e[:n] for e in expected])
    assert_summaries(sums, want)
    assert_summaries(sums, reduced([rec[0], rec[1]]))
    if n == 257:   # counted with the oracle side alone (tests/test_gpu_evaluate.py): the bins are populated
        assert [want[0]["reasons"][r] for r in (E.RANKED, E.ANAGRAM, E.EDIT, E.CROPPED)] == [175, 34, 44, 4]
    if n == 513:
        assert int(sums["gained_at_1"][1]) + int(sums["lost_at_1"][1]) > 0
        at0, at1 = rec[0]["rank"] == 0, rec[1]["rank"] == 0
        assert int(sums["gained_at_1"][1]) == int((at1 & ~at0).sum()) and int(sums["lost_at_1"][1]) == int((at0 & ~at1).sum())
        assert sum(1 for b in want[0]["rank_hist"] if b) > 3


def test_one_counter_under_full_contention(eng):
    g, _o, _words, side, _pairs, _expected = eng
    pairs = [(NONE_INPUTS[i % 2], "cat") for i in range(300)]
    want = [E.expected_record(side, a, b, EDGE_SETS[0]) for a, b in pairs[:2]]
    assert want[0]["reason"] == want[1]["reason"] != E.RANKED and want[0]["n_results"] == 0
    sums = sweep(g, pairs, EDGE_SETS[:1])
    reasons = [0] * 8
    reasons[want[0]["reason"]] = 300
    assert sums["reasons"][0].tolist() == reasons
    assert (int(sums["n"][0]), int(sums["gold_known"][0]), int(sums["n_results"][0]), int(sums["rr_fixed"][0])) == (300, 300, 0, 0)
    assert not sums["rank_hist"][0].any()


def test_the_overflow_bin(eng):
    """test_row_lists_that_cross_waves' parameters: every candidate of a 3-letter input is kept, gold in the middle and at the end of
    lists of more than 200 rows."""
    g, o, _words, side, _pairs, _expected = eng
    P = T.SearchParameters(("ratio", 1.0), ("ratio", 1.0), 0, 0.0, 0.0, False, 0.0)
    pairs = []
    for a in ("cat", "teh", "dog", "the"):
        rows = o.find_variants_via(a, oracle_params(P))
        assert len(rows) > 200, (a, len(rows))
        pairs += [(NONE_INPUTS[0], "cat"), (a, o.text(rows[len(rows) // 2][0])), (a, o.text(rows[-1][0])), (a, o.text(rows[65][0])), (a, o.text(rows[62][0])),
                  (a, o.text(rows[63][0])), (a, o.text(rows[0][0])), (a, "incomprehensible")]
    want = reduced(oracle_records(side, pairs, [P]))
    assert want[0]["rank_hist"][63] >= 12 and want[0]["rank_hist"][62] == 4 and want[0]["rank_hist"][0] == 4
    sums = sweep(g, pairs, [P])
    assert int(sums["rank_hist"][0][63]) > 0 and int(sums["rr_fixed"][0]) == want[0]["rr_fixed"]
    assert_summaries(sums, want)


# ---- what is shared between the sets --------------------------------------------------------------------------------------------------
def test_sharing_is_real(eng):
    g, _o, _words, _side, pairs, expected = eng
    Ps = EDGE_SETS + [T.SearchParameters(("abs", 3), ("abs", 1), 3, 0.25, 2.0, False, 0.0)]
    whole = sweep(g, pairs[:130], Ps)
    t0 = A.VariantModel.sweep_stats()
    cut = sweep(g, pairs[:130], Ps, chunk=64)
    t1 = A.VariantModel.sweep_stats()
    grew = {k: t1[k] - t0[k] for k in t0}
    assert (grew["calls"], grew["chunks"], grew["pair_passes"], grew["lookups"], grew["sets"]) == (1, 3, 3, 3, 9)
    assert grew["batch_runs"] == 9   # 64 inputs are one round of the batch path
    # out == NULL: one summary per set and chunk and nothing else.  The counter holds the copies sweep.hip itself issues; the batch
    # path's control reads happen inside anx_batch_run and are documented (anx.h) to add nothing here.
    assert grew["bytes_down"] == 9 * 624
    assert cut.tobytes() == whole.tobytes()
    assert_summaries(whole[:2], reduced([e[:130] for e in expected]))
    _s, rec, prs = sweep(g, pairs[:130], Ps, chunk=64, with_records=True, with_pairs=True)
    t2 = A.VariantModel.sweep_stats()
    assert t2["bytes_down"] - t1["bytes_down"] == 9 * 624 + 3 * 130 * 32 + 130 * 24
    _s, whole_rec, whole_prs = sweep(g, pairs[:130], Ps, with_records=True, with_pairs=True)
    assert rec.tobytes() == whole_rec.tobytes() and prs.tobytes() == whole_prs.tobytes()
    with pytest.raises(A.AnxError) as e:
        sweep(g, pairs[:130], Ps, chunk=0)
    assert e.value.code == L.ANX_EINVAL


def test_degenerate_set_lists(eng):
    g, _o, _words, _side, pairs, _expected = eng
    assert_against_evaluate(g, pairs[:100], EDGE_SETS[:1])
    sums = sweep(g, pairs[:100], [EDGE_SETS[1], EDGE_SETS[1]])
    assert sums[0].tobytes() == sums[1].tobytes()
    assert int(sums["gained_at_1"][1]) == 0 and int(sums["lost_at_1"][1]) == 0 and int(sums["n"][1]) == 100


def test_three_replicas(eng, data_dir):
    g1, _o, _words, _side, pairs, _expected = eng
    g3 = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g3.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    g3.build()
    g3.to_devices([0, 0, 0])
    assert g3.num_replicas == 3
    for n in (2, 65):   # n = 2: three sections, one of them empty
        s3, r3 = sweep(g3, pairs[:n], EDGE_SETS, with_records=True)
        s1, r1 = sweep(g1, pairs[:n], EDGE_SETS, with_records=True)
        assert s3.tobytes() == s1.tobytes() and r3.tobytes() == r1.tobytes()


# ---- variant lists and confusables ----------------------------------------------------------------------------------------------------
def test_variant_lists(eng, data_dir, tmp_path):
    _g, _o, words, _side, _pairs, _expected = eng
    g, _o2 = build_pair(data_dir, hand_made_lists(tmp_path, words), want_oracle=False)
    pairs = [("recieve", "receive"), ("recieve", "reprieve"), ("definately", "definitely"), ("definately", "definately"), ("definatly", "definatly"),
             ("seperate", "separate"), ("desperate", "separate"), ("thier", "their"), ("thier", "there"), ("qwertyx", "qwertyx"), ("occurence", "occurrence"),
             ("releive", "relieve"), ("releive", "recieve"), ("neccessary", "necesary")]   # test_variant_lists' pairs (tests/test_gpu_evaluate.py)
    sums, _rec = assert_against_evaluate(g, pairs, [EDGE_SETS[0], T.SearchParameters(("abs", 3), ("abs", 2), 1, 0.25, 2.0, False, 0.0)])
    assert int(sums["reasons"][0][E.RANKED]) > 0 and int(sums["reasons"][0][E.NOT_A_RESULT]) > 0


@pytest.mark.parametrize("early", [False, True])
def test_confusables_late_and_early(data_dir, early):
    alphabet, lexicon = os.path.join(data_dir, "simple.alphabet.tsv"), os.path.join(data_dir, "nld.aspell.lexicon")
    g = A.VariantModel(alphabet, A.Weights(), device=0)
    g.read_lexicon(lexicon)
    g.read_confusablelist(CONF10)
    if early:
        g.set_confusables_before_pruning()
    g.build()
    pairs = E.edited_pairs(synth.load_lexicon_words(lexicon), 64, seed=3)
    sums, _rec = assert_against_evaluate(g, pairs, EDGE_SETS)
    assert int(sums["reasons"][0][E.RANKED]) > 0
    if not early:
        A.set_switch("ANX_CONFUSABLES", "host")
        try:
            with pytest.raises(A.AnxError) as e:
                sweep(g, pairs, EDGE_SETS)
            assert e.value.code == L.ANX_EINVAL
        finally:
            A.set_switch("ANX_CONFUSABLES", None)


# ---- the call and its neighbours ------------------------------------------------------------------------------------------------------
def test_no_side_effects(eng):
    g, _o, _words, _side, pairs, _expected = eng
    a, b = [x for x, _ in pairs[:100]], [y for _, y in pairs[:100]]
    P = product_params(EDGE_SETS[0])
    before = g.find_variants_ids(a, P)
    rec_before = g.evaluate_arrays(a, b, P)
    t0 = small_stats()
    _sums, got_pairs = sweep(g, pairs[:100], EDGE_SETS, with_pairs=True)
    assert small_stats() == t0
    assert g.find_variants_ids(a, P) == before
    assert g.evaluate_arrays(a, b, P).tobytes() == rec_before.tobytes()
    cols = g.score_pairs_arrays(a, b)
    for k in A.VariantModel.PAIR_KEYS:
        assert got_pairs[k].tobytes() == cols[k].tobytes(), k
    assert not got_pairs["_pad"].any()


def test_cli_sweep(hand, data_dir, tmp_path, capsys):
    _g, _side, lex, pairs, _Ps, expected = hand
    want = reduced(expected[:2])
    inp = tmp_path / "pairs.tsv"
    inp.write_text("".join("%s\t%s\n" % p for p in pairs))
    grid = tmp_path / "grid.tsv"
    grid.write_text("s\n0\n1\n")   # hand_params() and hand_params(stop_at_exact_match=True); everything else from the command line
    summary = tmp_path / "summary.json"
    argv = ["sweep", "-a", os.path.join(data_dir, "simple.alphabet.tsv"), "-l", lex, "-k", "2", "-d", "1", "-n", "3", "-t", "0.71", "-T", "0", "--device", "0",
            "--grid", str(grid), "--summary-json", str(summary), str(inp)]
    assert cli.main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2
    n = len(pairs)
    for s, (line, e) in enumerate(zip(lines, want)):
        cells = line.split("\t")
        assert cells[:7] == ["2", "1", "3", "0.71", "0", str(s), "0"]
        assert cells[7] == str(n) and cells[8] == cli.rust_f64(e["rank_hist"][0] / n) and cells[9] == cli.rust_f64(e["rr_fixed"] / 2.0 ** 32 / n)
        assert cells[10] == cli.rust_f64(e["reasons"][E.RANKED] / n) and cells[11:19] == [str(x) for x in e["reasons"]]
        assert cells[19:] == [str(e["gained_at_1"]), str(e["lost_at_1"]), cli.rust_f64(e["n_results"] / n)]
    js = json.loads(summary.read_text())
    assert [j["params"]["s"] for j in js] == ["0", "1"]
    for j, e in zip(js, want):
        assert j["n"] == n and j["reasons"] == dict(zip(E.REASONS, e["reasons"])) and j["rank_hist"] == e["rank_hist"]
        assert (j["n_results"], j["gained_at_1"], j["lost_at_1"]) == (e["n_results"], e["gained_at_1"], e["lost_at_1"])
