"""The device fold of learn mode (learn.hip) on rows natural queries do not produce: every case of tests/learn_cases.py through the test
hook anx_debug_learn_fold_rows against the restatement of the reference's loop (tests/learn_twin.py) and against the host fold, with
the string hash narrowed (ANX_LEARN_HASH_BITS: collisions), over several export sections (contiguous and index-listed), without rows;
and learn_variants end to end with more than one row per input, several gather rounds, replicas and both shard policies.

Every comparison is equality of the count and of the whole state: per entry text, frequency, vocabulary type, lexicon index and the
(kind, id, score) links in order, the scores being the f64 values that went in."""
import functools
import os

import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import synth
from oracle import cwrap as O
from oracle import twin as T

import learn_cases as LC
import learn_twin as LT

CASES = LC.all_cases(seeds=(1,))
HASH_BITS = (63, 8, 3, 1)  # 1 bit: every unknown string in one of two hash runs, the vocabulary table one long probe chain


def _alpha(data_dir):
    return os.path.join(data_dir, "simple.alphabet.tsv")


def _fold_case(data_dir, tmp_path, case, kind, n_sections=1, by_index=False):
    """One case, call after call, through the device fold (g), the host fold (h) and the restatement (m)."""
    g, m = LC.build_models(_alpha(data_dir), tmp_path, kind, device=0)
    h, _ = LC.build_models(_alpha(data_dir), tmp_path, kind)
    ncalls = 0
    for inputs, rows in case.calls(m):
        before = A.VariantModel.learn_stats()
        ns = n_sections if n_sections > 0 else len(inputs) + 2
        c = g.learn_fold_rows_device(inputs, rows, n_sections=ns, by_index=by_index)
        after = A.VariantModel.learn_stats()
        assert after["device_folds"] == before["device_folds"] + 1 and after["host_folds"] == before["host_folds"]
        assert c == LT.learn_fold(m, inputs, rows)
        assert c == h.learn_apply_rows(inputs, rows)
        LT.assert_same_state(g, m)
        assert LT.product_state(g) == LT.product_state(h)
        ncalls += 1
    assert ncalls >= 2


@pytest.mark.parametrize("bits", HASH_BITS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_device_fold_cases(data_dir, tmp_path, case, bits):
    """Every generated case; the outcome may not depend on how many bits of the string hash are kept (a collision must neither merge
    two strings nor hide a vocabulary entry)."""
    L.set_switch("ANX_LEARN_HASH_BITS", bits)
    try:
        _fold_case(data_dir, tmp_path, case, "variants" if bits in (63, 3) else "plain")
        if bits == 63:  # (the other kind of model once, under the production hash)
            _fold_case(data_dir, tmp_path, case, "plain")
    finally:
        L.set_switch("ANX_LEARN_HASH_BITS", None)


def test_hash_bits_switch_rebuilds_the_table(data_dir, tmp_path):
    """One model, the switch changed between calls with the vocabulary size unchanged (a call without new strings): the cached
    table must follow, or known strings would be looked up under the wrong hash and entered twice."""
    g, m = LC.build_models(_alpha(data_dir), tmp_path, "variants", device=0)
    inputs = ["house", "mouse", "the", "house", "naïve", LC.LONG[:64]]
    rows = [[(m.encoder["hose"], 0.5)], [(m.encoder["house"], 0.25)], [(m.encoder["them"], 0.125)], [], [(m.encoder["é"], 0.75)],
            [(m.encoder[LC.LONG[:65]], 0.0625)]]
    try:
        for bits in (63, 5, 63, 1, 40):
            L.set_switch("ANX_LEARN_HASH_BITS", bits)
            V = g.vocab_size()
            assert g.learn_fold_rows_device(inputs, rows) == LT.learn_fold(m, inputs, rows)
            assert g.vocab_size() == V
            LT.assert_same_state(g, m)
    finally:
        L.set_switch("ANX_LEARN_HASH_BITS", None)


SECTION_CASES = [c for c in CASES if c.name in ("runs_across_block_borders", "second_call", "duplicate_pairs", "random_n2_s1", "random_n257_s1",
                                                "random_n5000_s1")]


@pytest.mark.parametrize("layout", [(1, False), (3, False), (7, False), (0, False), (3, True), (7, True)],
                         ids=["1", "3", "7", "n+2", "3_by_index", "7_by_index"])
@pytest.mark.parametrize("case", SECTION_CASES, ids=repr)
def test_device_fold_sections(data_dir, tmp_path, case, layout):
    """The same rows in 1, 3, 7 and n + 2 contiguous sections (lo > 0, empty sections) and in 3 and 7 index-listed ones (neighbouring
    inputs in different sections): each equals the restatement, hence all are identical."""
    assert len(SECTION_CASES) == 6
    _fold_case(data_dir, tmp_path, case, "variants", n_sections=layout[0], by_index=layout[1])


@pytest.mark.parametrize("bits", (63, 1))
def test_device_fold_without_rows(data_dir, tmp_path, bits):
    """R == 0 (sorts, scans and emit kernels over nothing) and n == 0: count 0, state unchanged, no error."""
    L.set_switch("ANX_LEARN_HASH_BITS", bits)
    try:
        g, m = LC.build_models(_alpha(data_dir), tmp_path, "variants", device=0)
        s0 = LT.product_state(g)
        for inputs in ([], ["house"], ["", "unknown"], ["house", "nowhere", "", "house"] * 200):
            for ns, by_index in ((1, False), (3, False), (3, True), (len(inputs) + 2, False)):
                assert g.learn_fold_rows_device(inputs, [[] for _ in inputs], n_sections=ns, by_index=by_index) == 0
                assert LT.product_state(g) == s0
        LT.assert_same_state(g, m)
        # ... and the model still folds afterwards
        inputs, rows = ["hous"], [[(m.encoder["house"], 0.5)]]
        assert g.learn_fold_rows_device(inputs, rows) == LT.learn_fold(m, inputs, rows) == 1
        LT.assert_same_state(g, m)
    finally:
        L.set_switch("ANX_LEARN_HASH_BITS", None)


def test_device_fold_rejects_bad_ids(data_dir, tmp_path):
    g, m = LC.build_models(_alpha(data_dir), tmp_path, "plain", device=0)
    for call in (g.learn_apply_rows, g.learn_fold_rows_device):
        with pytest.raises(A.AnxError) as e:
            call(["huis", "hous"], [[(3, 0.5)], [(4, 0.5), (g.vocab_size(), 0.5)]])
        assert e.value.code == L.ANX_EINVAL
    LT.assert_same_state(g, m)


# ---- end to end: learn_variants(strict) on eng.aspell ---------------------------------------------------------------------------------
def _paths(data_dir):
    return _alpha(data_dir), os.path.join(data_dir, "eng.aspell.lexicon")


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


def _params(max_matches):
    return A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=max_matches)


@functools.lru_cache(maxsize=None)
def _inputs(data_dir):
    """Natural queries with the empty string, row-less garbage and deliberate repeats (adjacent, across a row-less input, distant)."""
    words = synth.load_lexicon_words(_paths(data_dir)[1])
    qs = synth.make_queries(words, 2964, max_len=16, seed=77)
    special = ["seperate", "seperate", "", "seperate", "xqzxqzxqzjjj", "recieve", "xqzxqzxqzjjj", "recieve", "horse", "seperate", ""]
    qs = qs[:255] + special[:4] + qs[255:1500] + special[4:] + qs[1500:] + ["recieve", "", "seperate", "horse", "horse"] + qs[100:120]
    assert len(qs) == 3000
    return tuple(qs)


@functools.lru_cache(maxsize=None)
def _oracle_rows(data_dir, max_matches):
    alpha, lex = _paths(data_dir)
    o = O.OracleModel(alphabet_path=alpha)
    o.read_lexicon(lex)
    o.build()
    qs = list(_inputs(data_dir))
    # (the reference's find_variants asserts a non-empty input and the oracle refuses it; the product gives "" no rows)
    some = [q for q in qs if q]
    counts, vid, dist, _f, _, _ = O.batch_rows(o, some, O.make_params(("abs", 3), ("abs", 2), max_matches, 0.25, 2.0), stride=16)
    it = iter([[(int(vid[i, k]), float(dist[i, k])) for k in range(int(counts[i]))] for i in range(len(some))])
    rows = [next(it) if q else [] for q in qs]
    assert qs.count("") == 3 and rows[qs.index("xqzxqzxqzjjj")] == [] and max(len(r) for r in rows) == max_matches
    assert sum(len(r) > 1 for r in rows) > len(rows) // 4
    return rows


@functools.lru_cache(maxsize=None)
def _reference_run(data_dir, max_matches):
    """One gather round on one replica, against the restatement over the C oracle's rows; a second iteration on the rebuilt model
    against the restatement over the product's own rows.  -> (count, state) of the first iteration."""
    qs = list(_inputs(data_dir))
    g = _product(data_dir, device=0)
    m = _twin(data_dir)
    before = A.VariantModel.learn_stats()
    c1 = g.learn_variants(qs, _params(max_matches))
    assert A.VariantModel.learn_stats()["device_folds"] == before["device_folds"] + 1
    assert c1 == LT.learn_fold(m, qs, _oracle_rows(data_dir, max_matches)) and c1 > len(qs)
    LT.assert_same_state(g, m)
    s1 = LT.product_state(g)
    rows2 = [[(v, d) for v, d, _f in r] for r in g.find_variants_ids(qs, _params(max_matches))]
    c2 = g.learn_variants(qs, _params(max_matches), auto_build=False)
    assert A.VariantModel.learn_stats()["device_folds"] == before["device_folds"] + 2
    assert c2 == LT.learn_fold(m, qs, rows2) and c2 > 0
    LT.assert_same_state(g, m)
    assert m.decoder[m.encoder["seperate"]].frequency == 2 * 3  # (three runs per call: the second call finds it known)
    return c1, s1


@pytest.mark.parametrize("max_matches", (3, 10))
def test_learn_strict_many_rows_per_input(data_dir, max_matches):
    _reference_run(data_dir, max_matches)


@pytest.mark.parametrize("policy", ("length", "range"))
@pytest.mark.parametrize("replicas", (1, 3))
@pytest.mark.parametrize("max_matches", (3, 10))
def test_learn_strict_gather_rounds(data_dir, max_matches, replicas, policy):
    """ANX_MAX_BATCH lowered: the call takes four gather rounds or more (sections with lo > 0; under the length policy index-listed
    ones rebased by the round's first input), on one replica and on three: the count and state of the single-round call."""
    qs = list(_inputs(data_dir))
    c1, s1 = _reference_run(data_dir, max_matches)
    max_batch = 250
    assert -(-len(qs) // (max_batch * replicas)) >= 4
    A.set_switch("ANX_MAX_BATCH", max_batch)
    A.set_switch("ANX_SHARD_MIN", 64)
    A.set_switch("ANX_SHARD_POLICY", policy)
    try:
        g = _product(data_dir, device=0) if replicas == 1 else _product(data_dir, devices=[0] * replicas)
        assert g.num_replicas == replicas
        before = A.VariantModel.learn_stats()
        assert g.learn_variants(qs, _params(max_matches), auto_build=False) == c1
        assert A.VariantModel.learn_stats()["device_folds"] == before["device_folds"] + 1
        assert LT.product_state(g) == s1
    finally:
        A.set_switch("ANX_MAX_BATCH", None)
        A.set_switch("ANX_SHARD_MIN", None)
        A.set_switch("ANX_SHARD_POLICY", None)
