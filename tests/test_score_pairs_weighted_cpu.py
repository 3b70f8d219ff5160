"""anx_score_pairs_weighted / anx_model_confusable_weight_text / anx_debug_pairs_conf_stats without a device: the exports, the
argument checks (which answer before the model's state matters), the host function for two strings against
oracle/confusable_oracle.py (src/lib.rs:1733-1756 over oracle/sesdiff_twin.py) with `==`, and the `score --weighted` formats."""
import ctypes as C
import json

import pytest

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli
from oracle import confusable_oracle as CO
import pairs_conf_common as PC

TEST_ALPHABET_TSV = "\n".join(f"{c}\t{c.upper()}" for c in "abcdefghijklmnopqrstuvwxyz") + "\n"


@pytest.fixture(scope="module")
def host_model():
    m = A.VariantModel("", alphabet_text=TEST_ALPHABET_TSV, device=-1)
    PC.load_patterns(m)
    return m


def test_symbols_and_abi():
    lib = C.CDLL(L.LIB_PATH)
    for n in ("anx_score_pairs_weighted", "anx_score_pairs_weighted_packed", "anx_model_confusable_weight_text", "anx_debug_pairs_conf_stats"):
        assert hasattr(lib, n), n
    assert L.lib().anx_abi_version() == L.ABI_VERSION == 3
    st = A.VariantModel.pairs_conf_stats()
    assert set(st) == {"pairs", "screened", "device_scripts", "host_pairs"}
    assert L.lib().anx_debug_pairs_conf_stats(None) == L.ANX_EINVAL


def test_argument_checks_come_before_the_model_state():
    m = A.VariantModel("", alphabet_text=TEST_ALPHABET_TSV, device=-1)
    m.add_to_vocabulary("huis")
    lib = L.lib()
    a = (C.c_char_p * 1)(b"huys")
    b = (C.c_char_p * 1)(b"huis")
    out = (L.PairScore * 1)()
    w = (C.c_double * 1)()
    # not built, no device: n == 0 and the NULL checks answer first
    assert lib.anx_score_pairs_weighted(m.h, a, b, 0, out, w) == L.ANX_OK
    assert lib.anx_score_pairs_weighted(m.h, None, None, 0, None, None) == L.ANX_OK
    assert lib.anx_score_pairs_weighted_packed(m.h, None, 0, None, 0, 0, None, None) == L.ANX_OK
    assert lib.anx_score_pairs_weighted(None, a, b, 1, out, w) == L.ANX_EINVAL
    assert lib.anx_score_pairs_weighted(m.h, None, b, 1, out, w) == L.ANX_EINVAL
    assert lib.anx_score_pairs_weighted(m.h, a, None, 1, out, w) == L.ANX_EINVAL
    assert lib.anx_score_pairs_weighted(m.h, a, b, 1, None, w) == L.ANX_EINVAL
    assert lib.anx_score_pairs_weighted(m.h, a, b, 1, out, None) == L.ANX_EINVAL
    assert lib.anx_score_pairs_weighted_packed(m.h, None, 5, b"huis\0", 5, 1, out, w) == L.ANX_EINVAL
    assert lib.anx_score_pairs_weighted_packed(m.h, b"huys\0", 5, None, 5, 1, out, w) == L.ANX_EINVAL
    assert lib.anx_score_pairs_weighted_packed(m.h, b"huys\0", 5, b"huis\0", 5, 1, None, w) == L.ANX_EINVAL
    assert lib.anx_score_pairs_weighted_packed(m.h, b"huys\0", 5, b"huis\0", 5, 1, out, None) == L.ANX_EINVAL
    # then the model's state: not built, then not resident
    assert lib.anx_score_pairs_weighted(m.h, a, b, 1, out, w) == L.ANX_ENOTBUILT
    assert lib.anx_score_pairs_weighted_packed(m.h, b"huys\0", 5, b"huis\0", 5, 1, out, w) == L.ANX_ENOTBUILT
    m.build()
    assert lib.anx_score_pairs_weighted(m.h, a, b, 1, out, w) == L.ANX_ENODEVICE
    assert lib.anx_score_pairs_weighted_packed(m.h, b"huys\0", 5, b"huis\0", 5, 1, out, w) == L.ANX_ENODEVICE
    with pytest.raises(A.AnxError) as e:
        m.score_pairs(["huys"], ["huis"], weighted=True)
    assert e.value.code == L.ANX_ENODEVICE
    # the host function's own checks
    d = C.c_double()
    assert lib.anx_model_confusable_weight_text(m.h, None, b"x", C.byref(d)) == L.ANX_EINVAL
    assert lib.anx_model_confusable_weight_text(m.h, b"x", None, C.byref(d)) == L.ANX_EINVAL
    assert lib.anx_model_confusable_weight_text(m.h, b"x", b"y", None) == L.ANX_EINVAL
    assert lib.anx_model_confusable_weight_text(None, b"x", b"y", C.byref(d)) == L.ANX_EINVAL
    assert m.confusable_weight_text("huys", "huis") == 1.0  # no confusables in this model


def test_hand_made_pairs_equal_the_oracle(host_model):
    pats = PC.oracle_patterns()
    assert len(pats) == 14
    fired = set()
    for a, b, w in PC.HAND:
        assert CO.confusable_weight(pats, a, b) == w, (a, b)
        assert host_model.confusable_weight_text(a, b) == w, (a, b)
        for j, p in enumerate(pats):
            if CO.confusable_weight([p], a, b) != 1.0:
                fired.add(j)
    # both directions, as the device test runs them
    for a, b, _ in PC.HAND:
        assert host_model.confusable_weight_text(b, a) == CO.confusable_weight(pats, b, a), (b, a)
    assert len([j for j in fired if j < 10]) >= 8, sorted(fired)
    assert {10, 11, 12, 13} <= fired, sorted(fired)


def test_random_pairs_equal_the_oracle(host_model):
    pats = PC.oracle_patterns()
    pairs = PC.small_alphabet_pairs(20000)
    exp = PC.oracle_weights(pats, pairs)
    assert sum(1 for w in exp if w != 1.0) >= 400
    for (a, b), w in zip(pairs, exp):
        assert host_model.confusable_weight_text(a, b) == w, (a, b)


def test_vocabulary_items_equal_the_id_form():
    m = A.VariantModel("", alphabet_text=TEST_ALPHABET_TSV, device=-1)
    PC.load_patterns(m)
    words = ["huis", "kat", "zien", "see", "cirkel", "hebbe", "eer", "vrÿheid", "stad", "geloof", "vrouw", "akte"]
    ids = [m.add_to_vocabulary(w) for w in words]
    inputs = [a for a, _, _ in PC.HAND] + ["huys", "cirkel", "vrouuu"]
    hits = 0
    for q in inputs:
        for w, i in zip(words, ids):
            x = m.confusable_weight_text(q, w)
            assert x == m.compute_confusable_weight(q, i), (q, w)
            hits += x != 1.0
    assert hits >= 10


def test_score_weighted_formats():
    p = cli.build_parser()
    assert p.parse_intermixed_args(["score", "-a", "x", "--weighted", "f.tsv"]).weighted is True
    assert p.parse_intermixed_args(["score", "-a", "x", "f.tsv"]).weighted is False
    assert p.parse_intermixed_args(["score", "-a", "x", "--confusables", "c.tsv", "f.tsv"]).weighted is False
    r = {"score": 0.734375, "ld": 1, "lcs": 2, "prefixlen": 2, "suffixlen": 1, "samecase": True, "len_a": 4, "len_b": 4, "status": 0}
    old_tsv = "huys\thuis\t0.734375\t1\t2\t2\t1\t1"
    old_json = '    { "a": "huys", "b": "huis", "score": 0.734375, "ld": 1, "lcs": 2, "prefix": 2, "suffix": 1, "samecase": true }\n'
    assert cli.score_tsv_line("huys", "huis", r) == old_tsv
    assert cli.score_json_item("huys", "huis", r, 1) == old_json
    rw = dict(r, weight=1.1, weighted_score=0.734375 * 1.1)
    line = cli.score_tsv_line("huys", "huis", rw)
    assert line == old_tsv + "\t1.1\t" + cli.rust_f64(0.734375 * 1.1)
    assert len(line.split("\t")) == 10
    item = json.loads(cli.score_json_item("huys", "huis", rw, 2).lstrip(" ,"))
    assert item["weight"] == 1.1 and item["weighted_score"] == 0.734375 * 1.1 and item["score"] == 0.734375
    assert list(item)[-2:] == ["weight", "weighted_score"]
    # a pair with a status: empty columns, the status alone in JSON
    rs = {"score": 0.0, "ld": 0, "lcs": 0, "prefixlen": 0, "suffixlen": 0, "samecase": False, "len_a": 0, "len_b": 3, "status": L.ANX_EEMPTY}
    assert cli.score_tsv_line("", "abc", rs) == "\tabc\t\t\t\t\t\t"
    assert cli.score_tsv_line("", "abc", dict(rs, weight=1.0, weighted_score=0.0)) == "\tabc\t\t\t\t\t\t\t\t"
    assert json.loads(cli.score_json_item("", "abc", dict(rs, weight=1.0, weighted_score=0.0), 1)) == {"a": "", "b": "abc", "status": L.ANX_EEMPTY}
