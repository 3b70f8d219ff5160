"""anx_score_pairs / anx_score_pairs_packed without a device: the symbols are there, the argument checks answer before anything
touches the GPU, the ctypes struct has the C layout, and the `score` subcommand parses and formats."""
import ctypes as C

import pytest

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli

ALPHABET_TSV = "\n".join(f"{c}\t{c.upper()}" for c in "abcdefghijklmnopqrstuvwxyz") + "\n"


@pytest.fixture(scope="module")
def host_model():
    m = A.VariantModel("", alphabet_text=ALPHABET_TSV, device=-1)
    m.add_to_vocabulary("huis")
    return m


def _args(pairs):
    a = (C.c_char_p * len(pairs))(*[x.encode() for x, _ in pairs])
    b = (C.c_char_p * len(pairs))(*[y.encode() for _, y in pairs])
    return a, b, (L.PairScore * len(pairs))()


def test_symbols_exported_and_struct_layout():
    lib = C.CDLL(L.LIB_PATH)
    assert hasattr(lib, "anx_score_pairs") and hasattr(lib, "anx_score_pairs_packed")
    assert C.sizeof(L.PairScore) == 24
    assert [(n, getattr(L.PairScore, n).offset) for n, _ in L.PairScore._fields_] == [
        ("score", 0), ("ld", 8), ("lcs", 10), ("prefixlen", 12), ("suffixlen", 14), ("len_a", 16), ("len_b", 17), ("samecase", 18),
        ("status", 19), ("_pad", 20)]
    assert L.lib().anx_abi_version() == 3  # the addition is additive


def test_argument_checks_come_first(host_model):
    lib = L.lib()
    a, b, out = _args([("huys", "huis")])
    # n = 0 is answered before the model's state matters
    assert lib.anx_score_pairs(host_model.h, None, None, 0, None) == L.ANX_OK
    assert lib.anx_score_pairs_packed(host_model.h, None, 0, None, 0, 0, None) == L.ANX_OK
    # NULL arguments
    assert lib.anx_score_pairs(None, a, b, 1, out) == L.ANX_EINVAL
    assert lib.anx_score_pairs(host_model.h, None, b, 1, out) == L.ANX_EINVAL
    assert lib.anx_score_pairs(host_model.h, a, None, 1, out) == L.ANX_EINVAL
    assert lib.anx_score_pairs(host_model.h, a, b, 1, None) == L.ANX_EINVAL
    assert lib.anx_score_pairs_packed(host_model.h, None, 5, b"huis\0", 5, 1, out) == L.ANX_EINVAL
    assert lib.anx_score_pairs_packed(host_model.h, b"huys\0", 5, b"huis\0", 5, 1, None) == L.ANX_EINVAL
    assert lib.anx_last_error_code() == L.ANX_EINVAL


def test_unbuilt_then_no_device():
    m = A.VariantModel("", alphabet_text=ALPHABET_TSV, device=-1)
    m.add_to_vocabulary("huis")
    lib = L.lib()
    a, b, out = _args([("huys", "huis")])
    assert lib.anx_score_pairs(m.h, a, b, 1, out) == L.ANX_ENOTBUILT
    m.build()
    # built but not resident on a device (device=-1): there is no CPU path, with or without a GPU in the machine
    assert lib.anx_score_pairs(m.h, a, b, 1, out) == L.ANX_ENODEVICE
    assert lib.anx_score_pairs_packed(m.h, b"huys\0", 5, b"huis\0", 5, 1, out) == L.ANX_ENODEVICE
    with pytest.raises(A.AnxError) as e:
        m.score_pairs(["huys"], ["huis"])
    assert e.value.code == L.ANX_ENODEVICE
    with pytest.raises(ValueError):
        m.score_pairs(["a", "b"], ["a"])
    assert m.score_pairs([], []) == []


def test_score_subcommand_parses_and_formats():
    p = cli.build_parser()
    a = p.parse_intermixed_args(["score", "--alphabet", "a.tsv", "--lexicon", "l.tsv", "--weight-ld", "1", "--weight-lcs", "0", "--weight-prefix",
                                 "0.5", "--weight-suffix", "0", "--weight-case", "0", "--device", "0", "--json", "pairs.tsv"])
    assert a.mode == "score" and a.files == ["pairs.tsv"] and a.json and a.device == 0
    assert (a.weight_ld, a.weight_lcs, a.weight_prefix, a.weight_suffix, a.weight_case) == (1.0, 0.0, 0.5, 0.0, 0.0)
    ok = {"score": 0.734375, "ld": 1, "lcs": 4, "prefixlen": 3, "suffixlen": 4, "samecase": True, "len_a": 8, "len_b": 8, "status": 0}
    empty = dict(ok, status=L.ANX_EEMPTY, score=0.0)
    assert cli.score_tsv_line("seperate", "separate", ok) == "seperate\tseparate\t0.734375\t1\t4\t3\t4\t1"
    assert cli.score_tsv_line("x", "", empty) == "x\t\t\t\t\t\t\t"
    assert cli.score_tsv_line("x", "", empty).count("\t") == cli.score_tsv_line("a", "b", ok).count("\t")
    assert cli.score_json_item('se"p', "sep", ok, 2) == ('    ,{ "a": "se\\"p", "b": "sep", "score": 0.734375, "ld": 1, "lcs": 4, "prefix": 3, '
                                                        '"suffix": 4, "samecase": true }\n')
    assert cli.score_json_item("x", "", empty, 1) == '    { "a": "x", "b": "", "status": -6 }\n'
