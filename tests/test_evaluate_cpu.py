"""anx_evaluate_gold without a GPU: the C ABI and its Python layers exist and agree, the call refuses to run without a device, the
command line knows `evaluate`, evaluate_summary counts what it should, the oracle-side helper (tests/eval_twin.py) gives every reason on
the hand-made model, and the new kernels' gfx950 ISA metadata holds what DESIGN.md section 5 states (no scratch, no LDS, full occupancy)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli
from oracle import cwrap as O
from oracle import twin as T

import eval_twin as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "analiticcl_amd", "csrc")
NAMES = ("anx_evaluate_gold", "anx_evaluate_gold_packed", "anx_debug_evaluate_gold_chunk")


def oracle_params(p):
    return O.make_params(p.max_anagram_distance, p.max_edit_distance, p.max_matches, p.score_threshold, p.cutoff_threshold,
                         p.stop_at_exact_match, p.freq_weight)


def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "anx.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert hasattr(lib, n), n
    for i, name in enumerate(E.REASONS):
        assert re.search(r"\bANX_GOLD_%s = %d\b" % (name, i), hdr), name
    assert L.GOLD_REASONS == E.REASONS
    assert L.lib().anx_abi_version() == L.ABI_VERSION == 3


def test_record_layout():
    hdr = open(os.path.join(REPO, "include", "anx.h")).read()
    assert "static_assert(sizeof(anx_gold_eval) == 32" in hdr
    assert C.sizeof(L.GoldEval) == 32 == np.dtype(A.VariantModel.GOLD_DTYPE).itemsize
    dt = np.dtype(A.VariantModel.GOLD_DTYPE)
    for name, _t in L.GoldEval._fields_:
        assert dt.fields[name][1] == getattr(L.GoldEval, name).offset, name
    assert np.dtype(A.VariantModel.PAIR_DTYPE).itemsize == C.sizeof(L.PairScore) == 24
    # the record as a C compiler lays it out, and the header as plain C
    src = '#include "anx.h"\n#include <stddef.h>\nint a[sizeof(anx_gold_eval) == 32 ? 1 : -1]; int b[offsetof(anx_gold_eval, gold_score) == 16 ? 1 : -1];' \
          ' int c[offsetof(anx_gold_eval, reason) == 29 ? 1 : -1];\n'
    subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(REPO, "include"), "-x", "c", "-"], input=src.encode(), check=True)


def hand_model_no_device(tmp_path):
    alphabet = os.path.join(REPO, "tests", "golden", "data", "simple_alphabet.tsv")
    lex = tmp_path / "hand.lexicon"
    lex.write_text("\n".join(E.HAND_WORDS) + "\n")
    m = A.VariantModel(alphabet, A.Weights(), device=-1)   # host only: never resident on a device
    m.read_lexicon(str(lex))
    return m


def test_no_device_is_an_error(tmp_path):
    m = hand_model_no_device(tmp_path)
    p = A.SearchParameters(max_anagram_distance=2, max_edit_distance=1, max_matches=3)
    with pytest.raises(A.AnxError) as e:   # before build()
        m.evaluate_arrays(["abcdef"], ["abcdeg"], p)
    assert e.value.code == L.ANX_ENOTBUILT
    m.build()
    for kw in ({}, {"packed": False}, {"chunk": 1}):
        with pytest.raises(A.AnxError) as e:
            m.evaluate_arrays(["abcdef"], ["abcdeg"], p, **kw)
        assert e.value.code == L.ANX_ENODEVICE
    assert len(m.evaluate_arrays([], [], p)) == 0   # n == 0 needs nothing
    with pytest.raises(ValueError):
        m.evaluate_arrays(["a"], [], p)
    out = (L.GoldEval * 1)()
    cp = p._c()
    assert L.lib().anx_evaluate_gold(m.h, None, None, 1, C.byref(cp), out, None) == L.ANX_EINVAL
    assert L.lib().anx_evaluate_gold_packed(m.h, b"a\0", 2, b"b\0", 2, 1, None, out, None) == L.ANX_EINVAL


def test_cli_parses_evaluate_with_querys_options():
    p = cli.build_parser()
    common = ["-a", "a.tsv", "-l", "l.tsv", "-k", "2", "-d", "0.3;2", "-n", "5", "-t", "0.3", "-T", "1.5", "-s", "-C", "c.tsv", "--early-confusables",
              "-V", "v.tsv", "--devices", "0,1", "--batch-size", "7"]
    q = p.parse_intermixed_args(["query"] + common)
    e = p.parse_intermixed_args(["evaluate"] + common + ["--summary-json", "s.json", "pairs.tsv"])
    assert e.mode == "evaluate" and e.summary_json == "s.json" and e.files == ["pairs.tsv"]
    for k, v in vars(q).items():
        if k not in ("mode", "files", "summary_json"):
            assert getattr(e, k) == v, k
    r = {"rank": 2, "gold_score": 0.75, "ld": 1, "reason": "RANKED"}
    assert cli.evaluate_tsv_line("abcdef", "xbcdef", r, "abcdef") == "abcdef\txbcdef\t3\tabcdef\t0.75\t1\tRANKED"
    r = {"rank": None, "gold_score": 0.0, "ld": 0, "reason": "STATUS"}
    assert cli.evaluate_tsv_line("abcdef", "", r, "") == "abcdef\t\t-\t\t0\t0\tSTATUS"


def test_evaluate_summary_on_hand_written_records():
    rec = np.zeros(8, dtype=np.dtype(A.VariantModel.GOLD_DTYPE))
    rec["rank"] = [0, 0, 1, 3, -1, -1, -1, -1]
    rec["reason"] = [E.RANKED, E.RANKED, E.RANKED, E.RANKED, E.ANAGRAM, E.NOT_A_RESULT, E.CROPPED, E.ANAGRAM]
    rec["gold_vocab_id"] = [5, 6, 7, 8, 9, 0xFFFFFFFF, 10, 11]
    s = A.VariantModel.evaluate_summary(rec)
    assert s["n"] == 8 and s["gold_known"] == 7
    assert s["accuracy_at_1"] == 2 / 8 and s["ranked_share"] == 4 / 8
    assert s["mrr"] == (1.0 + 1.0 + 0.5 + 0.25) / 8
    assert s["reasons"] == {"RANKED": 4, "STATUS": 0, "NOT_A_RESULT": 1, "EXACT_STOP": 0, "ANAGRAM": 2, "EDIT": 0, "THRESHOLD": 0, "CROPPED": 1}
    assert list(s["reasons"]) == list(E.REASONS)
    z = A.VariantModel.evaluate_summary(rec[:0])
    assert z["n"] == 0 and z["mrr"] == 0.0 and sum(z["reasons"].values()) == 0
    assert "accuracy@1: 0.25\n" in cli.evaluate_summary_text(s) and "ANAGRAM: 2\n" in cli.evaluate_summary_text(s)


@pytest.fixture(scope="module")
def hand_sides():
    alphabet = os.path.join(REPO, "tests", "golden", "data", "simple_alphabet.tsv")
    tw = T.VariantModel(T.read_alphabet(alphabet))
    o = O.OracleModel(alphabet_path=alphabet)
    for w in E.HAND_WORDS:
        assert tw.add_to_vocabulary(w) == o.add(w)
    tw.build()
    o.build()
    rows = lambda text, P: o.find_variants_via(text, oracle_params(P))
    flags = lambda v: (tw.decoder[v].indexed, tw.decoder[v].transparent)
    return E.twin_side(tw, rows), E.oracle_side(o, tw.alphabet, tw.weights, tw.encoder, flags, oracle_params)


def test_helper_gives_every_reason_on_the_hand_made_model(hand_sides):
    """Pins the helper itself: the hand-made pairs give the reasons and ranks they were made for, all eight reasons occur, and the
    anagram stage of the C oracle (what the full-size GPU tests use) gives the records the twin's own stage gives."""
    twin_side, oracle_side = hand_sides
    seen = set()
    for P, pairs in ((E.hand_params(), E.HAND_PAIRS), (E.hand_params(stop_at_exact_match=True), E.HAND_PAIRS_STOP)):
        for a, g, reason, rank in pairs:
            r = E.expected_record(twin_side, a, g, P)
            assert (r["reason"], r["rank"]) == (reason, rank), (a, g[:10], r)
            assert r == E.expected_record(oracle_side, a, g, P), (a, g[:10])
            seen.add(r["reason"])
    assert seen == set(range(8))
    r = E.expected_record(twin_side, "abcdef", "abcd", E.hand_params())
    assert (r["k"], r["d"], r["ld"], r["status"], r["n_results"], r["gold_vocab_id"]) == (2, 1, 2, 0, 3, 3 + E.HAND_WORDS.index("abcd"))
    assert r["gold_score"] == 0.625 and r["top_vocab_id"] == 3
    r = E.expected_record(twin_side, "abcdef", "<unk>", E.hand_params())
    assert r["gold_vocab_id"] == 2 and r["reason"] == E.NOT_A_RESULT
    r = E.expected_record(twin_side, "abcdef", "a" * 256, E.hand_params())
    assert (r["status"], r["ld"], r["gold_score"], r["gold_vocab_id"]) == (E.ELIMIT, 0, 0.0, E.NONE)
    r = E.expected_record(twin_side, "", "abcdef", E.hand_params())
    assert (r["status"], r["k"], r["d"], r["n_results"], r["top_vocab_id"]) == (E.EEMPTY, 0, 0, 0, E.NONE)


def test_edited_pairs_are_seeded():
    words = ["separate", "receive", "definitely", "their", "occurrence", "necessary"]
    a, b = E.edited_pairs(words, 50, seed=5), E.edited_pairs(words, 50, seed=5)
    assert a == b and a != E.edited_pairs(words, 50, seed=6)
    assert all(g in words and q for q, g in a)


KEYS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


def test_eval_kernels_isa_metadata(tmp_path):
    """DESIGN.md section 5 "Gold evaluation": none of the four kernels uses scratch or LDS or spills, every one stays at or below 64
    VGPRs (eight waves per SIMD), k_eval_classify computes L1 with v_sad_u8 and writes the record as two 16-byte stores."""
    out = str(tmp_path / "eval.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                           "--cuda-device-only", "-o", out, os.path.join(CSRC, "eval.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        ks[m.group(2)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(3)).group(1)) for k in KEYS}
        ks[m.group(2)]["group_segment_fixed_size"] = int(m.group(1))
    for kernel in ("k_eval_sections", "k_eval_lookup", "k_eval_rows", "k_eval_classify"):
        r = [v for n, v in ks.items() if kernel in n]
        assert len(r) == 1, (kernel, sorted(ks))
        assert r[0]["vgpr_spill_count"] == 0 and r[0]["sgpr_spill_count"] == 0 and r[0]["private_segment_fixed_size"] == 0, (kernel, r[0])
        assert r[0]["group_segment_fixed_size"] == 0 and r[0]["vgpr_count"] <= 64, (kernel, r[0])
    body = text[text.index("k_eval_classify"):]
    body = body[:body.index("s_endpgm")]
    assert "v_sad_u8" in body and body.count("global_store_dwordx4") == 2
