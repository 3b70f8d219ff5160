"""anx_evaluate_sweep_confusables without a GPU: the C ABI and its Python layers exist, the call refuses what it must with a message
that says why (before the device is asked for), the empty call is answered before anything is counted, the command line builds the
one-pattern-on grid and names its limits, the host body of the mask kernel (confusables_core.hpp confusable_mask) agrees with
oracle/sesdiff_twin.py pattern by pattern and its product with anx_model_confusable_weight_text, and the gfx950 ISA metadata of
csweep.hip's kernels holds what DESIGN.md section 5 "Confusable sweep" states."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli

import eval_twin as E
import sweep_conf_common as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "analiticcl_amd", "csrc")
NAMES = ("anx_evaluate_sweep_confusables", "anx_evaluate_sweep_confusables_packed", "anx_debug_evaluate_sweep_confusables_chunk",
         "anx_debug_sweep_conf_masks", "anx_debug_conf_sweep_stats", "anx_debug_conf_mask_text")
ALPHABET = os.path.join(REPO, "tests", "golden", "data", "simple_alphabet.tsv")
STATS = ["calls", "chunks", "groups", "sets", "pair_passes", "batch_runs", "base_rows", "rows_listed", "rows_patched", "rows_host_mode", "bytes_down"]


def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "anx.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert hasattr(lib, n), n
    assert L.lib().anx_abi_version() == L.ABI_VERSION == 3
    version_comment = hdr[:hdr.index("#define ANX_ABI_VERSION")]
    assert "anx_evaluate_sweep_confusables" in version_comment
    subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(REPO, "include"), "-x", "c", "-"], input=b'#include "anx.h"\n', check=True)
    for name in ("evaluate_sweep_confusables", "evaluate_sweep_confusables_arrays", "conf_sweep_stats"):
        assert callable(getattr(A.VariantModel, name)), name


def hand_model_no_device(tmp_path, weights=None):
    lex = tmp_path / "hand.lexicon"
    lex.write_text("\n".join(E.HAND_WORDS) + "\n")
    m = A.VariantModel(ALPHABET, weights or A.Weights(), device=-1)   # host only: never resident on a device
    m.read_lexicon(str(lex))
    return m


def c_call(m, pats, sets, weights, n_sets, sums, a=(b"abcdef",), g=(b"abcdeg",), early=None, n_patterns=None, n=None):
    """the pointer form with ctypes arrays built here -> the return code"""
    aa, ag = (C.c_char_p * max(len(a), 1))(*a), (C.c_char_p * max(len(g), 1))(*g)
    pp = (C.c_char_p * max(len(pats), 1))(*pats)
    ws = (C.c_double * max(len(weights), 1))(*weights)
    return L.lib().anx_evaluate_sweep_confusables(m.h, aa, ag, len(a) if n is None else n, pp, len(pats) if n_patterns is None else n_patterns, sets, ws, early,
                                                  n_sets, sums, None)


def test_errors_and_the_empty_call(tmp_path):
    m = hand_model_no_device(tmp_path)
    p = A.SearchParameters(max_anagram_distance=2, max_edit_distance=1, max_matches=3)
    pats = ["-[y]+[i]", "+[e]"]
    with pytest.raises(A.AnxError) as e:   # before build()
        m.evaluate_sweep_confusables_arrays(["abcdef"], ["abcdeg"], pats, [p], [[1.0, 1.0]])
    assert e.value.code == L.ANX_ENOTBUILT
    m.build()
    for kw in ({}, {"packed": False}, {"chunk": 1}):   # the packed form, the pointer form, the chunk hook: a plain host-only model has no device
        with pytest.raises(A.AnxError) as e:
            m.evaluate_sweep_confusables_arrays(["abcdef"], ["abcdeg"], pats, [p, p], [[1.0, 1.0], [1.1, 0.9]], [False, True], **kw)
        assert e.value.code == L.ANX_ENODEVICE
    with pytest.raises(ValueError):
        m.evaluate_sweep_confusables_arrays(["a"], [], pats, [p], [[1.0, 1.0]])
    with pytest.raises(ValueError):   # lists of unequal length
        m.evaluate_sweep_confusables_arrays(["a"], ["a"], pats, [p, p], [[1.0, 1.0]])
    with pytest.raises(ValueError):   # a set without a weight per pattern
        m.evaluate_sweep_confusables_arrays(["a"], ["a"], pats, [p], [[1.0]])
    with pytest.raises(ValueError):
        m.evaluate_sweep_confusables_arrays(["a"], ["a"], pats, [p], [[1.0, 1.0]], [False, True])
    lib = L.lib()
    sets = (L.Params * 257)(*[p._c() for _ in range(257)])
    sums = (L.GoldSummary * 257)()
    bp = [x.encode() for x in pats]
    ones = [1.0] * (2 * 257)

    def refused(rc, *words):
        assert rc == L.ANX_EINVAL
        msg = L.last_error()
        assert all(w in msg for w in words), (msg, words)

    refused(c_call(m, bp, sets, ones, 0, sums), "sets", "256")
    refused(c_call(m, bp, sets, ones, 257, sums), "sets", "256")
    refused(c_call(m, bp, sets, ones, 1, sums, n_patterns=0), "patterns", "64")
    refused(c_call(m, [b"+[e]"] * 65, sets, [1.0] * 65, 1, sums), "patterns", "64")
    assert c_call(m, [b"+[e]"] * 64, sets, [1.0] * 64, 1, sums) == L.ANX_ENODEVICE   # 64 patterns are served
    for bad in (b"", b"+[e", b"x[e]", b"+[]", b"^$"):
        refused(c_call(m, [b"+[e]", bad], sets, ones, 1, sums), "pattern 1")
    for bad in (0.0, -1.1, math.nan, math.inf):
        for at in (0, 3):   # in any set of the list
            ws = [1.0] * 4
            ws[at] = bad
            refused(c_call(m, bp, sets, ws, 2, sums), "set %d" % (at // 2), "pattern %d" % (at % 2), "weight")
            refused(c_call(m, bp, sets, ws, 2, sums, a=(), g=(), n=0), "weight")
    aa, ag, pp, ws = (C.c_char_p * 1)(b"abcdef"), (C.c_char_p * 1)(b"abcdeg"), (C.c_char_p * 2)(*bp), (C.c_double * 4)(1, 1, 1, 1)
    f = lib.anx_evaluate_sweep_confusables
    assert f(None, aa, ag, 1, pp, 2, sets, ws, None, 1, sums, None) == L.ANX_EINVAL
    assert f(m.h, None, ag, 1, pp, 2, sets, ws, None, 1, sums, None) == L.ANX_EINVAL
    assert f(m.h, aa, None, 1, pp, 2, sets, ws, None, 1, sums, None) == L.ANX_EINVAL
    assert f(m.h, aa, ag, 1, None, 2, sets, ws, None, 1, sums, None) == L.ANX_EINVAL
    assert f(m.h, aa, ag, 1, pp, 2, None, ws, None, 1, sums, None) == L.ANX_EINVAL
    assert f(m.h, aa, ag, 1, pp, 2, sets, None, None, 1, sums, None) == L.ANX_EINVAL
    assert f(m.h, aa, ag, 1, pp, 2, sets, ws, None, 1, None, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep_confusables_packed(m.h, None, 0, b"abcdeg\0", 7, 1, pp, 2, sets, ws, None, 1, sums, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep_confusables_packed(m.h, b"abcdef\0", 7, b"abcdeg\0", 7, 1, pp, 2, sets, ws, None, 0, sums, None) == L.ANX_EINVAL
    assert lib.anx_debug_evaluate_sweep_confusables_chunk(m.h, aa, ag, 1, pp, 2, sets, ws, None, 257, sums, None, 1) == L.ANX_EINVAL
    assert lib.anx_debug_conf_sweep_stats(None, 8) == L.ANX_EINVAL
    # n == 0: zeroed summaries, no build and no device needed, the bytes behind them left alone, the stats not moved
    fresh = hand_model_no_device(tmp_path)
    before = A.VariantModel.conf_sweep_stats()
    assert list(before) == STATS
    C.memset(sums, 0xAB, 3 * C.sizeof(L.GoldSummary))
    assert f(fresh.h, None, None, 0, pp, 2, sets, ws, None, 2, sums, None) == L.ANX_OK
    assert bytes(sums)[:2 * 624] == bytes(2 * 624) and bytes(sums)[2 * 624:3 * 624] == b"\xab" * 624
    got = fresh.evaluate_sweep_confusables_arrays([], [], pats, [p, p, p], [[1.0, 1.0]] * 3, with_records=True)
    assert len(got[0]) == 3 and got[0].tobytes() == bytes(3 * 624) and got[1].shape == (3, 0)
    d = fresh.evaluate_sweep_confusables([], [], pats, [p, p], [[1.0, 1.0], [1.0, 0.9]], [False, True])
    assert d[0]["mrr"] == 0.0 and d[0]["confusable_weights"] == {} and d[1]["confusable_weights"] == {"+[e]": 0.9} and [x["early"] for x in d] == [False, True]
    assert A.VariantModel.conf_sweep_stats() == before


def test_models_with_lists_are_refused(tmp_path):
    """Built host-only models: the refusal comes before the device is asked for, with a message that says why."""
    p, pats = A.SearchParameters(max_anagram_distance=2, max_edit_distance=1, max_matches=3), ["-[y]+[i]"]
    lists = hand_model_no_device(tmp_path)
    lists.add_variant(3, "abcdefx", 0.9)   # ids 0-2 are <bos>, <eos>, <unk>: 3 is "abcdef"
    lists.build()
    with pytest.raises(A.AnxError) as e:
        lists.evaluate_sweep_confusables_arrays(["abcdef"], ["abcdeg"], pats, [p], [[1.1]])
    assert e.value.code == L.ANX_EINVAL and "variant list" in str(e.value)
    conf = hand_model_no_device(tmp_path)
    conf.add_to_confusables("-[y]+[i]", 1.1)
    conf.build()
    with pytest.raises(A.AnxError) as e:
        conf.evaluate_sweep_confusables_arrays(["abcdef"], ["abcdeg"], pats, [p], [[1.1]], packed=False)
    assert e.value.code == L.ANX_EINVAL and "confusable list of its own" in str(e.value)
    with pytest.raises(A.AnxError) as e:   # the mask hook refuses the same models
        conf.sweep_conf_masks(["abcdef"], pats, p)
    assert e.value.code == L.ANX_EINVAL and "confusable list of its own" in str(e.value)
    # the model-weight condition of the weight sweep: a model whose own weights sum to 0 would score NaN in the base run
    zero = hand_model_no_device(tmp_path, A.Weights(ld=0, lcs=0, prefix=0, suffix=0, case=0))
    zero.build()
    with pytest.raises(A.AnxError) as e:
        zero.evaluate_sweep_confusables_arrays(["abcdef"], ["abcdeg"], pats, [p], [[1.1]])
    assert e.value.code == L.ANX_EINVAL and "own weights" in str(e.value)
    plain = hand_model_no_device(tmp_path)
    plain.build()
    with pytest.raises(A.AnxError) as e:
        plain.evaluate_sweep_confusables_arrays(["abcdef"], ["abcdeg"], pats, [p], [[1.1]])
    assert e.value.code == L.ANX_ENODEVICE


def test_cli_builds_the_one_pattern_on_grid(tmp_path, capsys):
    a = cli.build_parser().parse_intermixed_args(["sweep", "-a", "a.tsv", "-l", "l.tsv", "--candidates", "c.tsv", "--candidate-weights", "1.1,1.25,0.9",
                                                  "--early-confusables", "pairs.tsv"])
    assert a.candidates == "c.tsv" and a.early_confusables and cli.parse_candidate_weights(a.candidate_weights) == [1.1, 1.25, 0.9]
    pats = cli.parse_candidates(["-[y]+[i]\t1.1", "", "+[e]$\t0.5\tignored", "=[a]-[b]\r"])   # a confusable list: the weight column is ignored
    assert pats == ["-[y]+[i]", "+[e]$", "=[a]-[b]"]
    labels, rows = cli.candidate_grid(pats, [1.1, 0.9])
    assert labels == [("-", 1.0), ("-[y]+[i]", 1.1), ("-[y]+[i]", 0.9), ("+[e]$", 1.1), ("+[e]$", 0.9), ("=[a]-[b]", 1.1), ("=[a]-[b]", 0.9)]
    assert rows == [[1.0, 1.0, 1.0], [1.1, 1.0, 1.0], [0.9, 1.0, 1.0], [1.0, 1.1, 1.0], [1.0, 0.9, 1.0], [1.0, 1.0, 1.1], [1.0, 1.0, 0.9]]
    s = {"n": 4, "accuracy_at_1": 0.5, "mrr": 0.625, "ranked_share": 0.75, "reasons": dict(zip(E.REASONS, (3, 0, 0, 0, 1, 0, 0, 0))),
         "gained_at_1": 1, "lost_at_1": 0, "n_results": 10}
    assert cli.candidate_tsv_line(labels[3], s) == "+[e]$\t1.1\t0.5\t0.625\t1\t0\t3\t0\t0\t0\t1\t0\t0\t0"
    assert cli.candidate_tsv_line(labels[0], s).split("\t")[:2] == ["-", "1"]
    assert len(cli.candidate_grid(["+[e]"] * 64, [1.1, 0.9, 1.2])[0]) == 193 and len(cli.candidate_grid(["+[e]"] * 51, [1.1] * 5)[0]) == 256
    with pytest.raises(ValueError, match="64"):   # 65 candidates
        cli.parse_candidates(["+[e]\t1.1"] * 65)
    with pytest.raises(ValueError, match="64"):
        cli.candidate_grid(["+[e]"] * 65, [1.1])
    with pytest.raises(ValueError, match="256"):   # 257 sets
        cli.candidate_grid(["+[e]"] * 64, [1.1, 0.9, 1.2, 1.3])
    for bad in ("", "1.1,heavy", "1.1,0", "-2", "nan"):
        with pytest.raises(ValueError):
            cli.parse_candidate_weights(bad)
    with pytest.raises(ValueError):
        cli.parse_candidates(["", "\r"])
    # the command itself: the limits are errors that name the limit, before a model is asked for anything it cannot do
    cand = tmp_path / "cand.tsv"
    cand.write_text("".join("+[%s]\t1.1\n" % chr(ord("a") + i % 26) for i in range(65)))
    lex = tmp_path / "hand.lexicon"
    lex.write_text("\n".join(E.HAND_WORDS) + "\n")
    pairs = tmp_path / "pairs.tsv"
    pairs.write_text("abcdef\tabcdeg\n")
    argv = ["sweep", "-a", ALPHABET, "-l", str(lex), "--device=-1", "--candidates", str(cand), "--candidate-weights", "1.1", str(pairs)]
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2 and "64" in capsys.readouterr().err
    cand.write_text("".join("+[%s]\t1.1\n" % chr(ord("a") + i % 26) for i in range(64)))
    with pytest.raises(SystemExit) as e:
        cli.main(argv[:-2] + ["1.1,0.9,1.2,1.3", str(pairs)])
    assert e.value.code == 2 and "256" in capsys.readouterr().err


def test_host_mask_against_the_oracle(tmp_path):
    """confusable_mask's host body (anx_debug_conf_mask_text) on 2 000 random (word, edited word) pairs and the twelve patterns: bit j is
    the oracle's found_in of pattern j, and the product of the set bits' weights in ascending order is, with `==`, what
    anx_model_confusable_weight_text gives on a model that holds the list."""
    pats = list(SC.PATTERNS)
    weights = [1.1, 0.7, 1.3, 0.95, 1.05, 0.9, 1.2, 0.85, 1.15, 0.8, 1.25, 0.75]
    assert len(pats) == 12 and any("|" in p for p in pats) and any(p.startswith("^") for p in pats) and any(p.endswith("$") for p in pats)
    assert any(p.startswith("=") or "=[" in p[1:] for p in pats) and any(not p.isascii() for p in pats)
    m = hand_model_no_device(tmp_path)
    for p, w in zip(pats, weights):
        m.add_to_confusables(p, w)
    pairs = SC.random_pairs(2000, seed=5) + [("huys", "huis"), ("abc", "abc"), ("", "e"), ("ë", "e"), ("zeë", "zee"), ("abd", "ad"), ("abz", "abzz")]
    seen, many = 0, 0
    for a, b in pairs:
        want = SC.oracle_mask(pats, a, b)
        got = A.VariantModel.conf_mask_text(pats, a, b)
        assert got == want, (a, b, bin(got), bin(want))
        assert SC.weight_of(got, weights) == m.confusable_weight_text(a, b), (a, b)
        seen |= got
        many += bin(got).count("1") >= 3
    assert seen == (1 << 12) - 1 and many > 0   # every pattern matched somewhere, and some pair by three or more
    lib = L.lib()
    out = C.c_uint64(7)
    one = (C.c_char_p * 1)(b"+[e")
    assert lib.anx_debug_conf_mask_text(one, 1, b"a", b"b", C.byref(out)) == L.ANX_EINVAL and "pattern 0" in L.last_error()
    assert lib.anx_debug_conf_mask_text(one, 0, b"a", b"b", C.byref(out)) == L.ANX_EINVAL
    assert lib.anx_debug_conf_mask_text((C.c_char_p * 1)(b"+[e]"), 1, None, b"b", C.byref(out)) == L.ANX_EINVAL


KEYS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
LDS_BYTES = {"k_cs_score": 0, "k_cs_ranges": 0, "k_cs_inbits": 0, "k_cs_screen": 0, "k_cs_mask_prep": 0, "k_cs_mask_diff": 0, "k_cs_mask_clean": 768,
             "k_cs_mask_find": 0, "k_cs_count": 0, "k_cs_fill": 512, "k_cs_slot_w": 512}
# DESIGN.md section 5 "Confusable sweep"; 512 bytes: the set's 64 weights; 768 bytes: three words per lane the compiler keeps in LDS for the
# clean-up's line-break patterns (semantic_score)


@pytest.fixture(scope="module")
def csweep_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("csweep") / "csweep.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                           "--cuda-device-only", "-o", out, os.path.join(CSRC, "csweep.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        ks[m.group(2)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(3)).group(1)) for k in KEYS}
        ks[m.group(2)]["group_segment_fixed_size"] = int(m.group(1))
    return ks


def test_csweep_instantiates_its_own_kernels_only(csweep_isa):
    """k_rank, k_conf_apply_late, k_rw_classify and the radix sort stay their files': csweep.hip reaches them through host functions."""
    assert len(csweep_isa) == len(LDS_BYTES) and all("k_cs_" in n for n in csweep_isa), sorted(csweep_isa)


@pytest.mark.parametrize("kernel", sorted(LDS_BYTES))
def test_csweep_kernels_isa_metadata(csweep_isa, kernel):
    """DESIGN.md section 5 "Confusable sweep": no kernel of csweep.hip uses scratch or spills (VGPRs or SGPRs), and the VGPR and LDS
    figures are the ones the document states.  Resource figures only.  The mask pass is four kernels for this very bound: as ONE kernel
    around the edit-script body it spilled 83 SGPRs into VGPR lanes, as k_conf_script does."""
    r = [v for n, v in csweep_isa.items() if kernel + "ENS" in n or n.endswith(kernel)]
    assert len(r) == 1, (kernel, sorted(csweep_isa))
    r = r[0]
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    section = design[design.index("### Confusable sweep"):]
    section = section[:section.index("\n### ", 1)]
    print(kernel, r)
    assert r["group_segment_fixed_size"] == LDS_BYTES[kernel], (kernel, r)
    assert re.search(r"`%s`[^\n]*\b%d VGPRs" % (kernel, r["vgpr_count"]), section), (kernel, r["vgpr_count"])   # the figures DESIGN.md states
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, (kernel, r)
    assert r["sgpr_spill_count"] == 0, (kernel, r)
