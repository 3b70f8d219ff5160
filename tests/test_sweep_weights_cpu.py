"""anx_evaluate_sweep_weights without a GPU: the C ABI and its Python layers exist, the call refuses what it must (also the models it
does not serve yet: variant lists and confusable lists), the empty call is answered before anything is counted, the command line knows
weight grids and leaves the grids without weights alone, and the gfx950 ISA metadata of reweigh.hip's kernels holds what DESIGN.md
section 5 "Weight sweep" states."""
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "analiticcl_amd", "csrc")
NAMES = ("anx_evaluate_sweep_weights", "anx_evaluate_sweep_weights_packed", "anx_debug_evaluate_sweep_weights_chunk", "anx_debug_weight_sweep_stats")
ALPHABET = os.path.join(REPO, "tests", "golden", "data", "simple_alphabet.tsv")


def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "anx.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert hasattr(lib, n), n
    assert L.lib().anx_abi_version() == L.ABI_VERSION == 3
    version_comment = hdr[:hdr.index("#define ANX_ABI_VERSION")]
    assert "anx_evaluate_sweep_weights" in version_comment
    subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(REPO, "include"), "-x", "c", "-"], input=b'#include "anx.h"\n', check=True)


def hand_model_no_device(tmp_path, weights=None):
    lex = tmp_path / "hand.lexicon"
    lex.write_text("\n".join(E.HAND_WORDS) + "\n")
    m = A.VariantModel(ALPHABET, weights or A.Weights(), device=-1)   # host only: never resident on a device
    m.read_lexicon(str(lex))
    return m


def test_errors_and_the_empty_call(tmp_path):
    m = hand_model_no_device(tmp_path)
    p, w = A.SearchParameters(max_anagram_distance=2, max_edit_distance=1, max_matches=3), A.Weights()
    with pytest.raises(A.AnxError) as e:   # before build()
        m.evaluate_sweep_weights_arrays(["abcdef"], ["abcdeg"], [p], [w])
    assert e.value.code == L.ANX_ENOTBUILT
    m.build()
    for kw in ({}, {"packed": False}, {"chunk": 1}):   # the packed form, the pointer form, the chunk hook
        with pytest.raises(A.AnxError) as e:
            m.evaluate_sweep_weights_arrays(["abcdef"], ["abcdeg"], [p, p], [w, A.Weights(ld=1.0)], **kw)
        assert e.value.code == L.ANX_ENODEVICE
    with pytest.raises(ValueError):
        m.evaluate_sweep_weights_arrays(["a"], [], [p], [w])
    with pytest.raises(ValueError):   # lists of unequal length
        m.evaluate_sweep_weights_arrays(["a"], ["a"], [p, p], [w])
    lib = L.lib()
    sets = (L.Params * 257)(*[p._c() for _ in range(257)])
    ws = (L.Weights * 257)(*[w._c() for _ in range(257)])
    sums = (L.GoldSummary * 257)()
    a, g = (C.c_char_p * 1)(b"abcdef"), (C.c_char_p * 1)(b"abcdeg")
    for n_sets in (0, 257):
        assert lib.anx_evaluate_sweep_weights(m.h, a, g, 1, sets, ws, n_sets, sums, None) == L.ANX_EINVAL
        assert lib.anx_evaluate_sweep_weights_packed(m.h, b"abcdef\0", 7, b"abcdeg\0", 7, 1, sets, ws, n_sets, sums, None) == L.ANX_EINVAL
        assert lib.anx_debug_evaluate_sweep_weights_chunk(m.h, a, g, 1, sets, ws, n_sets, sums, None, 1) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep_weights(m.h, a, g, 1, None, ws, 1, sums, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep_weights(m.h, a, g, 1, sets, None, 1, sums, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep_weights(m.h, a, g, 1, sets, ws, 1, None, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep_weights(None, a, g, 1, sets, ws, 1, sums, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep_weights(m.h, None, g, 1, sets, ws, 1, sums, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep_weights(m.h, a, None, 1, sets, ws, 1, sums, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep_weights_packed(m.h, None, 0, b"abcdeg\0", 7, 1, sets, ws, 1, sums, None) == L.ANX_EINVAL
    assert lib.anx_debug_weight_sweep_stats(None, 8) == L.ANX_EINVAL
    # a weight below 0, one that is not finite, a set whose five weights sum to 0: in any set of the list
    for bad in (A.Weights(ld=-0.5), A.Weights(lcs=math.nan), A.Weights(case=math.inf), A.Weights(ld=0, lcs=0, prefix=0, suffix=0, case=0)):
        for at in (0, 1):
            two = (L.Weights * 2)(*[bad._c() if s == at else w._c() for s in range(2)])
            assert lib.anx_evaluate_sweep_weights(m.h, a, g, 1, sets, two, 2, sums, None) == L.ANX_EINVAL, (bad.to_dict(), at)
            assert lib.anx_evaluate_sweep_weights(m.h, None, None, 0, sets, two, 2, sums, None) == L.ANX_EINVAL
    # n == 0: zeroed summaries, no build and no device needed, the bytes behind them left alone, the stats not moved
    fresh = hand_model_no_device(tmp_path)
    before = A.VariantModel.weight_sweep_stats()
    assert list(before) == ["calls", "chunks", "groups", "sets", "pair_passes", "batch_runs", "rows_rescored", "bytes_down"]
    C.memset(sums, 0xAB, 3 * C.sizeof(L.GoldSummary))
    assert lib.anx_evaluate_sweep_weights(fresh.h, None, None, 0, sets, ws, 2, sums, None) == L.ANX_OK
    assert bytes(sums)[:2 * 624] == bytes(2 * 624) and bytes(sums)[2 * 624:3 * 624] == b"\xab" * 624
    got = fresh.evaluate_sweep_weights_arrays([], [], [p, p, p], [w, w, w], with_records=True)
    assert len(got[0]) == 3 and got[0].tobytes() == bytes(3 * 624) and got[1].shape == (3, 0)
    d = fresh.evaluate_sweep_weights([], [], [p], [A.Weights(ld=1.0, lcs=0.0)])
    assert d[0]["mrr"] == 0.0 and d[0]["weights"] == {"ld": 1.0, "lcs": 0.0, "prefix": 0.125, "suffix": 0.125, "case": 0.125}
    assert A.VariantModel.weight_sweep_stats() == before


def test_models_that_are_not_plain_are_refused(tmp_path):
    """Built host-only models: the refusal comes before the device is asked for, with a message that says why."""
    p, w = A.SearchParameters(max_anagram_distance=2, max_edit_distance=1, max_matches=3), A.Weights()
    lists = hand_model_no_device(tmp_path)
    lists.add_variant(3, "abcdefx", 0.9)   # ids 0-2 are <bos>, <eos>, <unk>: 3 is "abcdef"
    lists.build()
    with pytest.raises(A.AnxError) as e:
        lists.evaluate_sweep_weights_arrays(["abcdef"], ["abcdeg"], [p], [w])
    assert e.value.code == L.ANX_EINVAL and "variant list" in str(e.value)
    conf = hand_model_no_device(tmp_path)
    conf.add_to_confusables("-[y]+[i]", 1.1)
    conf.build()
    with pytest.raises(A.AnxError) as e:
        conf.evaluate_sweep_weights_arrays(["abcdef"], ["abcdeg"], [p], [w], packed=False)
    assert e.value.code == L.ANX_EINVAL and "confusable list" in str(e.value)
    # a model whose own weights sum to 0 would score NaN in the base run: refused as the sets' weights are
    zero = hand_model_no_device(tmp_path, A.Weights(ld=0, lcs=0, prefix=0, suffix=0, case=0))
    zero.build()
    with pytest.raises(A.AnxError) as e:
        zero.evaluate_sweep_weights_arrays(["abcdef"], ["abcdeg"], [p], [w])
    assert e.value.code == L.ANX_EINVAL
    plain = hand_model_no_device(tmp_path)
    plain.build()
    with pytest.raises(A.AnxError) as e:
        plain.evaluate_sweep_weights_arrays(["abcdef"], ["abcdeg"], [p], [w])
    assert e.value.code == L.ANX_ENODEVICE


def test_cli_parses_grids_with_and_without_weight_columns():
    assert cli.GRID_COLUMNS == ("k", "d", "n", "t", "T", "s", "freq-weight")
    assert cli.GRID_WEIGHT_COLUMNS == ("w-ld", "w-lcs", "w-prefix", "w-suffix", "w-case")
    a = cli.build_parser().parse_intermixed_args(["sweep", "-a", "a.tsv", "-l", "l.tsv", "-k", "2", "-d", "1", "-n", "5", "-t", "0.3", "-T", "1.5", "--weight-ld", "0.4",
                                                  "--weight-case", "0", "--grid", "g.tsv", "pairs.tsv"])
    plain = cli.parse_grid(["k\tn", "3\t1", "2\t7"], a)
    assert [sorted(d) for d in plain] == [sorted(cli.GRID_COLUMNS)] * 2   # a grid without weight columns: the dicts it always gave
    s = {"n": 4, "accuracy_at_1": 0.5, "mrr": 0.625, "ranked_share": 0.75, "reasons": dict(zip(E.REASONS, (3, 0, 0, 0, 1, 0, 0, 0))),
         "gained_at_1": 1, "lost_at_1": 0, "n_results": 10}
    assert cli.sweep_tsv_line(plain[1], s) == "2\t1\t7\t0.3\t1.5\t0\t0\t4\t0.5\t0.625\t0.75\t3\t0\t0\t0\t1\t0\t0\t0\t1\t0\t2.5"
    sets = cli.parse_grid(["n\tw-ld\tw-prefix", "1\t1\t0", "3\t0.25\t0.5", ""], a)
    assert [(d["n"], d["w-ld"], d["w-lcs"], d["w-prefix"], d["w-suffix"], d["w-case"]) for d in sets] == \
        [("1", "1", "0.125", "0", "0.125", "0"), ("3", "0.25", "0.125", "0.5", "0.125", "0")]
    assert all(d["k"] == "2" and d["t"] == "0.3" for d in sets)
    assert cli.grid_weights(sets[1]).to_dict() == {"ld": 0.25, "lcs": 0.125, "prefix": 0.5, "suffix": 0.125, "case": 0.0}
    assert cli.grid_params(sets[1], a)._c().max_matches == 3
    assert cli.sweep_tsv_line(sets[1], s) == "2\t1\t3\t0.3\t1.5\t0\t0\t0.25\t0.125\t0.5\t0.125\t0\t4\t0.5\t0.625\t0.75\t3\t0\t0\t0\t1\t0\t0\t0\t1\t0\t2.5"
    for bad in (["w-ld\tw-ld", "1\t1"], ["w-ld\tq", "1\t2"], ["w-ld", "1\t2"]):
        with pytest.raises(ValueError):
            cli.parse_grid(bad, a)
    with pytest.raises(ValueError):
        cli.grid_weights(cli.parse_grid(["w-ld", "heavy"], a)[0])


KEYS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
LDS_BYTES = {"k_rw_base": 0, "k_rw_pre": 0, "k_rw_score": 0, "k_rw_fill": 0, "k_rw_classify": 320}   # DESIGN.md section 5 "Weight sweep"


def test_reweigh_kernels_isa_metadata(tmp_path):
    """DESIGN.md section 5 "Weight sweep": no kernel of reweigh.hip uses scratch or spills, every one stays at or below 64 VGPRs (eight
    waves per SIMD), only k_rw_classify uses LDS (k_sweep_classify's 320 bytes), and reweigh.hip instantiates no kernel of another
    file: k_rank stays engine.hip's."""
    out = str(tmp_path / "reweigh.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                           "--cuda-device-only", "-o", out, os.path.join(CSRC, "reweigh.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        ks[m.group(2)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(3)).group(1)) for k in KEYS}
        ks[m.group(2)]["group_segment_fixed_size"] = int(m.group(1))
    assert len(ks) == len(LDS_BYTES) and all("k_rw_" in n for n in ks), sorted(ks)
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    section = design[design.index("### Weight sweep"):]
    section = section[:section.index("\n### ", 1)]
    for kernel, lds in LDS_BYTES.items():
        r = [v for n, v in ks.items() if kernel in n]
        assert len(r) == 1, (kernel, sorted(ks))
        assert r[0]["vgpr_spill_count"] == 0 and r[0]["sgpr_spill_count"] == 0 and r[0]["private_segment_fixed_size"] == 0, (kernel, r[0])
        assert r[0]["group_segment_fixed_size"] == lds and r[0]["vgpr_count"] <= 64, (kernel, r[0])
        assert re.search(r"`%s`[^\n]*\b%d VGPRs" % (kernel, r[0]["vgpr_count"]), section), (kernel, r[0]["vgpr_count"])   # the figures DESIGN.md states
    # one 64-bit integer atomic per counter goes to HBM from the reduction, and nothing is summed in floating point
    body = text[text.index("k_rw_classify"):]
    body = body[:body.index("s_endpgm")]
    assert body.count("global_atomic_add_x2") == 1 and "atomic_add_f" not in text and "atomic_pk_add" not in text
