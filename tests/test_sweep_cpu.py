"""anx_evaluate_sweep without a GPU: the C ABI and its Python layers exist and agree, the call refuses what it must, the summary helper
(tests/sweep_twin.py) agrees with evaluate_summary on hand-written records, the command line knows `sweep --grid`, and the new kernels'
gfx950 ISA metadata holds what DESIGN.md section 5 "Parameter sweep" states."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli

import eval_twin as E
import sweep_twin as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "analiticcl_amd", "csrc")
NAMES = ("anx_evaluate_sweep", "anx_evaluate_sweep_packed", "anx_debug_evaluate_sweep_chunk", "anx_debug_sweep_stats")


def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "anx.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert hasattr(lib, n), n
    assert "#define ANX_SWEEP_MAX_SETS 256" in hdr and "#define ANX_GOLD_RANK_BINS 64" in hdr
    assert (L.SWEEP_MAX_SETS, L.GOLD_RANK_BINS, S.RANK_BINS) == (256, 64, 64)
    assert L.lib().anx_abi_version() == L.ABI_VERSION == 3


def test_summary_layout():
    hdr = open(os.path.join(REPO, "include", "anx.h")).read()
    assert "static_assert(sizeof(anx_gold_summary) == 624" in hdr
    dt = np.dtype(A.VariantModel.SUMMARY_DTYPE)
    assert C.sizeof(L.GoldSummary) == 624 == dt.itemsize
    offsets = {"n": 0, "gold_known": 8, "reasons": 16, "rank_hist": 80, "rr_fixed": 592, "n_results": 600, "gained_at_1": 608, "lost_at_1": 616}
    assert [name for name, _t in L.GoldSummary._fields_] == list(offsets) == list(dt.names) == list(S.KEYS)
    for name, off in offsets.items():
        assert getattr(L.GoldSummary, name).offset == off == dt.fields[name][1], name
    # the struct as a C compiler lays it out, and the header as plain C
    src = '#include "anx.h"\n#include <stddef.h>\nint a[sizeof(anx_gold_summary) == 624 ? 1 : -1];\n' + \
          "".join("int b%d[offsetof(anx_gold_summary, %s) == %d ? 1 : -1];\n" % (i, name, off) for i, (name, off) in enumerate(offsets.items()))
    subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(REPO, "include"), "-x", "c", "-"], input=src.encode(), check=True)


def hand_model_no_device(tmp_path):
    alphabet = os.path.join(REPO, "tests", "golden", "data", "simple_alphabet.tsv")
    lex = tmp_path / "hand.lexicon"
    lex.write_text("\n".join(E.HAND_WORDS) + "\n")
    m = A.VariantModel(alphabet, A.Weights(), device=-1)   # host only: never resident on a device
    m.read_lexicon(str(lex))
    return m


def test_errors_and_the_empty_call(tmp_path):
    m = hand_model_no_device(tmp_path)
    p = A.SearchParameters(max_anagram_distance=2, max_edit_distance=1, max_matches=3)
    with pytest.raises(A.AnxError) as e:   # before build()
        m.evaluate_sweep_arrays(["abcdef"], ["abcdeg"], [p])
    assert e.value.code == L.ANX_ENOTBUILT
    m.build()
    for kw in ({}, {"packed": False}, {"chunk": 1}):   # the packed form, the pointer form, the chunk hook
        with pytest.raises(A.AnxError) as e:
            m.evaluate_sweep_arrays(["abcdef"], ["abcdeg"], [p, p], **kw)
        assert e.value.code == L.ANX_ENODEVICE
    with pytest.raises(ValueError):
        m.evaluate_sweep_arrays(["a"], [], [p])
    lib = L.lib()
    sets = (L.Params * 257)(*[p._c() for _ in range(257)])
    sums = (L.GoldSummary * 257)()
    a, g = (C.c_char_p * 1)(b"abcdef"), (C.c_char_p * 1)(b"abcdeg")
    for n_sets in (0, 257):
        assert lib.anx_evaluate_sweep(m.h, a, g, 1, sets, n_sets, sums, None, None) == L.ANX_EINVAL
        assert lib.anx_evaluate_sweep_packed(m.h, b"abcdef\0", 7, b"abcdeg\0", 7, 1, sets, n_sets, sums, None, None) == L.ANX_EINVAL
        assert lib.anx_debug_evaluate_sweep_chunk(m.h, a, g, 1, sets, n_sets, sums, None, None, 1) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep(m.h, a, g, 1, None, 1, sums, None, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep(m.h, a, g, 1, sets, 1, None, None, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep(None, a, g, 1, sets, 1, sums, None, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep(m.h, None, g, 1, sets, 1, sums, None, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep(m.h, a, None, 1, sets, 1, sums, None, None) == L.ANX_EINVAL
    assert lib.anx_evaluate_sweep_packed(m.h, None, 0, b"abcdeg\0", 7, 1, sets, 1, sums, None, None) == L.ANX_EINVAL
    assert lib.anx_debug_sweep_stats(None, 7) == L.ANX_EINVAL
    # n == 0: zeroed summaries, no build and no device needed
    fresh = hand_model_no_device(tmp_path)
    C.memset(sums, 0xAB, 3 * C.sizeof(L.GoldSummary))
    assert lib.anx_evaluate_sweep(fresh.h, None, None, 0, sets, 2, sums, None, None) == L.ANX_OK
    assert bytes(sums)[:2 * 624] == bytes(2 * 624) and bytes(sums)[2 * 624:3 * 624] == b"\xab" * 624
    got = fresh.evaluate_sweep_arrays([], [], [p, p, p], with_records=True, with_pairs=True)
    assert len(got[0]) == 3 and got[0].tobytes() == bytes(3 * 624) and got[1].shape == (3, 0) and len(got[2]) == 0
    assert fresh.evaluate_sweep([], [], [p])[0]["mrr"] == 0.0
    before = A.VariantModel.sweep_stats()
    assert list(before) == ["calls", "chunks", "sets", "pair_passes", "lookups", "batch_runs", "bytes_down"]
    assert fresh.evaluate_sweep([], [], [p]) and A.VariantModel.sweep_stats() == before   # an empty call is answered before anything is counted


def hand_written_records():
    rec = np.zeros(8, dtype=np.dtype(A.VariantModel.GOLD_DTYPE))   # test_evaluate_summary_on_hand_written_records' records
    rec["rank"] = [0, 0, 1, 3, -1, -1, -1, -1]
    rec["reason"] = [E.RANKED, E.RANKED, E.RANKED, E.RANKED, E.ANAGRAM, E.NOT_A_RESULT, E.CROPPED, E.ANAGRAM]
    rec["gold_vocab_id"] = [5, 6, 7, 8, 9, 0xFFFFFFFF, 10, 11]
    rec["n_results"] = [1, 2, 3, 4, 0, 5, 6, 0]
    return rec


def test_helper_agrees_with_evaluate_summary():
    rec = hand_written_records()
    s, ref = S.summarize(rec), A.VariantModel.evaluate_summary(rec)
    assert s["n"] == ref["n"] == 8 and s["gold_known"] == ref["gold_known"] == 7
    assert s["reasons"] == [ref["reasons"][name] for name in E.REASONS]
    assert s["rank_hist"][:4] == [2, 1, 0, 1] and sum(s["rank_hist"]) == 4 and s["n_results"] == 21
    assert s["rr_fixed"] == 2 * (1 << 32) + (1 << 31) + (1 << 30)
    assert s["rank_hist"][0] / s["n"] == ref["accuracy_at_1"] and s["reasons"][E.RANKED] / s["n"] == ref["ranked_share"]
    # each term of rr_fixed is truncated by less than 2^-32; 1e-12 covers the float sum over so few pairs
    assert abs(s["rr_fixed"] / 2.0 ** 32 / s["n"] - ref["mrr"]) < 2.0 ** -32 + 1e-12
    assert s["gained_at_1"] == s["lost_at_1"] == 0
    # against a baseline: pair 2 (rank 1) and pair 4 (not ranked) move to rank 0, pair 0 leaves it
    other = rec.copy()
    other["rank"][[2, 4, 0]] = [0, 0, 2]
    other["reason"][4] = E.RANKED
    t = S.summarize(other, baseline=rec)
    assert (t["gained_at_1"], t["lost_at_1"], t["rank_hist"][0]) == (2, 1, 3)
    # the product's own conversion reads the same numbers off a summary
    arr = np.zeros(1, dtype=np.dtype(A.VariantModel.SUMMARY_DTYPE))
    for k in S.KEYS:
        arr[k][0] = s[k]
    assert S.of_product(arr[0]) == s
    d = A.VariantModel.sweep_summary(arr[0])
    assert d["accuracy_at_1"] == ref["accuracy_at_1"] and d["ranked_share"] == ref["ranked_share"] and d["reasons"] == ref["reasons"]
    assert abs(d["mrr"] - ref["mrr"]) < 2.0 ** -32 + 1e-12 and d["rank_hist"] == s["rank_hist"] and d["n_results"] == 21
    # third-of-a-unit terms are truncated, not rounded
    three = np.zeros(1, dtype=rec.dtype)
    three["rank"], three["reason"] = 2, E.RANKED
    assert S.summarize(three)["rr_fixed"] == 1431655765


def test_ranks_beyond_the_last_bin():
    rec = np.zeros(4, dtype=np.dtype(A.VariantModel.GOLD_DTYPE))
    rec["rank"] = [62, 63, 64, 1000]
    rec["reason"] = E.RANKED
    s = S.summarize(rec)
    assert s["rank_hist"][62] == 1 and s["rank_hist"][63] == 3 and sum(s["rank_hist"]) == 4
    assert s["rr_fixed"] == (1 << 32) // 63 + (1 << 32) // 64 + (1 << 32) // 65 + (1 << 32) // 1001


def test_cli_parses_sweep_and_the_grid(tmp_path):
    p = cli.build_parser()
    common = ["-a", "a.tsv", "-l", "l.tsv", "-k", "2", "-d", "0.3;2", "-n", "5", "-t", "0.3", "-T", "1.5", "-s", "--devices", "0,1"]
    q = p.parse_intermixed_args(["query"] + common)
    assert q.grid is None
    a = p.parse_intermixed_args(["sweep"] + common + ["--grid", "g.tsv", "--summary-json", "s.json", "pairs.tsv"])
    assert a.mode == "sweep" and a.grid == "g.tsv" and a.summary_json == "s.json" and a.files == ["pairs.tsv"]
    for k, v in vars(q).items():
        if k not in ("mode", "files", "summary_json", "grid"):
            assert getattr(a, k) == v, k
    # three lines: a ratio with limit, an absent column (n, t, T, freq-weight come from the command line)
    sets = cli.parse_grid(["k\td\ts", "3\t2\t0", "2\t0.3;2\t1", "0.5\t1\t0", ""], a)
    assert [(d["k"], d["d"], d["s"]) for d in sets] == [("3", "2", "0"), ("2", "0.3;2", "1"), ("0.5", "1", "0")]
    assert all((d["n"], d["t"], d["T"], d["freq-weight"]) == ("5", "0.3", "1.5", "0") for d in sets)
    P = [cli.grid_params(d, a) for d in sets]
    c = [x._c() for x in P]
    assert (c[0].max_anagram_distance.kind, c[0].max_anagram_distance.value, c[0].max_edit_distance.value, c[0].stop_at_exact_match) == (0, 3, 2, 0)
    assert (c[1].max_edit_distance.kind, c[1].max_edit_distance.value, c[1].stop_at_exact_match) == (2, 2, 1)
    assert abs(c[1].max_edit_distance.ratio - 0.3) < 1e-7
    assert (c[2].max_anagram_distance.kind, c[2].max_anagram_distance.ratio) == (1, 0.5)
    assert all((x.max_matches, x.score_threshold, x.cutoff_threshold) == (5, 0.3, 1.5) for x in c)
    # a grid without the column s takes the command line's -s
    assert [d["s"] for d in cli.parse_grid(["n", "1"], a)] == ["1"]
    for bad in (["k\tq", "1\t2"], ["k\td", "1"], ["k"], [], ["k\tk", "1\t1"], ["s", "yes"]):
        with pytest.raises(ValueError):
            cli.parse_grid(bad, a)
    s = {"n": 4, "accuracy_at_1": 0.5, "mrr": 0.625, "ranked_share": 0.75, "reasons": dict(zip(E.REASONS, (3, 0, 0, 0, 1, 0, 0, 0))),
         "gained_at_1": 1, "lost_at_1": 0, "n_results": 10}
    assert cli.sweep_tsv_line(sets[1], s) == "2\t0.3;2\t5\t0.3\t1.5\t1\t0\t4\t0.5\t0.625\t0.75\t3\t0\t0\t0\t1\t0\t0\t0\t1\t0\t2.5"


KEYS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
LDS_BYTES = {"k_sweep_sections": 0, "k_sweep_lookup": 0, "k_sweep_rows": 0, "k_sweep_classify": 320}   # DESIGN.md section 5 "Parameter sweep"


def test_sweep_kernels_isa_metadata(tmp_path):
    """DESIGN.md section 5 "Parameter sweep": no kernel of sweep.hip uses scratch or spills, every one stays at or below 64 VGPRs (eight
    waves per SIMD), and only k_sweep_classify uses LDS: 76 32-bit cells and two 64-bit cells, 320 bytes."""
    out = str(tmp_path / "sweep.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                           "--cuda-device-only", "-o", out, os.path.join(CSRC, "sweep.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        ks[m.group(2)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(3)).group(1)) for k in KEYS}
        ks[m.group(2)]["group_segment_fixed_size"] = int(m.group(1))
    assert len(ks) == len(LDS_BYTES) and all("k_sweep_" in n for n in ks), sorted(ks)
    for kernel, lds in LDS_BYTES.items():
        r = [v for n, v in ks.items() if kernel in n]
        assert len(r) == 1, (kernel, sorted(ks))
        assert r[0]["vgpr_spill_count"] == 0 and r[0]["sgpr_spill_count"] == 0 and r[0]["private_segment_fixed_size"] == 0, (kernel, r[0])
        assert r[0]["group_segment_fixed_size"] == lds and r[0]["vgpr_count"] <= 64, (kernel, r[0])
    for n in ks:   # eval.hip's pinned kernels stay the only ones of their names
        assert not any(old in n for old in ("k_eval_sections", "k_eval_lookup", "k_eval_rows", "k_eval_classify")), n
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    section = design[design.index("### Parameter sweep"):]
    assert "320 bytes" in section[:section.index("\n### ", 1)]
    # one 64-bit integer atomic per counter goes to HBM, and nothing is summed in floating point
    body = text[text.index("k_sweep_classify"):]
    body = body[:body.index("s_endpgm")]
    assert body.count("global_atomic_add_x2") == 1 and "atomic_add_f" not in body and "atomic_pk_add" not in body
