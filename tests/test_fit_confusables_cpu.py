"""anx_fit_confusable_weights without a GPU: the C ABI and its Python layers exist with the struct sizes the header states, the call
refuses what it must with a message that says why (before the device is asked for), the empty call is answered without a build or a
device, the round's selection (anx_debug_fit_select, host only) picks what the contract says on hand-made trial tables, the command line
names its argument errors, and fit.hip's kernels compile for gfx950 without scratch and without spills."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli

import eval_twin as E
import fit_twin as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "analiticcl_amd", "csrc")
NAMES = ("anx_fit_confusable_weights", "anx_fit_confusable_weights_packed", "anx_debug_fit_confusable_weights_chunk", "anx_debug_fit_select",
         "anx_debug_fit_stats")
ALPHABET = os.path.join(REPO, "tests", "golden", "data", "simple_alphabet.tsv")
STATS = ["calls", "chunks", "rounds", "trial_launches", "state_pairs", "state_slots", "bytes_down"]


def test_symbols_and_struct_sizes():
    hdr = open(os.path.join(REPO, "include", "anx.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert hasattr(lib, n), n
    assert L.lib().anx_abi_version() == L.ABI_VERSION == 3   # additive: the version stays
    assert "anx_fit_confusable_weights" in hdr[:hdr.index("#define ANX_ABI_VERSION")]
    assert (C.sizeof(L.FitCounts), C.sizeof(L.FitRound), C.sizeof(L.FitResult)) == (24, 40, 64)
    assert (np.dtype(A.VariantModel.FIT_COUNTS_DTYPE).itemsize, np.dtype(A.VariantModel.FIT_ROUND_DTYPE).itemsize,
            np.dtype(A.VariantModel.FIT_RESULT_DTYPE).itemsize) == (24, 40, 64)
    prog = (b'#include "anx.h"\n#include <stddef.h>\n_Static_assert(sizeof(anx_fit_counts) == 24 && sizeof(anx_fit_round) == 40, "sizes");\n'
            b'_Static_assert(offsetof(anx_fit_params, start) == %d && offsetof(anx_fit_params, min_gain) == %d && sizeof(anx_fit_params) == %d, "params");\n'
            % (L.FitParams.start.offset, L.FitParams.min_gain.offset, C.sizeof(L.FitParams)))
    subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(REPO, "include"), "-x", "c", "-"], input=prog, check=True)
    assert (L.FIT_MAX_GRID, L.FIT_MAX_ROUNDS, L.ANX_FIT_ACC1, L.ANX_FIT_MRR) == (16, 256, 0, 1)
    for name in ("fit_confusables", "fit_confusables_arrays", "fit_stats", "fit_select"):
        assert callable(getattr(A.VariantModel, name)), name


def hand_model_no_device(tmp_path, weights=None):
    lex = tmp_path / "hand.lexicon"
    lex.write_text("\n".join(E.HAND_WORDS) + "\n")
    m = A.VariantModel(ALPHABET, weights or A.Weights(), device=-1)   # host only: never resident on a device
    m.read_lexicon(str(lex))
    return m


class Call:
    """the pointer form with ctypes arrays built here; every argument can be replaced"""

    def __init__(self, m, pats=(b"-[y]+[i]", b"+[e]"), grid=(0.8, 1.25), start=None, objective=0, max_rounds=4, min_gain=1, a=(b"abcdef",), g=(b"abcdeg",)):
        self.m, self.n, self.np = m, len(a), len(pats)
        self.aa, self.ag = (C.c_char_p * max(len(a), 1))(*a), (C.c_char_p * max(len(g), 1))(*g)
        self.pp = (C.c_char_p * max(len(pats), 1))(*pats)
        self.grid = (C.c_double * max(len(grid), 1))(*grid)
        self.start = None if start is None else (C.c_double * max(len(start), 1))(*start)
        self.fp = L.FitParams(self.grid, len(grid), 0, self.start, objective, max_rounds, min_gain)
        self.params = A.SearchParameters(max_anagram_distance=2, max_edit_distance=1, max_matches=3)._c()
        self.w = (C.c_double * 64)(*([7.0] * 64))
        self.rounds = (L.FitRound * 256)()
        self.res = L.FitResult()
        C.memset(C.byref(self.res), 0xAB, C.sizeof(self.res))

    def __call__(self, **over):
        v = dict(m=self.m.h, a=self.aa, g=self.ag, n=self.n, pats=self.pp, np=self.np, params=C.byref(self.params), fp=C.byref(self.fp), w=self.w,
                 rounds=self.rounds, res=C.byref(self.res))
        v.update(over)
        return L.lib().anx_fit_confusable_weights(v["m"], v["a"], v["g"], v["n"], v["pats"], v["np"], v["params"], v["fp"], v["w"], v["rounds"], None, v["res"])


def refused(rc, *words):
    assert rc == L.ANX_EINVAL
    msg = L.last_error()
    assert all(w in msg for w in words), (msg, words)


def test_refusals_and_the_empty_call(tmp_path):
    m = hand_model_no_device(tmp_path)
    p = A.SearchParameters(max_anagram_distance=2, max_edit_distance=1, max_matches=3)
    pats = ["-[y]+[i]", "+[e]"]
    with pytest.raises(A.AnxError) as e:   # before build()
        m.fit_confusables_arrays(["abcdef"], ["abcdeg"], pats, p, [0.8, 1.25])
    assert e.value.code == L.ANX_ENOTBUILT
    m.build()
    for kw in ({}, {"packed": False}, {"chunk": 1}):   # a plain host-only model has no device
        with pytest.raises(A.AnxError) as e:
            m.fit_confusables_arrays(["abcdef"], ["abcdeg"], pats, p, [0.8, 1.25], **kw)
        assert e.value.code == L.ANX_ENODEVICE
    assert Call(m, pats=[b"+[e]"] * 64, grid=[1.1] * 16, max_rounds=256)() == L.ANX_ENODEVICE   # the limits themselves are served
    for over in ("m", "a", "g", "pats", "params", "fp", "w", "rounds", "res"):
        refused(Call(m)(**{over: None}), "NULL")
    c = Call(m)
    c.fp.grid = None
    refused(c(), "NULL")
    refused(Call(m)(np=0), "patterns", "64")
    refused(Call(m, pats=[b"+[e]"] * 65)(), "patterns", "64")
    for bad in (b"", b"+[e", b"x[e]", b"+[]", b"^$"):
        refused(Call(m, pats=[b"+[e]", bad])(), "pattern 1")
    refused(Call(m, grid=[])(), "grid", "16")
    refused(Call(m, grid=[1.1] * 17)(), "grid", "16")
    refused(Call(m, max_rounds=0)(), "max_rounds", "256")
    refused(Call(m, max_rounds=257)(), "max_rounds", "256")
    refused(Call(m, objective=2)(), "objective")
    for bad in (0.0, -1.1, math.nan, math.inf):
        refused(Call(m, grid=[0.8, bad])(), "grid weight 1", "not finite or not above 0")
        refused(Call(m, start=[bad, 1.0])(), "start weight 0", "not finite or not above 0")
        refused(Call(m, grid=[bad], a=(), g=())(), "grid weight 0")   # checked before the empty call is answered
    assert L.lib().anx_debug_fit_stats(None, 7) == L.ANX_EINVAL
    # above 2^24 pairs: a stated limit, checked before a string is read
    big = Call(m)
    assert big(n=(1 << 24) + 1) == L.ANX_ELIMIT and "2^24" in L.last_error()
    lib = L.lib()
    assert lib.anx_fit_confusable_weights_packed(m.h, None, 0, b"abcdeg\0", 7, 1, big.pp, 2, C.byref(big.params), C.byref(big.fp), big.w, big.rounds, None,
                                                 C.byref(big.res)) == L.ANX_EINVAL
    assert lib.anx_debug_fit_confusable_weights_chunk(m.h, big.aa, big.ag, 1, big.pp, 2, C.byref(big.params), C.byref(big.fp), big.w, big.rounds, None,
                                                      C.byref(big.res), 0) == L.ANX_ENODEVICE   # (the model is asked first; a device-resident model gets EINVAL for chunk 0)
    # n == 0: no build, no device; zero rounds, zero counts, weights_out = start, the bytes behind them left alone, the stats not moved
    fresh = hand_model_no_device(tmp_path)
    before = A.VariantModel.fit_stats()
    assert list(before) == STATS
    c = Call(fresh, start=[0.9, 1.0], a=(), g=())
    assert c(a=None, g=None) == L.ANX_OK
    assert bytes(c.res) == bytes(64) and list(c.w)[:3] == [0.9, 1.0, 7.0]
    c = Call(fresh, a=(), g=())
    assert c() == L.ANX_OK and list(c.w)[:3] == [1.0, 1.0, 7.0]
    w, rounds, res, trials = fresh.fit_confusables_arrays([], [], pats, p, [0.8, 1.25], start=[1.1, 1.0], with_trials=True)
    assert list(w) == [1.1, 1.0] and len(rounds) == 0 and res.tobytes() == bytes(64) and trials.shape == (0, 2, 2)
    d = fresh.fit_confusables([], [], pats, p, [0.8, 1.25], start=[1.1, 1.0])
    assert d["weights"] == {"-[y]+[i]": 1.1} and d["rounds"] == [] and d["stop"] == "converged" and d["start"]["mrr"] == 0.0 and d["final"]["at1"] == 0
    assert A.VariantModel.fit_stats() == before


def test_models_the_fit_refuses(tmp_path):
    """Built host-only models: the refusal comes before the device is asked for, with the confusable sweep's wording where it is the sweep's."""
    p, pats = A.SearchParameters(max_anagram_distance=2, max_edit_distance=1, max_matches=3), ["-[y]+[i]"]

    def fit(m, **kw):
        return m.fit_confusables_arrays(["abcdef"], ["abcdeg"], pats, p, [1.1], **kw)

    lists = hand_model_no_device(tmp_path)
    lists.add_variant(3, "abcdefx", 0.9)
    lists.build()
    with pytest.raises(A.AnxError) as e:
        fit(lists)
    assert e.value.code == L.ANX_EINVAL and "confusable sweep: the model has a variant list" in str(e.value)
    conf = hand_model_no_device(tmp_path)
    conf.add_to_confusables("-[y]+[i]", 1.1)
    conf.build()
    with pytest.raises(A.AnxError) as e:
        fit(conf, packed=False)
    assert e.value.code == L.ANX_EINVAL and "confusable sweep: the model has a confusable list of its own" in str(e.value)
    L.set_switch("ANX_CONFUSABLES", "host")
    try:
        with pytest.raises(A.AnxError) as e:
            fit(conf)
        assert e.value.code == L.ANX_EINVAL and "weighted on the host" in str(e.value)
    finally:
        L.set_switch("ANX_CONFUSABLES", None)
    early = hand_model_no_device(tmp_path)
    early.set_confusables_before_pruning()
    early.build()
    with pytest.raises(A.AnxError) as e:
        fit(early)
    assert e.value.code == L.ANX_EINVAL and "before pruning" in str(e.value) and "late" in str(e.value)
    zero = hand_model_no_device(tmp_path, A.Weights(ld=0, lcs=0, prefix=0, suffix=0, case=0))
    zero.build()
    with pytest.raises(A.AnxError) as e:
        fit(zero)
    assert e.value.code == L.ANX_EINVAL and "own weights" in str(e.value)
    plain = hand_model_no_device(tmp_path)
    plain.build()
    with pytest.raises(A.AnxError) as e:
        fit(plain)
    assert e.value.code == L.ANX_ENODEVICE


def test_python_layer_argument_errors(tmp_path):
    m = hand_model_no_device(tmp_path)
    p, pats = A.SearchParameters(), ["-[y]+[i]", "+[e]"]
    with pytest.raises(ValueError):
        m.fit_confusables_arrays(["a"], [], pats, p, [1.1])
    with pytest.raises(ValueError):
        m.fit_confusables_arrays(["a"], ["a"], pats, p, [1.1], start=[1.0])
    with pytest.raises(ValueError):
        m.fit_confusables_arrays(["a"], ["a"], pats, p, [1.1], objective="f1")
    with pytest.raises(ValueError):
        m.fit_confusables_arrays(["a"], ["a"], pats, p, [1.1], min_gain=-1)
    with pytest.raises(ValueError):
        m.fit_confusables_arrays(["a"], ["a"], pats, p, [1.1], min_gain=0.5)   # acc1 counts pairs
    assert A.VariantModel.fit_min_gain("acc1", 2) == 2 and A.VariantModel.fit_min_gain("mrr", 0.5) == 1 << 31 and A.VariantModel.fit_min_gain("mrr", 0) == 0
    with pytest.raises(A.AnxError) as e:   # max_rounds is the library's to refuse
        m.fit_confusables_arrays([], [], pats, p, [1.1], max_rounds=0)
    assert e.value.code == L.ANX_EINVAL and "max_rounds" in str(e.value)
    s = A.VariantModel.fit_counts_summary({"at1": 3, "ranked": 4, "rr_fixed": 7 << 31}, 8)
    assert (s["accuracy_at_1"], s["ranked_share"], s["mrr"]) == (3 / 8, 0.5, 3.5 / 8)


# ---- the selection of a round -------------------------------------------------------------------------------------------------------------
def table(J, G, fill, **at):
    t = [[fill] * G for _ in range(J)]
    for k, v in at.items():
        j, g = (int(x) for x in k[1:].split("_"))
        t[j][g] = v
    return t


def select(trials, cur, grid, now, objective="acc1", min_gain=1):
    got = A.VariantModel.fit_select(trials, cur, grid, now, objective, min_gain)
    # the twin's selection on the same table
    want = F.greedy(lambda rows: [now] + [trials[j][g] for j in range(len(cur)) for g in range(len(grid)) if grid[g] != cur[j]], len(cur), grid, cur, objective, 1, min_gain)
    assert got == ((want["rounds"][0][0], want["rounds"][0][1]) if want["rounds"] else (-1, -1))
    return got


def test_select_on_hand_made_tables():
    grid, ones, now = [0.8, 1.25], [1.0, 1.0, 1.0], (5, 9, 100)
    assert select(table(3, 2, now), ones, grid, now) == (-1, -1)                                      # nothing improves
    assert select(table(3, 2, now, t2_1=(6, 9, 100), t1_0=(6, 9, 100), t1_1=(6, 9, 100)), ones, grid, now) == (1, 0)   # tie: smallest pattern, then smallest grid index
    assert select(table(3, 2, now, t0_1=(6, 9, 90), t2_0=(6, 9, 95)), ones, grid, now) == (2, 0)      # ACC1: at1, then rr_fixed
    assert select(table(3, 2, now, t0_1=(7, 9, 90), t2_0=(6, 9, 195)), ones, grid, now) == (0, 1)
    assert select(table(3, 2, now, t0_1=(7, 9, 90), t2_0=(6, 9, 195)), ones, grid, now, "mrr", 0) == (2, 0)   # MRR: rr_fixed first
    assert select(table(3, 2, now, t0_1=(7, 9, 195), t2_0=(6, 9, 195)), ones, grid, now, "mrr", 0) == (0, 1)  # then at1
    # min_gain: a trial that only improves the second component
    second = table(3, 2, now, t1_1=(5, 9, 101))
    assert select(second, ones, grid, now, min_gain=1) == (-1, -1) and select(second, ones, grid, now, min_gain=0) == (1, 1)
    assert select(table(3, 2, now, t1_1=(7, 9, 100)), ones, grid, now, min_gain=3) == (-1, -1)
    assert select(table(3, 2, now, t1_1=(7, 9, 100)), ones, grid, now, min_gain=2) == (1, 1)
    assert select(table(3, 2, now, t1_1=(5, 9, 100 + 5)), ones, grid, now, "mrr", 6) == (-1, -1)       # MRR: the gain is in rr_fixed
    assert select(table(3, 2, now, t1_1=(4, 9, 100 + 6)), ones, grid, now, "mrr", 6) == (1, 1)
    assert select(table(3, 2, now, t1_1=(9, 9, 99)), ones, grid, now, "mrr", 0) == (-1, -1)
    # the best trial decides: a lesser trial that would pass is not looked at (the best has the larger first component anyway)
    assert select(table(3, 2, (4, 9, 100)), ones, grid, now, min_gain=0) == (-1, -1)                   # every trial is worse
    # a skipped trial (grid[g] == cur[j]) is never chosen, whatever its cell holds
    cur = [0.8, 1.0, 1.25]
    assert select(table(3, 2, now, t0_0=(9, 9, 900), t2_1=(9, 9, 900)), cur, grid, now) == (-1, -1)
    assert select(table(3, 2, now, t0_0=(9, 9, 900), t2_1=(9, 9, 900), t2_0=(6, 9, 100)), cur, grid, now) == (2, 0)
    assert select(table(1, 1, (9, 9, 900)), [0.8], [0.8], now, min_gain=0) == (-1, -1)                 # no trial at all
    # 64-bit components: no wrap in the gain
    big = (1 << 63) + 5
    assert select(table(1, 1, (1, 1, big + 2)), [1.0], [0.8], (1, 1, big), "mrr", 2) == (0, 0)
    assert select(table(1, 1, (1, 1, 3)), [1.0], [0.8], (1, 1, big), "mrr", 0) == (-1, -1)
    lib, out = L.lib(), C.c_int32(0)
    t, d, cc = (L.FitCounts * 1)(), (C.c_double * 1)(1.0), L.FitCounts()
    assert lib.anx_debug_fit_select(None, d, 1, d, 1, C.byref(cc), 0, 0, C.byref(out), C.byref(out)) == L.ANX_EINVAL
    assert lib.anx_debug_fit_select(t, d, 0, d, 1, C.byref(cc), 0, 0, C.byref(out), C.byref(out)) == L.ANX_EINVAL
    assert lib.anx_debug_fit_select(t, d, 1, d, 17, C.byref(cc), 0, 0, C.byref(out), C.byref(out)) == L.ANX_EINVAL
    assert lib.anx_debug_fit_select(t, d, 1, d, 1, C.byref(cc), 2, 0, C.byref(out), C.byref(out)) == L.ANX_EINVAL


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def test_cli_fit_arguments(tmp_path, capsys):
    a = cli.build_parser().parse_intermixed_args(["sweep", "-a", "a.tsv", "-l", "l.tsv", "--candidates", "c.tsv", "--candidate-weights", "0.8,1.25", "--fit",
                                                  "--fit-objective", "mrr", "--fit-rounds", "5", "--fit-min-gain", "0.25", "--fit-output", "o.tsv", "pairs.tsv"])
    assert a.fit and (a.fit_objective, a.fit_rounds, a.fit_min_gain, a.fit_output) == ("mrr", 5, 0.25, "o.tsv") and cli.fit_args_error(a) is None
    plain = cli.build_parser().parse_intermixed_args(["sweep", "-a", "a.tsv", "--candidates", "c.tsv", "--candidate-weights", "0.8", "pairs.tsv"])
    assert not plain.fit and cli.fit_args_error(plain) is None and cli.fit_min_gain_of(plain) == 1.0   # the table mode is unchanged
    lex = tmp_path / "hand.lexicon"
    lex.write_text("\n".join(E.HAND_WORDS) + "\n")
    pairs = tmp_path / "pairs.tsv"
    pairs.write_text("abcdef\tabcdeg\n")
    cand = tmp_path / "cand.tsv"
    cand.write_text("+[g]\t1.1\n")
    base = ["sweep", "-a", ALPHABET, "-l", str(lex), "--device=-1"]
    for extra, word in ((["--fit"], "--candidates"), (["--fit", "--candidates", str(cand), "--candidate-weights", "0.8", "--early-confusables"], "--early-confusables"),
                        (["--fit", "--candidates", str(cand), "--candidate-weights", "0.8", "--fit-rounds", "0"], "--fit-rounds"),
                        (["--fit", "--candidates", str(cand), "--candidate-weights", "0.8", "--fit-rounds", "257"], "--fit-rounds"),
                        (["--fit", "--candidates", str(cand), "--candidate-weights", "0.8", "--fit-min-gain=-1"], "--fit-min-gain"),
                        (["--fit", "--candidates", str(cand), "--candidate-weights", "0.8", "--fit-min-gain", "0.5"], "--fit-min-gain"),
                        (["--candidates", str(cand), "--candidate-weights", "0.8", "--fit-output", "x.tsv"], "--fit"),
                        (["--fit", "--candidates", str(cand), "--candidate-weights", "0.8", "--grid", "g.tsv"], "--grid")):
        assert cli.main(base + extra + [str(pairs)]) == 2
        assert word in capsys.readouterr().err, extra
    with pytest.raises(SystemExit) as e:   # 17 weights: the grid's limit, before the model is asked for anything
        cli.main(base + ["--fit", "--candidates", str(cand), "--candidate-weights", ",".join(["1.1"] * 17), str(pairs)])
    assert e.value.code == 2 and "16" in capsys.readouterr().err
    # the fitted list is written so that it reads back bit for bit
    text = cli.fit_list_text({"-[y]+[i]": 1.1, "+[e]$": 0.1 + 0.2, "-[a]": 1.25})
    assert text == "-[y]+[i]\t1.1\n+[e]$\t0.30000000000000004\n-[a]\t1.25\n"
    out = tmp_path / "fitted.tsv"
    out.write_text(text)
    m = hand_model_no_device(tmp_path)
    m.read_confusablelist(str(out))
    assert m.confusable_weight_text("abd", "bd") == 1.25 and m.confusable_weight_text("lov", "love").hex() == (0.1 + 0.2).hex()
    c = A.VariantModel.fit_counts_summary({"at1": 1, "ranked": 3, "rr_fixed": 3 << 31}, 4)
    assert cli.fit_tsv_line("-", 1.0, c) == "-\t1\t0.25\t0.375\t3"


# ---- the kernels' resources ----------------------------------------------------------------------------------------------------------------
KEYS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
KERNELS = ("k_fit_gold", "k_fit_state", "k_fit_trials")


@pytest.fixture(scope="module")
def fit_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fit") / "fit.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(CSRC, "fit.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(\S+)\n(.*?)\.wavefront_size:\s+(\d+)", text, re.S):
        ks[m.group(2)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(3)).group(1)) for k in KEYS}
        ks[m.group(2)]["group_segment_fixed_size"], ks[m.group(2)]["wavefront_size"] = int(m.group(1)), int(m.group(4))
    return ks


def test_fit_instantiates_its_own_kernels_only(fit_isa):
    """k_rank, the base run and the mask pass stay their files': fit.hip reaches them through host functions."""
    assert len(fit_isa) == len(KERNELS) and all("k_fit_" in n for n in fit_isa), sorted(fit_isa)


@pytest.mark.parametrize("kernel", KERNELS)
def test_fit_kernels_isa_metadata(fit_isa, kernel):
    """No kernel of fit.hip uses scratch or spills: the trials re-read the rows from the state and keep no per-lane array.  The LDS of
    k_fit_trials is dynamic (sized by the call's patterns x grid), so its fixed size is 0.  Wave64."""
    r = [v for n, v in fit_isa.items() if kernel + "ENS" in n or n.endswith(kernel)]
    assert len(r) == 1, (kernel, sorted(fit_isa))
    r = r[0]
    print(kernel, r)
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (kernel, r)
    assert r["group_segment_fixed_size"] == 0 and r["wavefront_size"] == 64 and r["vgpr_count"] <= 128, (kernel, r)
