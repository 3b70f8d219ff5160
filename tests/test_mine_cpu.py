"""anx_mine_confusables without a device (ANX_MINE=host: every pair through the host core): the table and the site list `==` the twin
(tests/mine_twin.py over oracle/sesdiff_twin.py) on 20 000 seeded pairs for context 0, 1, 2 x anchors off / on, with and without
counts; the packed and the pointer form; count sums beyond 2^32; the `mine` command line and the confusable list it writes; the exports
and their ctypes entries."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli, synth
from oracle.sesdiff_twin import Confusable
import mine_twin as MT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("anx_mine_confusables", "anx_mine_confusables_packed", "anx_mine_result_free", "anx_default_mine_params", "anx_debug_mine_stats",
         "anx_debug_mine_chunk", "anx_format_confusable_list")


@pytest.fixture(scope="module")
def host_mode():
    L.set_switch("ANX_MINE", "host")
    yield
    L.set_switch("ANX_MINE", None)


@pytest.fixture(scope="module")
def model(data_dir, host_mode):
    return A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=-1)  # never built, no device


@pytest.fixture(scope="module")
def pairs(data_dir):
    eng = synth.load_lexicon_words(os.path.join(data_dir, "eng.aspell.lexicon"))
    nld = synth.load_lexicon_words(os.path.join(data_dir, "nld.aspell.lexicon"))
    return MT.random_pairs(eng, nld, 20000)


def test_exports_and_ctypes_entries():
    with open(os.path.join(REPO, "include", "anx.h"), encoding="utf-8") as f:
        header = f.read()
    lib = L.lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
    assert C.sizeof(L.MineSite) == 32 and C.sizeof(L.MineParams) == 16
    mp = L.MineParams(9, 9, 9, 9)
    lib.anx_default_mine_params(C.byref(mp))
    assert (mp.context, mp.anchors, mp.no_sites) == (0, 0, 0)
    assert lib.anx_abi_version() == 3


@pytest.mark.parametrize("context,anchors", MT.GRID)
@pytest.mark.parametrize("counted", [False, True])
def test_random_pairs_equal_the_twin(model, pairs, context, anchors, counted):
    pr, counts = pairs
    cnt = counts if counted else None
    a, b = [x for x, _ in pr], [y for _, y in pr]
    before = A.VariantModel.mine_stats()
    got = MT.lib_result(model.mine_confusables_arrays(a, b, cnt, context=context, anchors=anchors, sites=True))
    want = MT.twin_result(pr, cnt, context, anchors)
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    after = A.VariantModel.mine_stats()
    assert after["host_pairs"] - before["host_pairs"] == len(pr) and after["device_pairs"] == before["device_pairs"]
    assert after["sites"] - before["sites"] == len(want[2]) and after["odd_shape_pairs"] == before["odd_shape_pairs"]


def test_pointer_form_dicts_and_no_sites(model, pairs):
    pr = pairs[0][:500]
    a, b = [x for x, _ in pr], [y for _, y in pr]
    want = MT.twin_result(pr, None, 1, True)
    r = model.mine_confusables_arrays(a, b, context=1, anchors=True, sites=True, packed=False)
    assert MT.lib_result(r) == want
    r = model.mine_confusables_arrays(a, b, context=1, anchors=True, sites=False)
    assert MT.lib_result(r, with_sites=False) == want[0] and "site" not in r and r["n_sites"] == len(want[2])
    table, lists = model.mine_confusables(a, b, context=1, anchors=True, sites=True)
    assert [(t["pattern"], t["count"], t["sites"], t["representable"]) for t in table] == [(t, c, s, not f) for t, c, s, f in want[0]]
    assert [len(x) for x in lists] == [want[1][i + 1] - want[1][i] for i in range(len(pr))]
    flat = [(p, s["a_pos"], s["a_len"], s["b_pos"], s["b_len"], s["pattern"], (1 if s["first"] else 0) | (2 if s["last"] else 0))
            for p, l in enumerate(lists) for s in l]
    assert flat == want[2]
    assert model.mine_confusables(a, b, context=1, anchors=True) == table


def test_hand_pairs(model):
    pr = [("huys", "huis"), ("huis", "huis"), ("", "abc"), ("abc", ""), ("", ""), ("abcd", "abdc"), ("xhuysx", "yhuisy"), ("café", "cafe"),
          ("a]b", "a[b"), ("a|b", "ab"), ("abcabc", "abdabd"), ("𝔘nicode", "unicode"), ("é" * 70 + "x", "é" * 70 + "y")]
    a, b = [x for x, _ in pr], [y for _, y in pr]
    for context, anchors in MT.GRID:
        got = MT.lib_result(model.mine_confusables_arrays(a, b, context=context, anchors=anchors, sites=True))
        assert got == MT.twin_result(pr, None, context, anchors), (context, anchors)
    table = model.mine_confusables(a, b)
    assert {t["pattern"] for t in table if not t["representable"]} == {"-[]]+[[]", "-[|]"}


def test_counts_beyond_32_bits(model):
    a, b = ["huys", "huys", "cat", "huys"], ["huis", "huis", "kat", "huis"]
    r = model.mine_confusables(a, b, counts=[0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFF])
    assert r == [{"pattern": "-[y]+[i]", "count": 3 * 0xFFFFFFFF, "sites": 3, "representable": True},
                 {"pattern": "-[c]+[k]", "count": 0, "sites": 1, "representable": True}]
    assert 3 * 0xFFFFFFFF > 1 << 33


def test_argument_errors(model):
    with pytest.raises(L.AnxError):
        model.mine_confusables(["a"], ["b"], context=9)
    with pytest.raises(ValueError):
        model.mine_confusables(["a"], ["b", "c"])
    assert model.mine_confusables([], []) == []


def test_cli_parser_accepts_mine():
    a = cli.build_parser().parse_intermixed_args(["mine", "--alphabet", "x.tsv", "--context", "2", "--anchors", "--as-confusables", "0.9",
                                                  "--min-count", "3", "--json", "pairs.tsv"])
    assert (a.mode, a.context, a.anchors, a.as_confusables, a.min_count, a.json, a.files) == ("mine", 2, True, 0.9, 3, True, ["pairs.tsv"])
    a = cli.build_parser().parse_intermixed_args(["mine", "-a", "x.tsv"])
    assert (a.context, a.anchors, a.as_confusables, a.min_count) == (0, False, None, 1)


def test_cli_table_and_confusable_list(data_dir, tmp_path, pairs, monkeypatch, host_mode):
    pr = pairs[0][:2000] + [("a]b", "a[b")]
    src = tmp_path / "pairs.tsv"
    src.write_text("".join(f"{a}\t{b}\t{2 if k % 3 == 0 else 1}\n" for k, (a, b) in enumerate(pr)), encoding="utf-8")
    counts = [2 if k % 3 == 0 else 1 for k in range(len(pr))]
    alphabet = os.path.join(data_dir, "simple.alphabet.tsv")

    def run(*opts):
        out = io.StringIO()
        monkeypatch.setattr(cli.sys, "stdout", out)
        try:
            assert cli.main(["mine", "--alphabet", alphabet, str(src), *opts]) == 0
        finally:
            monkeypatch.undo()
            L.set_switch("ANX_MINE", "host")  # (main set it; the module's fixture resets it at the end)
        return out.getvalue()

    want = MT.twin_result(pr, counts, 1, True)[0]
    assert run("--context", "1", "--anchors") == "".join(f"{t}\t{c}\t{s}\n" for t, c, s, _f in want)
    listed = run("--context", "1", "--anchors", "--as-confusables", "0.9", "--min-count", "2")
    rows = [line.split("\t") for line in listed.splitlines()]
    assert [r[0] for r in rows] == [t for t, c, _s, f in want if c >= 2 and not f]
    assert rows and all(float(r[1]) == 0.9 for r in rows)
    for text, _w in rows:  # the reference's parser reads every line back into the instructions it was written from
        c = Confusable(text, 0.9)
        assert "".join(f"{op}[{'|'.join(opts)}]" for op, opts in c.instructions) == text.strip("^$")
        assert (c.strictbegin, c.strictend) == (text.startswith("^"), text.endswith("$"))
    m = A.VariantModel(alphabet, A.Weights(), device=-1)
    lst = tmp_path / "mined.confusables.tsv"
    lst.write_text(listed, encoding="utf-8")
    m.read_confusablelist(str(lst))  # and so does the library's
