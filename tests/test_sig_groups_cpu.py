"""The search for the signature's symbol groups (host_model.cpp, search_sig_groups), on models without a device.

Any partition of the count-vector slots is exact; the search only has to be deterministic, keep the constraints the kernels rely on
(group index below the group count, no group sum above the greedy partition's largest), leave the greedy partition alone when it is
switched off (ANX_SIG_SEARCH=0: the groups of the commit before the search, recorded in tests/golden/sig_groups_greedy.json), survive an
index image, and pay: fewer lexicon records inside the signature ball of held-out queries.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def signature(m, text):
    s = C.c_uint64()
    L.check(L.lib().anx_debug_signature(m.h, text.encode("utf-8"), C.byref(s)))
    return [(s.value >> (8 * i)) & 0xFF for i in range(8)]


def alphabet_symbols(data_dir):
    """The first member of every class of the golden alphabet: one string per count-vector slot."""
    with open(os.path.join(data_dir, "simple.alphabet.tsv"), encoding="utf-8") as f:
        first = [line.split("\t")[0] for line in f.read().split("\n") if line]
    return [{"\\s": " ", "\\t": "\t", "\\n": "\n"}.get(x, x) for x in first]


def groups_of(m, symbols):
    out = []
    for sym in symbols:
        sig = signature(m, sym)
        assert sum(sig) == 1, sym
        out.append(sig.index(1))
    return out


def build(data_dir, lex, search, sig_groups=None):
    A.set_switch("ANX_SIG_SEARCH", search)
    if sig_groups is not None:
        A.set_switch("ANX_SIG_GROUPS", sig_groups)
    try:
        m = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=-1)
        m.read_lexicon(os.path.join(data_dir, f"{lex}.aspell.lexicon"))
        m.build()
    finally:
        A.set_switch("ANX_SIG_SEARCH", None)
        A.set_switch("ANX_SIG_GROUPS", None)
    return m


@pytest.fixture(scope="module")
def models(data_dir):
    return {(lex, s): build(data_dir, lex, s) for lex in ("eng", "nld") for s in (0, 1)}


@pytest.fixture(scope="module")
def word_signatures(models, data_dir):
    """Per model of the eng lexicon: (lengths, signatures) of every lexicon word, computed once."""
    words = synth.load_lexicon_words(os.path.join(data_dir, "eng.aspell.lexicon"))
    lens = np.array([len(w) for w in words], dtype=np.int16)
    return words, lens, {s: np.array([signature(models[("eng", s)], w) for w in words], dtype=np.int16) for s in (0, 1)}


def test_two_builds_give_identical_groups(models, data_dir):
    syms = alphabet_symbols(data_dir)
    for lex in ("eng", "nld"):
        again = build(data_dir, lex, 1)
        assert groups_of(again, syms) == groups_of(models[(lex, 1)], syms)
    assert groups_of(models[("eng", 1)], syms) != groups_of(models[("eng", 0)], syms)  # the search does move slots


def test_one_thread_gives_the_same_groups(models, data_dir):
    """The thread count is fixed when the library is first used, so a fresh process pinned to one CPU builds the model again."""
    import subprocess
    import sys
    code = ("import os, sys, json; os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]}); sys.path[:0] = [%r, %r]\n"
            "import test_sig_groups_cpu as T\n"
            "print(json.dumps(T.groups_of(T.build(%r, 'eng', 1), T.alphabet_symbols(%r))))\n"
            % (os.path.dirname(GOLDEN), os.path.dirname(os.path.dirname(GOLDEN)), data_dir, data_dir))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout
    assert json.loads(out.strip().splitlines()[-1]) == groups_of(models[("eng", 1)], alphabet_symbols(data_dir))


def test_every_group_is_below_the_group_count(models, data_dir):
    syms = alphabet_symbols(data_dir)
    for m in models.values():
        g = groups_of(m, syms)
        assert max(g) < 8 and len(set(g)) == 8  # every group stays in use
    for n in (5, 7):
        g = groups_of(build(data_dir, "eng", 1, sig_groups=n), syms)
        assert max(g) == n - 1 and len(set(g)) == n
    assert set(groups_of(build(data_dir, "eng", 1, sig_groups=1), syms)) == {0}


def test_no_group_sum_exceeds_the_greedy_maximum(models, word_signatures, data_dir):
    _words, _lens, sigs = word_signatures
    assert sigs[1].max() <= sigs[0].max()
    words = synth.load_lexicon_words(os.path.join(data_dir, "nld.aspell.lexicon"))
    mx = {s: max(max(signature(models[("nld", s)], w)) for w in words) for s in (0, 1)}
    assert mx[1] <= mx[0]


def test_switch_off_reproduces_the_greedy_groups(models, data_dir):
    with open(os.path.join(GOLDEN, "sig_groups_greedy.json"), encoding="utf-8") as f:
        want = json.load(f)
    syms = alphabet_symbols(data_dir)
    assert want["symbols"] == syms
    for lex in ("eng", "nld"):
        assert groups_of(models[(lex, 0)], syms) == want[lex], lex


def test_fewer_records_in_the_ball_of_held_out_queries(models, word_signatures):
    """Mean number of lexicon words with |len diff| <= 3 and L1(sig) <= 3 over 2 000 synth.make_queries queries the search never saw:
    searched <= 0.90 x greedy (measured: 0.827)."""
    words, lens, sigs = word_signatures
    qs = synth.make_queries(words, 2000, max_len=16, seed=12345)
    mean = {}
    for s in (0, 1):
        # distinct (length, signature) rows with their word counts
        rows, counts = np.unique(np.concatenate([lens[:, None], sigs[s]], axis=1), axis=0, return_counts=True)
        total = 0
        for q in qs:
            qsig = np.array(signature(models[("eng", s)], q), dtype=np.int16)
            sel = np.abs(rows[:, 0] - len(q)) <= 3
            total += int(counts[sel][np.abs(rows[sel, 1:] - qsig).sum(axis=1) <= 3].sum())
        mean[s] = total / len(qs)
    print(f"ball population per query: greedy {mean[0]:.1f}, searched {mean[1]:.1f}, ratio {mean[1] / mean[0]:.3f}")
    assert mean[1] <= 0.90 * mean[0], mean


def test_index_image_keeps_the_groups(models, data_dir, tmp_path):
    syms = alphabet_symbols(data_dir)
    img = str(tmp_path / "eng.anxidx")
    models[("eng", 1)].save_index(img)
    A.set_switch("ANX_SIG_SEARCH", 0)  # a loaded image runs no search and no greedy assignment either: the groups are the file's
    try:
        m2 = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=-1)
        m2.load_index(img)
    finally:
        A.set_switch("ANX_SIG_SEARCH", None)
    assert groups_of(m2, syms) == groups_of(models[("eng", 1)], syms)
    for w in ("separate", "it's", "Zürich", "qqqq"):
        assert signature(m2, w) == signature(models[("eng", 1)], w)
