"""anx_batch_fetch_measures on the device (analiticcl_amd/csrc/kernels_explain.hpp) against the oracle's per-pair functions: record r
describes row r of fetch_compact(with_via=True) -- the unrestricted Damerau-Levenshtein, the longest common substring, the common
prefix and suffix, the case flag and the lengths of (input, scored entry), the L1 of their symbol counts, and the unweighted distance
score, which on a plain model is the row's dist_score bit for bit.  The scored entry is the row's vocabulary item, or its `via`."""
import collections
import ctypes as C
import json
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import synth
from oracle import cwrap as O

import pairs_conf_common as PC
from test_gpu_score_pairs import edits, expected, letters_of
from variant_models_common import build_pair, hand_made_lists, queries_for

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
DEFAULT_W = (0.5, 0.125, 0.125, 0.125, 0.125)
FIELDS = ("ld", "lcs", "prefixlen", "suffixlen", "len_input", "len_entry", "anagram_distance", "flags", "score")


def plain_model(data_dir, weights=None, lexicon="eng.aspell.lexicon"):
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), weights or A.Weights(), device=0)
    g.read_lexicon(os.path.join(data_dir, lexicon))
    g.build()
    return g


@pytest.fixture(scope="module")
def oracle(data_dir):
    return O.OracleModel(alphabet_path=os.path.join(data_dir, "simple.alphabet.tsv"))


@pytest.fixture(scope="module")
def words(data_dir):
    return synth.load_lexicon_words(os.path.join(data_dir, "eng.aspell.lexicon"))


@pytest.fixture(scope="module")
def eng(data_dir):
    return plain_model(data_dir)


def run_batch(g, qs, p):
    b = g.encode_batch(qs, p)
    b.run()
    return b


def fetch_both(b):
    """(offsets, compact records, via, measures) of a batch that has run; the two calls agree on the offsets"""
    off, rec, via = b.fetch_compact(with_via=True)
    moff, m = b.fetch_measures()
    assert moff.dtype == np.uint32 and np.array_equal(moff, off)
    assert m.shape == rec.shape and m.dtype.itemsize == 16
    return off, rec, via, m


def anagram_l1(o, a, b):
    ca, cb = collections.Counter(o.normalize(a)), collections.Counter(o.normalize(b))
    return sum(abs(ca[k] - cb[k]) for k in set(ca) | set(cb))


def check_rows(g, o, qs, off, rec, via, m, w=DEFAULT_W, memo=None):
    """every record `==` the oracle's measures of (input, text of the scored item); -> the rows' (input index, scored text)"""
    memo = {} if memo is None else memo
    text = {}
    out = []
    for i, q in enumerate(qs):
        for r in range(int(off[i]), int(off[i + 1])):
            has_via = int(via[r]) != NONE
            item = int(via[r]) if has_via else int(rec["vocab_id"][r])
            t = text.get(item)
            if t is None:
                t = text[item] = g.vocab_text(item)
            e = memo.get((q, t))
            if e is None:
                e = memo[(q, t)] = dict(expected(o, q, t, w), l1=anagram_l1(o, q, t))
            got = m[r]
            what = (q[:40], len(q), t[:40], len(t), {k: got[k].item() for k in FIELDS}, e)
            assert e["status"] == 0, what
            assert (got["ld"], got["lcs"], got["prefixlen"], got["suffixlen"]) == (e["ld"], e["lcs"], e["prefixlen"], e["suffixlen"]), what
            assert (got["len_input"], got["len_entry"]) == (e["len_a"], e["len_b"]), what
            assert got["anagram_distance"] == e["l1"], what
            assert got["flags"] == (1 if e["samecase"] else 0) | (2 if has_via else 0), what
            assert got["score"] == e["score"], what
            out.append((i, t))
    return out


def clamped(value, length):
    return min(value, length // 2)


# ---- 1. eng.aspell, default weights ----------------------------------------------------------------------------------------------------
def test_eng_aspell_every_row(eng, oracle, words):
    qs = synth.make_queries(words, 2000, max_len=16, seed=4100)
    edge = ["", "a" * 256, "seperate", "seperate", "recieve", "rec@ive", "@#$%&", "Separate", "separate", "SEPARATE", "1separate", "2nd", "teh", "Teh",
            "internationalisation", "internationalizations", "counterrevolutionaries"]
    qs = qs[:1000] + edge + qs[1000:]
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
    b = run_batch(eng, qs, p)
    off, rec, via, m = fetch_both(b)
    total = int(off[-1])
    assert total > 4000 and bool((via == NONE).all())
    i_empty, i_long = qs.index(""), qs.index("a" * 256)
    assert off[i_empty] == off[i_empty + 1] and off[i_long] == off[i_long + 1]
    for q in ("seperate", "rec@ive", "Separate", "1separate", "internationalisation"):
        i = qs.index(q)
        assert off[i + 1] > off[i], q   # the edge inputs have rows to describe
    rows = check_rows(eng, oracle, qs, off, rec, via, m)
    assert np.array_equal(m["score"], rec["dist_score"])   # operator ==, every row
    klen = np.repeat(np.array([clamped(3, len(oracle.normalize(q))) if 0 < len(q) <= 255 else 0 for q in qs]), np.diff(off.astype(np.int64)))
    assert bool((m["anagram_distance"] <= klen).all())
    assert int((m["len_entry"] > 16).sum()) >= 1 and int((m["len_input"] > 16).sum()) >= 1   # the long kernel took part
    assert int((m["flags"] & 1 == 0).sum()) >= 1 and int((m["flags"] & 1).sum()) >= 1
    i = qs.index("seperate")
    assert m[off[i]:off[i + 1]].tobytes() == m[off[i + 1]:off[i + 2]].tobytes()   # the duplicate
    mc = m.copy()
    # direct rows against the debug dump of every scored pair (it re-runs the batch)
    by_pair = {(q, v): (ld, lcs, pre, suf, same, sc) for q, v, ld, lcs, pre, suf, same, sc in b.fetch_pairs()}
    assert len(by_pair) > total
    for r, (i, _t) in enumerate(rows):
        e = by_pair[(i, int(rec["vocab_id"][r]))]
        assert (mc["ld"][r], mc["lcs"][r], mc["prefixlen"][r], mc["suffixlen"][r], mc["flags"][r] & 1, mc["score"][r]) == e, (qs[i], r, e)
    b.free()


# ---- 2. a hand-made lexicon: every tier, every boundary -------------------------------------------------------------------------------
TIER_LENGTHS = (1, 15, 16, 17, 32, 33, 64, 65, 200, 255)


def tier_lexicon_and_queries():
    rng = random.Random(4200)
    entries, queries = [], []
    for n in TIER_LENGTHS:
        for _ in range(3):
            e = letters_of(rng, n)
            entries.append(e)
            queries.append(e)
            if n > 1:
                queries.append(edits(rng, e, rng.randint(1, 4), "abc", max_len=255)[:255])
                queries.append(e[1:])        # one symbol shorter: 16/17, 17/16, 32/33, 64/65 pairs
                queries.append((e + "a")[:255])
    # transpositions across a gap (alone, and behind a common prefix that is long enough for d >= 2), repeated symbols
    entries += ["abc", "ca", "abcd", "dabc", "aab", "aba", "abab", "baba", "ccccccabc", "ccccccca", "ccccabcd", "ccccdabc", "aaaaaaaa", "aaaaaaaaaaaaaaaaaa"]
    queries += ["abc", "ca", "abcd", "dabc", "aab", "abab", "baba", "ccccccabc", "ccccccca", "ccccabcd", "ccccdabc", "aaaaaaa", "aaaaaaaaaaaaaaaaa"]
    s16 = "abcabcabcabcabca"
    entries += [s16, s16 + "b"]
    queries += ["bacabcabcabcabca", "bacabcabcabcabca" + "b", s16[:15]]
    return sorted(set(entries)), queries


def test_tiers_on_a_hand_made_lexicon(data_dir, oracle, tmp_path):
    entries, qs = tier_lexicon_and_queries()
    lex = tmp_path / "tiers.lexicon"
    lex.write_text("\n".join(entries) + "\n")
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g.read_lexicon(str(lex))
    g.build()
    p = A.SearchParameters(max_anagram_distance=8, max_edit_distance=8, max_matches=0, score_threshold=0.0, cutoff_threshold=0.0)
    assert [len(q) for q in qs] != sorted(len(q) for q in qs)   # the batch sorts its queries by length: q_orig is not the identity
    b = run_batch(g, qs, p)
    off, rec, via, m = fetch_both(b)
    rows = check_rows(g, oracle, qs, off, rec, via, m)
    assert np.array_equal(m["score"], rec["dist_score"])
    li, le = m["len_input"].astype(int), m["len_entry"].astype(int)
    longest = np.maximum(li, le)
    for lo, hi in ((1, 16), (17, 32), (33, 64), (65, 128), (129, 255)):
        assert int(((longest >= lo) & (longest <= hi)).sum()) >= 1, (lo, hi)
    assert int(((li == 16) & (le == 17)).sum()) >= 1 and int(((li == 17) & (le == 16)).sum()) >= 1
    assert int(((li == 255) & (le == 255)).sum()) >= 1 and int((m["ld"] >= 3).sum()) >= 1
    pairs = {(qs[i], t): int(m["ld"][r]) for r, (i, t) in enumerate(rows)}
    assert pairs[("ccccabcd", "ccccdabc")] == 2 and pairs[("abcd", "dabc")] == 2 and pairs[("ccccccabc", "ccccccca")] == 2
    b.free()


# ---- 3. weights with zeros: every measure is computed whatever its weight ------------------------------------------------------------------
def test_weights_with_zeros(data_dir, oracle, words):
    g = plain_model(data_dir, A.Weights(ld=1, lcs=0, prefix=0.5, suffix=0, case=0))
    qs = synth.make_queries(words, 300, max_len=16, seed=4300) + ["Separate", "seperate", "internationalisation"]
    b = run_batch(g, qs, A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10))
    off, rec, via, m = fetch_both(b)
    assert int(off[-1]) > 500
    check_rows(g, oracle, qs, off, rec, via, m, w=(1.0, 0.0, 0.5, 0.0, 0.0))
    assert np.array_equal(m["score"], rec["dist_score"])
    assert int((m["lcs"] > 0).sum()) > 500 and int((m["suffixlen"] > 0).sum()) >= 1 and int((m["flags"] & 1).sum()) >= 1
    b.free()


# ---- 4. variant lists: the scored entry is the via item ---------------------------------------------------------------------------------------
def test_variant_lists(data_dir, oracle, words, tmp_path):
    lists = hand_made_lists(tmp_path, words)
    g = build_pair(data_dir, lists, want_oracle=False)[0]
    qs = queries_for(words, lists, 200, seed=4400)
    b = run_batch(g, qs, A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=20))
    off, rec, via, m = fetch_both(b)
    has_via = via != NONE
    assert int(has_via.sum()) >= 5 and int((~has_via).sum()) >= 100
    assert np.array_equal((m["flags"] & 2) != 0, has_via)   # bit 1 exactly on the rows with a via
    check_rows(g, oracle, qs, off, rec, via, m)
    assert np.array_equal(m["score"][~has_via], rec["dist_score"][~has_via])
    transparent = 0
    for r in np.nonzero(has_via)[0].tolist():
        # k_compact: dist_score = (score of the via item) * (variant score of its reference to the row's item)
        refs = [s for kind, v, s in g.variants(int(via[r])) if kind == "VariantOf" and v == int(rec["vocab_id"][r])]
        assert refs and any(m["score"][r] * s == rec["dist_score"][r] for s in refs), (g.vocab_text(int(via[r])), g.vocab_text(int(rec["vocab_id"][r])), refs)
        transparent += bool(g.vocabtype(int(via[r])) & 4)
    assert transparent >= 1
    b.free()


# ---- 5. confusables, late and early ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("early", [False, True])
def test_confusables(data_dir, oracle, early):
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g.read_lexicon(os.path.join(data_dir, "nld.aspell.lexicon"))
    PC.load_patterns(g)
    if early:
        g.set_confusables_before_pruning()
    g.build()
    nld = synth.load_lexicon_words(os.path.join(data_dir, "nld.aspell.lexicon"))
    qs = synth.make_queries(nld, 400, seed=41) + ["huys", "cyrkel", "sien"]
    b = run_batch(g, qs, A.SearchParameters())
    off, rec, via, m = fetch_both(b)
    assert int(off[-1]) > 1000 and bool((via == NONE).all())
    rows = check_rows(g, oracle, qs, off, rec, via, m)
    weighted = 0
    for r, (i, t) in enumerate(rows):
        w = g.confusable_weight_text(qs[i], t)
        assert m["score"][r] * w == rec["dist_score"][r], (qs[i], t, w)
        weighted += w != 1.0
    assert weighted >= 1
    b.free()
    A.set_switch("ANX_CONFUSABLES", "host")
    try:
        b = run_batch(g, qs[:50], A.SearchParameters())
        with pytest.raises(A.AnxError) as e:
            b.fetch_measures()
        assert e.value.code == L.ANX_EINVAL
        b.free()
    finally:
        A.set_switch("ANX_CONFUSABLES", None)


# ---- 6. several shards ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["length", "range"])
def test_two_replicas_equal_one(data_dir, eng, words, policy):
    qs = synth.make_queries(words, 600, max_len=16, seed=4600) + ["internationalisation", "", "seperate"]
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
    b = run_batch(eng, qs, p)
    off1, rec1, via1, m1 = fetch_both(b)
    off1, m1 = off1.copy(), m1.copy()
    b.free()
    A.set_switch("ANX_SHARD_MIN", 64)
    A.set_switch("ANX_SHARD_POLICY", policy)
    try:
        g = plain_model(data_dir)
        g.to_devices([0, 0])
        b = run_batch(g, qs, p)
        assert len(b.shards()) == 2 and (b.shard_inputs(0) is not None) == (policy == "length")
        off, rec, via, m = fetch_both(b)
        assert np.array_equal(off, off1) and m.tobytes() == m1.tobytes() and int(off[-1]) > 1000
        b.free()
    finally:
        A.set_switch("ANX_SHARD_MIN", None)
        A.set_switch("ANX_SHARD_POLICY", None)


# ---- 7. error cases and re-runs ---------------------------------------------------------------------------------------------------------------
def test_errors_and_reruns(eng, oracle, words):
    qs = synth.make_queries(words, 200, max_len=16, seed=4700)
    p1 = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
    b = eng.encode_batch(qs, p1)
    with pytest.raises(A.AnxError) as e:   # not run yet
        b.fetch_measures()
    assert e.value.code == L.ANX_EINVAL
    rows, offs = C.c_void_p(), C.POINTER(C.c_uint32)()
    assert L.lib().anx_batch_fetch_measures(None, C.byref(rows), C.byref(offs)) == L.ANX_EINVAL
    assert L.lib().anx_batch_fetch_measures(b.h, None, C.byref(offs)) == L.ANX_EINVAL
    assert L.lib().anx_batch_fetch_measures(b.h, C.byref(rows), None) == L.ANX_EINVAL
    b.run()
    off, rec, via, m = fetch_both(b)
    first = (off.copy(), m.copy())
    b.free()
    # the same inputs under other parameters: the measures describe the run they follow
    p2 = A.SearchParameters(max_anagram_distance=2, max_edit_distance=1, max_matches=3)
    b = run_batch(eng, qs, p2)
    off, rec, via, m = fetch_both(b)
    assert int(off[-1]) < int(first[0][-1]) and int(m["ld"].max()) <= 1 and int(first[1]["ld"].max()) == 2
    check_rows(eng, oracle, qs, off, rec, via, m)
    assert np.array_equal(m["score"], rec["dist_score"])
    b.free()
    # no rows at all
    none = ["qqqqqqqqqqqqqqzzzzzzzzzzzzzz", "", "xjxjxjxjxjxjxjxjxjxjxjxjxjxjxj"]
    b = run_batch(eng, none, p2)
    off, m = b.fetch_measures()
    assert off.tolist() == [0, 0, 0, 0] and len(m) == 0
    b.free()


def test_two_threads_two_batches(eng, words):
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
    sets = [synth.make_queries(words, 400, max_len=20, seed=4800 + t) for t in range(2)]
    want = []
    for qs in sets:
        b = run_batch(eng, qs, p)
        off, m = b.fetch_measures()
        want.append((off.copy(), m.copy()))
        b.free()
    errors = []

    def work(t):
        try:
            b = run_batch(eng, sets[t], p)
            for _ in range(5):
                off, m = b.fetch_measures()
                if not np.array_equal(off, want[t][0]) or m.tobytes() != want[t][1].tobytes():
                    errors.append((t, "differs"))
            b.free()
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[:3]


# ---- 8. explain_variants and query --explain ---------------------------------------------------------------------------------------------------
def test_explain_variants_and_command_line(eng, data_dir, tmp_path):
    qs = ["seperate", "recieve", "Teh", "", "internationalisation", 'quo"te']
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
    plain = eng.find_variants_par(qs, p)
    got = eng.explain_variants(qs, p)
    assert [r["input"] for r in got] == qs and sum(len(r["variants"]) for r in got) > 10
    for a, e in zip(plain, got):
        assert len(a["variants"]) == len(e["variants"])
        for va, ve in zip(a["variants"], e["variants"]):
            assert set(ve) == set(va) | set(A.VariantModel.EXPLAIN_KEYS) and all(ve[k] == va[k] for k in va)
            assert ve["unweighted_score"] == ve["dist_score"] and isinstance(ve["samecase"], bool)
    top = got[0]["variants"][0]
    assert (top["text"], top["ld"], top["len_input"], top["len_entry"], top["anagram_distance"]) == ("separate", 1, 8, 8, 2)
    src = tmp_path / "in.txt"
    src.write_text("\n".join(qs) + "\n", encoding="utf-8")
    base = [sys.executable, "-m", "analiticcl_amd", "query", "--alphabet", os.path.join(data_dir, "simple.alphabet.tsv"), "--lexicon",
            os.path.join(data_dir, "eng.aspell.lexicon"), "--device", "0"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONIOENCODING="utf-8")
    js = subprocess.run(base + ["--json", "--explain", str(src)], cwd=REPO, env=env, capture_output=True, text=True, encoding="utf-8", timeout=300)
    assert js.returncode == 0, js.stderr[-2000:]
    items = json.loads(js.stdout)
    assert [it["input"] for it in items] == qs
    for it, e in zip(items, got):
        assert len(it["variants"]) == len(e["variants"])
        for v, ve in zip(it["variants"], e["variants"]):
            assert v["text"] == ve["text"] and all(k in v for k in A.VariantModel.EXPLAIN_KEYS)
            assert (v["ld"], v["lcs"], v["samecase"], v["anagram_distance"]) == (ve["ld"], ve["lcs"], ve["samecase"], ve["anagram_distance"])
    tsv = subprocess.run(base + ["--explain", str(src)], cwd=REPO, env=env, capture_output=True, text=True, encoding="utf-8", timeout=300)
    assert tsv.returncode == 0, tsv.stderr[-2000:]
    lines = tsv.stdout.split("\n")
    assert lines[-1] == "" and len(lines) == len(qs) + 1
    f = lines[0].split("\t")
    assert f[0] == "seperate" and f[1] == "separate" and f[3:6] == ["1", str(top["lcs"]), str(top["prefixlen"])]
