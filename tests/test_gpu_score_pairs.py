"""anx_score_pairs on the device (analiticcl_amd/csrc/pairs.hip) against the oracle's per-pair functions: the unrestricted
Damerau-Levenshtein without a distance bound (src/distance.rs:101-179 with max_distance 255), the longest common substring, the
common prefix and suffix, the case flag, and the distance score of src/lib.rs:1433-1452 -- which for a pair find_variants ranks
has to be the row's dist_score bit for bit.  Both tiers (a pair per lane for sides of at most 16 bytes, a pair per wave above)
answer every question here; out[i] is pair i whatever tier it took."""
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
from analiticcl_amd import cli, synth
from oracle import cwrap as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURES = ("ld", "lcs", "prefixlen", "suffixlen", "len_a", "len_b", "samecase", "status")
SHORT_BYTES = 16


@pytest.fixture(scope="module")
def eng(data_dir):
    g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
    g.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    g.build()
    o = O.OracleModel(alphabet_path=os.path.join(data_dir, "simple.alphabet.tsv"))
    words = synth.load_lexicon_words(os.path.join(data_dir, "eng.aspell.lexicon"))
    return g, o, words


def nbytes(s):
    return len(s.encode("utf-8"))


def is_short(a, b):
    return nbytes(a) <= SHORT_BYTES and nbytes(b) <= SHORT_BYTES


def expected(o, a, b, w=(0.5, 0.125, 0.125, 0.125, 0.125)):
    """What the oracle's per-pair functions say about (a, b), and the score of src/lib.rs:1433-1452 in the reference's association."""
    if not a or not b:
        return {"status": L.ANX_EEMPTY}
    if len(a) > 255 or len(b) > 255:  # (only used with one-symbol characters)
        return {"status": L.ANX_ELIMIT}
    na, nb = o.normalize(a), o.normalize(b)
    ld, lcs, pre, suf = O.dl(na, nb, 255), O.lcs(na, nb), O.prefix(na, nb), O.suffix(na, nb)
    same = a[0].islower() == b[0].islower()
    n = float(len(na))
    ds = 0.0 if ld > len(na) else 1.0 - ld / n
    score = (w[0] * ds + w[1] * (lcs / n) + w[2] * (pre / n) + w[3] * (suf / n) + (w[4] if same else 0.0)) / sum(w)
    return {"status": 0, "ld": ld, "lcs": lcs, "prefixlen": pre, "suffixlen": suf, "len_a": len(na), "len_b": len(nb), "samecase": same,
            "score": score}


def check_against_oracle(g, o, pairs):
    got = g.score_pairs([a for a, _ in pairs], [b for _, b in pairs])
    assert len(got) == len(pairs)
    for (a, b), r in zip(pairs, got):
        e = expected(o, a, b)
        what = (a[:40], len(a), b[:40], len(b), r, e)
        if e["status"]:
            assert r["status"] == e["status"] and r["score"] == 0.0 and r["ld"] == 0, what
            continue
        for k in MEASURES:
            assert r[k] == e[k], (k,) + what
        assert r["score"] == e["score"], what
    return got


def edits(rng, s, n, letters="abcdefghijklmnopqrstuvwxyz", max_len=40):
    cs = list(s)
    for _ in range(n):
        op = rng.randrange(5)
        if op == 0 and len(cs) > 1:
            del cs[rng.randrange(len(cs))]
        elif op == 1 and len(cs) < max_len:
            cs.insert(rng.randrange(len(cs) + 1), rng.choice(letters))
        elif op == 2:
            cs[rng.randrange(len(cs))] = rng.choice(letters)
        elif len(cs) > 1:  # transpositions twice as often: the term this kernel adds
            p = rng.randrange(len(cs) - 1)
            cs[p], cs[p + 1] = cs[p + 1], cs[p]
    return "".join(cs)


def letters_of(rng, n, alphabet="abc"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def edge_pairs():
    rng = random.Random(77)
    p = []
    # transposition across a gap (expected ld: 2 2 2 3 1)
    p += [("abc", "ca"), ("acb", "ba"), ("abcd", "dabc"), ("abcdef", "badcfe"), ("ab", "ba")]
    # repeated symbols
    p += [("aab", "aba"), ("abab", "baba"), ("aaaa", "aa")]
    # trivial lengths
    p += [("a", "b"), ("separate", "separate"), ("x" * 200, "x" * 200), ("a", "b" * 255), ("b" * 255, "a"), ("a", "a" * 255)]
    # tier boundary: 16/16, 16/17, 17/16 bytes; 9 two-byte characters (9 symbols, 18 bytes)
    s16, t16 = "abcdefghijklmnop", "bacdefghijklmnpo"
    p += [(s16, t16), (s16, t16 + "q"), (s16 + "q", t16), ("é" * 9, "é" * 4 + "a" + "é" * 4), ("éaéaéaéaé", "aéaéaéaéa"), ("abcabcabc", "é" * 9)]
    # wave-step boundaries of the long tier
    for la, lb in ((63, 64), (64, 65), (65, 63), (64, 64), (128, 129), (129, 128), (127, 65), (192, 193)):
        a = letters_of(rng, la)
        p += [(a, letters_of(rng, lb)), (a, edits(rng, a, 9, "abc", max_len=255)[:lb].ljust(lb, "c"))]
    # the largest shapes
    a254 = letters_of(rng, 254, "ab")
    p += [(a254, edits(rng, a254, 12, "ab", max_len=255).ljust(255, "b")[:255]), ("x" * 255, "y" * 255), ("ab" * 127 + "a", "ba" * 127 + "b"),
          (letters_of(rng, 255, "abcdefgh"), letters_of(rng, 255, "abcdefgh"))]
    # statuses; characters outside the alphabet are scored (they are all the unknown symbol)
    p += [("", "abc"), ("abc", ""), ("", ""), ("a" * 256, "abc"), ("abc", "b" * 300), ("", "a" * 256), ("@#$%", "@#%$"), ("\x1b\x01", "ab")]
    # case flag
    p += [("Hello", "hello"), ("hello", "Hello"), ("Hello", "Hallo")]
    return p


def test_edge_table_against_oracle(eng):
    g, o, _ = eng
    pairs = edge_pairs()
    got = {pr: r for pr, r in zip(pairs, check_against_oracle(g, o, pairs))}
    for pr, ld in ((("abc", "ca"), 2), (("acb", "ba"), 2), (("abcd", "dabc"), 2), (("abcdef", "badcfe"), 3), (("ab", "ba"), 1)):
        assert got[pr]["ld"] == ld, pr
    assert got[("x" * 255, "y" * 255)]["ld"] == 255 and got[("x" * 255, "y" * 255)]["lcs"] == 0
    big = got[("ab" * 127 + "a", "ba" * 127 + "b")]
    assert (big["ld"], big["lcs"], big["len_a"], big["len_b"]) == (2, 254, 255, 255)
    assert got[("", "abc")]["status"] == got[("abc", "")]["status"] == L.ANX_EEMPTY
    assert got[("a" * 256, "abc")]["status"] == got[("abc", "b" * 300)]["status"] == L.ANX_ELIMIT
    assert got[("@#$%", "@#%$")]["status"] == 0 and got[("@#$%", "@#%$")]["ld"] == 0  # four times the unknown symbol on either side
    assert got[("Hello", "hello")]["samecase"] is False and got[("Hello", "Hallo")]["samecase"] is True
    assert got[("é" * 9, "é" * 4 + "a" + "é" * 4)]["len_a"] == 9
    # the same symbol sequences give the same answer from either tier: a short pair, and the pair again with a side padded beyond 16 bytes
    a, b = "abcabcab", "bacbacba"
    pad = "q" * 12
    r = g.score_pairs([a, a + pad, pad + a], [b, b + pad, pad + b])
    assert is_short(a, b) and not is_short(a + pad, b + pad)
    assert r[0]["ld"] == r[1]["ld"] == r[2]["ld"] == O.dl(o.normalize(a), o.normalize(b), 255)


def random_pairs(words, n=20000, seed=20240917):
    rng = random.Random(seed)
    qs = synth.make_queries(words, n // 2, max_len=40, seed=seed)
    pairs = [(q, rng.choice(words)[:40]) for q in qs]
    while len(pairs) < n:
        w = "".join(rng.choice(words) for _ in range(rng.choice((1, 1, 2, 3))))[:40]
        pairs.append((w, edits(rng, w, rng.randint(1, 6))))
    rng.shuffle(pairs)
    return pairs


def test_random_pairs_both_tiers(eng):
    g, o, words = eng
    pairs = random_pairs(words)
    assert len(pairs) == 20000
    nshort = sum(is_short(a, b) for a, b in pairs)
    assert nshort >= 1000 and len(pairs) - nshort >= 1000, nshort  # the comparison cannot pass on one tier alone
    got = check_against_oracle(g, o, pairs)
    lens = [r["len_a"] for r in got] + [r["len_b"] for r in got]
    assert min(lens) >= 1 and max(lens) <= 40 and max(lens) > 16


def ranked_rows(g, qs):
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=3, max_matches=0, score_threshold=0.0, cutoff_threshold=0.0)
    b = g.encode_batch(qs, p)
    b.run()
    rows = b.fetch()
    pairs = b.fetch_pairs()
    b.free()
    return rows, pairs


def test_agrees_with_find_variants_bit_for_bit(eng, data_dir):
    g, _, words = eng
    qs = synth.make_queries(words, 300, max_len=16, seed=31)
    rows, dbg = ranked_rows(g, qs)
    by_pair = {(q, v): (ld, lcs, pre, suf, same) for q, v, ld, lcs, pre, suf, same, _ in dbg}
    flat = [(i, v, d) for i, r in enumerate(rows) for v, d, _ in r]
    assert len(flat) > 1000
    got = g.score_pairs([qs[i] for i, _, _ in flat], [g.vocab_text(v) for _, v, _ in flat])
    for (i, v, d), r in zip(flat, got):
        assert r["status"] == 0 and r["score"] == d and r["ld"] <= 3, (qs[i], g.vocab_text(v), r, d)
        assert (r["ld"], r["lcs"], r["prefixlen"], r["suffixlen"], int(r["samecase"])) == by_pair[(i, v)], (qs[i], g.vocab_text(v), r)
    # a model whose weights make the reference skip three measures: the score is still the row's
    gw = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(ld=1, lcs=0, prefix=0.5, suffix=0, case=0), device=0)
    gw.read_lexicon(os.path.join(data_dir, "eng.aspell.lexicon"))
    gw.build()
    rows, _ = ranked_rows(gw, qs)
    flat = [(i, v, d) for i, r in enumerate(rows) for v, d, _ in r]
    assert len(flat) > 1000
    got = gw.score_pairs([qs[i] for i, _, _ in flat], [gw.vocab_text(v) for _, v, _ in flat])
    for (i, v, d), r in zip(flat, got):
        assert r["score"] == d, (qs[i], gw.vocab_text(v), r, d)


@pytest.fixture(scope="module")
def checked_set(eng):
    """41 pairs, short and long interleaved (a pair of > 64 symbols and two with a status among them), checked against the oracle once."""
    g, o, words = eng
    rng = random.Random(5)
    pairs = []
    for i in range(41):
        if i % 2 == 0:
            w = rng.choice([x for x in words if len(x) <= 12])
            pairs.append((w, edits(rng, w, 2, max_len=14)))
        else:
            w = "".join(rng.choice(words) for _ in range(3))[:40].ljust(18, "e")
            pairs.append((w, edits(rng, w, 4)))
    pairs[7] = (letters_of(rng, 130), letters_of(rng, 140))
    pairs[20] = ("", "word")
    pairs[33] = ("b" * 256, "word")
    assert sum(is_short(a, b) for a, b in pairs) >= 15 and sum(not is_short(a, b) for a, b in pairs) >= 15
    check_against_oracle(g, o, pairs)
    cols = g.score_pairs_arrays([a for a, _ in pairs], [b for _, b in pairs])
    return pairs, cols


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, (1 << 20) + 3])
def test_order_and_sizes(eng, checked_set, n):
    g, _, _ = eng
    pairs, cols = checked_set
    m = len(pairs)
    start = n % m  # (not always from the set's first pair)
    ix = (np.arange(n) + start) % m
    a = [pairs[i][0] for i in ix.tolist()]
    b = [pairs[i][1] for i in ix.tolist()]
    got = g.score_pairs_arrays(a, b)
    for k in A.VariantModel.PAIR_KEYS:
        assert got[k].shape == (n,)
        bad = np.nonzero(got[k] != cols[k][ix])[0]
        assert bad.size == 0, (k, n, bad[:5].tolist(), [pairs[ix[j]] for j in bad[:2].tolist()])


def test_packed_form_equals_pointer_form(eng, checked_set):
    g, _, _ = eng
    pairs, cols = checked_set
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    ptr = g.score_pairs_arrays(a, b, packed=False)
    for k in A.VariantModel.PAIR_KEYS:
        assert np.array_equal(ptr[k], cols[k]), k
    # a blob that is one string short
    ba = b"\0".join(x.encode() for x in a) + b"\0"
    bb = b"\0".join(x.encode() for x in b[:-1]) + b"\0"
    out = (L.PairScore * len(pairs))()
    assert L.lib().anx_score_pairs_packed(g.h, ba, len(ba), bb, len(bb), len(pairs), out) == L.ANX_EINVAL
    assert "fewer strings than announced" in L.last_error()
    assert L.lib().anx_score_pairs_packed(g.h, ba, len(ba) - 1, ba, len(ba), len(pairs), out) == L.ANX_EINVAL  # the last string has no terminator
    assert L.lib().anx_score_pairs_packed(g.h, ba, len(ba), ba, len(ba), len(pairs), out) == L.ANX_OK
    assert all(out[i].ld == 0 and out[i].status == cols["status"][i] for i in range(len(pairs)))  # (a, a): the statuses are those of a


def test_four_host_threads(eng, checked_set):
    g, _, _ = eng
    pairs, cols = checked_set
    m = len(pairs)
    sizes = [1, 2, 17, 64, 65, 200, 41, 333, 1000, 5, 2048, 77, 129, 640, 3, 4097, 31, 500, 96, 1500]
    errors = []

    def work(t):
        try:
            for c, n in enumerate(sizes):
                ix = (np.arange(n) + 7 * t + c) % m
                got = g.score_pairs_arrays([pairs[i][0] for i in ix.tolist()], [pairs[i][1] for i in ix.tolist()], packed=bool((t + c) & 1))
                for k in A.VariantModel.PAIR_KEYS:
                    if not np.array_equal(got[k], cols[k][ix]):
                        errors.append((t, n, k))
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[:5]


def test_command_line(eng, data_dir, tmp_path):
    g, _, _ = eng
    pairs = [("seperate", "separate"), ("recieve", "receive"), ("Hello", "hello"), ("abc", "ca"), ("", "empty side"), ("teh", "the"),
             ("an input of more than sixteen bytes", "an inptu of more than sixten bytes"), ("x" * 70, "xy" * 35), ("naïve", "naive"),
             ('quo"te', "quote"), ("a", "b"), ("same", "same")]
    assert len(pairs) == 12
    src = tmp_path / "pairs.tsv"
    src.write_text("".join(f"{a}\t{b}\n" for a, b in pairs), encoding="utf-8")
    exp = g.score_pairs([a for a, _ in pairs], [b for _, b in pairs])
    assert exp[4]["status"] == L.ANX_EEMPTY and sum(1 for r in exp if r["status"]) == 1
    base = [sys.executable, "-m", "analiticcl_amd", "score", "--alphabet", os.path.join(data_dir, "simple.alphabet.tsv"), "--lexicon",
            os.path.join(data_dir, "eng.aspell.lexicon"), "--device", "0"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONIOENCODING="utf-8")
    # a fresh child process per form
    tsv = subprocess.run(base + [str(src)], cwd=REPO, env=env, capture_output=True, text=True, encoding="utf-8", timeout=300)
    assert tsv.returncode == 0, tsv.stderr[-2000:]
    lines = tsv.stdout.split("\n")
    assert lines[-1] == "" and len(lines) == 13
    for (a, b), r, line in zip(pairs, exp, lines):
        assert line == cli.score_tsv_line(a, b, r), (a, b)
        f = line.split("\t")
        assert len(f) == 8 and f[:2] == [a, b]
        if r["status"]:
            assert f[2:] == [""] * 6
        else:
            assert f[2] == cli.rust_f64(r["score"]) and [int(x) for x in f[3:]] == [r["ld"], r["lcs"], r["prefixlen"], r["suffixlen"], int(r["samecase"])]
    js = subprocess.run(base + ["--json", str(src)], cwd=REPO, env=env, capture_output=True, text=True, encoding="utf-8", timeout=300)
    assert js.returncode == 0, js.stderr[-2000:]
    assert js.stdout == "[\n" + "".join(cli.score_json_item(a, b, r, i + 1) for i, ((a, b), r) in enumerate(zip(pairs, exp))) + "]\n"
    items = json.loads(js.stdout)
    assert len(items) == 12
    for (a, b), r, it in zip(pairs, exp, items):
        assert (it["a"], it["b"]) == (a, b)
        if r["status"]:
            assert it == {"a": a, "b": b, "status": r["status"]}
        else:
            assert (it["score"], it["ld"], it["lcs"], it["prefix"], it["suffix"], it["samecase"]) == (
                float(cli.rust_f64(r["score"])), r["ld"], r["lcs"], r["prefixlen"], r["suffixlen"], r["samecase"])
