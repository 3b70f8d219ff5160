"""Context rules in the device lattice decoder (lattice.hip: k_ctx_rules scores them, k_lattice_lm uses the score in its rerank): a
model with context rules takes the one-pass path and the device decoder like any other; the device scores the rules of every final
path and returns what covers the chosen one, the host expands the tags.  Checked against the reference's own rule tests (tests/main.rs:1575-1728, values transcribed), and, on random
models / rule sets / parameters, the default path == the classic path with the device lattice (ANX_SEARCH_ONEPASS=0) == the host
decoder (ANX_LATTICE=host) == the oracle twin.  anx_debug_search_lattice_stats tells where the lattices were decoded."""
import contextlib
import os
import random

import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import synth
from oracle import cwrap as O
from oracle import twin as T

from search_common import TwinOverOracle

TEST_ALPHABET_TSV = "\n".join(f"{c}\t{c.upper()}" for c in "abcdefghijklmnopqrstuvwxyz") + "\n.\t,\n"
LM = A.VocabParams(vocabtype="LM")


class Decoded:
    """what anx_debug_search_lattice_stats counted inside the block"""

    def __enter__(self):
        self.before = A.VariantModel.search_lattice_stats()
        return self

    def __exit__(self, *exc):
        after = A.VariantModel.search_lattice_stats()
        self.device, self.host, self.rules, self.onepass = (after[k] - self.before[k] for k in ("device", "host", "device_rules", "onepass_parts"))

    def assert_device_rules(self):
        """the default path: every decoded lattice on the device, with the rules scored there"""
        assert self.device > 0 and self.rules == self.device and self.host == 0, (self.device, self.host, self.rules)


@contextlib.contextmanager
def switch(name, value):
    A.set_switch(name, value)
    try:
        yield
    finally:
        A.set_switch(name, None)


def sparams(**kw):  # src/test.rs:48-68
    d = dict(max_anagram_distance=2, max_edit_distance=2, max_matches=10, score_threshold=0.0, cutoff_threshold=0.0, max_ngram=2)
    d.update(kw)
    return A.SearchParameters(**d)


def rules_model(lm=False, devices=None):
    g = A.VariantModel("", alphabet_text=TEST_ALPHABET_TSV, **({"devices": devices} if devices else {"device": 0}))
    for w in ("I", "think", "sink", "you", "are", "right"):
        g.add_to_vocabulary(w, 2)
    if lm:
        for t, f in (("<bos> I", 2), ("I think", 2), ("I sink", 1), ("you are", 2), ("right <eos>", 2)):
            g.add_to_vocabulary(t, f, LM)
    g.build()
    return g


def chosen(r):
    return [m["variants"][0]["text"] if m["variants"] else m["input"] for m in r]


# -- 1. the reference's values (tests/main.rs:1575-1728: test0902 bonus, 0903 penalty, 0904 tags, 0905 two tags) ---------------------
@pytest.mark.parametrize("lm", [False, True])
def test_reference_rule_setups_on_the_device(lm):
    """lm=False: max_ngram 1 and no LM -- the lattice exists only because of the rules, and reaches the device on the classic path;
    lm=True: the same sentences through the one-pass path (an LM whose weight is 0 changes no choice)."""
    p = sparams(max_ngram=1, lm_weight=0.0)
    text = "I tink you are rihgt"
    with Decoded() as d:
        g = rules_model(lm)
        g.add_contextrule("I; think", 1.1, ["testtag"], [])  # bonus
        r = g.find_all_matches(text, p)
        assert chosen(r) == ["I", "think", "you", "are", "right"]
        assert (r[0]["tag"], r[0]["seqnr"], r[1]["tag"], r[1]["seqnr"]) == (["testtag"], [0], ["testtag"], [1])
        assert "tag" not in r[2]
        g = rules_model(lm)
        g.add_contextrule("I; think", 0.9)  # penalty
        assert chosen(g.find_all_matches(text, p)) == ["I", "sink", "you", "are", "right"]
        g = rules_model(lm)
        for w in ("think", "are", "right"):
            g.add_contextrule(w, 1.0, ["testtag"])
        r = g.find_all_matches(text, p)
        assert chosen(r) == ["I", "think", "you", "are", "right"]
        assert [m.get("tag", []) for m in r] == [[], ["testtag"], [], ["testtag"], ["testtag"]]
        assert [m.get("seqnr", []) for m in r] == [[], [0], [], [0], [0]]
        g = rules_model(lm)
        g.add_contextrule("I; think", 1.1, ["testtag", "testtag2"])
        r = g.find_all_matches(text, p)
        assert (r[0]["tag"], r[0]["seqnr"], r[1]["tag"], r[1]["seqnr"]) == \
            (["testtag", "testtag2"], [0, 0], ["testtag", "testtag2"], [1, 1])
        assert g.tags == ["testtag", "testtag2"]
    d.assert_device_rules()
    assert d.device == 4 and d.onepass == (4 if lm else 0)


# -- 2. randomised A/B ---------------------------------------------------------------------------------------------------------------
ENG = [w for w in synth.load_lexicon_words(os.path.join(synth.GOLDEN_DATA, "eng_aspell.lexicon.gz")) if w.isascii() and w.isalpha() and 2 <= len(w) <= 9]


def world(rng, tmp_path, tag, with_lm, twin=True, devices=None):
    """A small lexicon split over two or three lexicon files (overlapping: @lexicon patterns see different masks), some indexed
    two-word entries, in some rounds a bigram LM; the same model as product, twin and C oracle (ids aligned by insertion order)."""
    words = rng.sample(ENG[::29], rng.randrange(30, 70))
    nlex = rng.choice((2, 3))
    files = []
    for k in range(nlex):
        mine = [w for i, w in enumerate(words) if i % nlex == k or rng.random() < 0.15]
        mine += [f"{rng.choice(words)} {rng.choice(words)}" for _ in range(4)]
        f = tmp_path / f"{tag}_lex{k}.tsv"
        f.write_text("".join(f"{w}\t{rng.randrange(1, 40)}\n" for w in mine))
        files.append(str(f))
    g = A.VariantModel("", alphabet_text=TEST_ALPHABET_TSV, **({"devices": devices} if devices else {"device": 0}))
    tw = TwinOverOracle(T.TEST_ALPHABET) if twin else None
    orc = O.OracleModel(alphabet_text=TEST_ALPHABET_TSV) if twin else None
    for f in files:
        g.read_lexicon(f)
        if twin:
            tw.read_vocabulary(f)
            orc.read_lexicon(f)
    if with_lm:
        for _ in range(150):
            a, b = rng.choice(words), rng.choice(words)
            fr = rng.randrange(1, 9)
            g.add_to_vocabulary(f"{a} {b}", fr, LM)
            if twin:
                tw.add_lm(f"{a} {b}", fr)
        for w in words[:10]:
            g.add_to_vocabulary(f"<bos> {w}", 3, LM)
            if twin:
                tw.add_lm(f"<bos> {w}", 3)
    g.build()
    if twin:
        tw.build()
        orc.build()
        tw.attach(orc)
    return g, tw, words, [os.path.basename(f) for f in files]


def random_rules(rng, words, lexnames, n, score=lambda rng: rng.choice((0.5, 0.75, 0.9, 1.1, 1.25, 1.5))):
    """every pattern form; few distinct words so that the rules overlap and their order decides what covers a position"""
    hot = words[:12]
    w = lambda: rng.choice(hot)  # noqa: E731
    lx = lambda: "@" + rng.choice(lexnames)  # noqa: E731

    def element():
        k = rng.randrange(10)
        return (w(), w(), lx(), "?", "^", "!" + w(), "|".join(w() for _ in range(3)), f"!({w()}|{lx()})", f"!{w()}|{w()}", "!" + lx())[k]
    out = []
    for _ in range(n):
        length = rng.choice((1, 1, 2, 2, 3, 4))
        pat = "; ".join(element() for _ in range(length))
        kind = rng.randrange(5)
        if kind <= 1:
            tags, offs = [], []
        elif kind == 2:
            tags, offs = [f"t{rng.randrange(4)}"], []
        elif kind == 3:
            tags, offs = [f"t{rng.randrange(4)}"], [f"{rng.randrange(length)}:1"]
        else:
            tags, offs = [f"t{rng.randrange(4)}", "u"], ["0:1", f"{rng.randrange(length)}:"]
        out.append((pat, score(rng), tags, offs))
    return out


def sentences(rng, words, n):
    qs = synth.make_queries(words, n * 8, max_len=20, seed=rng.randrange(1 << 30))
    seps = [" "] * 14 + [", ", ". ", "\n", "; ", " (", "  "]
    texts, k = [], 0
    for _ in range(n):
        nw = rng.randrange(2, 8)
        t = ""
        for j in range(nw):
            t += qs[k] if rng.random() < 0.8 else rng.choice(words[:12])  # (clean frequent words: the rules do fire)
            k += 1
            if j + 1 < nw:
                t += rng.choice(seps)
        texts.append(t)
    return texts


def flat(per_text):
    """every Match field of a find_all_matches_ids result, comparable with =="""
    return [[(m["begin"], m["end"], m["n"], m["selected"], tuple(m["variants"]), tuple(m["tag"]), tuple(m["seqnr"])) for m in ms] for ms in per_text]


def assert_equals_twin(texts, got, tw, tp):
    for text, gm in zip(texts, got):
        exp = tw.find_all_matches(text, tp)
        raw = text.encode()
        assert [(raw[m["begin"]:m["end"]].decode(), m["begin"], m["end"]) for m in gm] == [(e.text, e.begin, e.end) for e in exp], text
        for m, e in zip(gm, exp):
            ev = e.variants or []
            assert [(v[0], v[1], v[2]) for v in m["variants"]] == [(v.vocab_id, v.dist_score, v.freq_score) for v in ev], (text, e.text)
            if ev:
                assert m["selected"] == e.selected, (text, e.text)
            assert (m["tag"], m["seqnr"]) == (e.tag, e.seqnr), (text, e.text)


def test_random_rule_sets_four_ways(tmp_path):
    rng = random.Random(90210)
    n_tagged = n_onepass = 0
    for rnd in range(30):
        with_lm = rnd % 3 != 2
        g, tw, words, lexnames = world(rng, tmp_path, f"r{rnd}", with_lm)
        rules = random_rules(rng, words, lexnames, rng.choice((1, 3, 8, 20, 40, 80)))
        for pat, sc, tags, offs in rules:
            g.add_contextrule(pat, sc, tags, offs)
            tw.add_contextrule(pat, sc, tags, offs)
        assert g.tags == tw.tags
        texts = sentences(rng, words, rng.choice((50, 50, 60, 80, 200)))
        max_ngram, max_seq, cw = rng.choice((1, 2, 3)), rng.choice((1, 5, 250)), rng.choice((0.0, 1.0, 3.0))
        lw = 1.0 if with_lm else rng.choice((0.0, 1.0))
        gp = A.SearchParameters(max_anagram_distance=2, max_edit_distance=2, max_matches=6, score_threshold=0.3, cutoff_threshold=0.0,
                                max_ngram=max_ngram, max_seq=max_seq, lm_weight=lw, contextrules_weight=cw)
        tp = T.SearchParams(("abs", 2), ("abs", 2), 6, 0.3, 0.0, False, 0.0, max_ngram=max_ngram, max_seq=max_seq, lm_weight=lw, contextrules_weight=cw)
        what = (rnd, len(rules), max_ngram, max_seq, cw, with_lm)
        with Decoded() as d:
            default = g.find_all_matches_ids(texts, gp)
        d.assert_device_rules()
        n_onepass += d.onepass
        with switch("ANX_SEARCH_ONEPASS", "0"), Decoded() as dc:
            classic = g.find_all_matches_ids(texts, gp)
        dc.assert_device_rules()
        assert dc.onepass == 0, what
        with switch("ANX_LATTICE", "host"), Decoded() as dh:
            host = g.find_all_matches_ids(texts, gp)
        assert dh.device == 0 and dh.host > 0, what
        assert flat(default) == flat(host), what
        assert flat(classic) == flat(host), what
        assert_equals_twin(texts, default, tw, tp)
        n_tagged += sum(bool(m["tag"]) for ms in default for m in ms)
    assert n_tagged > 200 and n_onepass > 10  # the rules fired, and the one-pass path took the rounds it is eligible for


# -- 3. hostile scores: the device against the host decoder (0 / 0 and logs of non-positive numbers: C and Rust return NaN / -inf where
#       the twin's math.log raises) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["zero", "negative", "mixed", "too_long", "all_equal"])
def test_hostile_scores_device_equals_host(tmp_path, case):
    rng = random.Random({"zero": 1, "negative": 2, "mixed": 3, "too_long": 4, "all_equal": 5}[case])
    g, _tw, words, lexnames = world(rng, tmp_path, case, with_lm=case != "negative", twin=False)
    if case == "zero":
        rules = random_rules(rng, words, lexnames, 20, score=lambda r: 0.0)
    elif case == "negative":
        rules = random_rules(rng, words, lexnames, 20, score=lambda r: r.choice((-1.0, -0.5, -2.5)))
    elif case == "mixed":
        rules = random_rules(rng, words, lexnames, 40, score=lambda r: r.choice((0.0, -1.0, 1.2, -0.25, 0.5, 1e30, -1e30)))
    elif case == "too_long":
        rules = [("; ".join(["?"] * 12), 1.3, ["long"], []), ("; ".join(["?"] * 40), 0.7, [], [])]
    else:
        rules = [("?", 1.25, ["all"], [])]  # every position of every path covered with the same score: every path scores 1.25
    for pat, sc, tags, offs in rules:
        g.add_contextrule(pat, sc, tags, offs)
    texts = sentences(rng, words, 120)
    n = 0
    for max_ngram, max_seq, cw, lw in ((2, 250, 1.0, 1.0), (3, 5, 3.0, 0.0), (1, 250, 1.0, 0.0), (2, 1, 1.0, 1.0)):
        gp = A.SearchParameters(max_anagram_distance=2, max_edit_distance=2, max_matches=6, score_threshold=0.3, cutoff_threshold=0.0,
                                max_ngram=max_ngram, max_seq=max_seq, lm_weight=lw, contextrules_weight=cw)
        with Decoded() as d:
            default = g.find_all_matches_ids(texts, gp)
        d.assert_device_rules()
        with switch("ANX_SEARCH_ONEPASS", "0"), Decoded() as dc:
            classic = g.find_all_matches_ids(texts, gp)
        dc.assert_device_rules()
        with switch("ANX_LATTICE", "host"), Decoded() as dh:
            host = g.find_all_matches_ids(texts, gp)
        assert dh.device == 0 and dh.host > 0
        assert flat(default) == flat(host), (case, max_ngram, max_seq, cw, lw)
        assert flat(classic) == flat(host), (case, max_ngram, max_seq, cw, lw)
        n += sum(bool(m["tag"]) for ms in default for m in ms)
    if case == "all_equal":
        assert n > 0
    if case == "too_long":
        assert n == 0  # no stretch has twelve tokens


# -- 4. replicas ---------------------------------------------------------------------------------------------------------------------
def test_three_replicas_decode_on_the_device(tmp_path):
    A.set_switch("ANX_SHARD_MIN", "2")  # every replica takes a share of the lattices
    try:
        outs = []
        for devices in ([0], [0, 0, 0]):
            rng = random.Random(4711)
            g, _tw, words, lexnames = world(rng, tmp_path, f"rep{len(devices)}", with_lm=True, twin=False, devices=devices)
            assert g.num_replicas == len(devices)
            for pat, sc, tags, offs in random_rules(rng, words, lexnames, 30):
                g.add_contextrule(pat, sc, tags, offs)
            texts = sentences(rng, words, 200)
            gp = A.SearchParameters(max_anagram_distance=2, max_edit_distance=2, max_matches=6, score_threshold=0.3, cutoff_threshold=0.0, max_ngram=3)
            with Decoded() as d:
                outs.append(flat(g.find_all_matches_ids(texts, gp)))
            d.assert_device_rules()
            assert d.onepass == (1 if len(devices) == 1 else 0)
        assert outs[0] == outs[1]
        assert sum(bool(m[5]) for ms in outs[0] for m in ms) > 0
    finally:
        A.set_switch("ANX_SHARD_MIN", None)


# -- 5. a model without rules ----------------------------------------------------------------------------------------------------------
def test_model_without_rules_scores_none(tmp_path):
    rng = random.Random(5)
    g, _tw, words, _lex = world(rng, tmp_path, "plain", with_lm=True, twin=False)
    texts = sentences(rng, words, 100)
    gp = A.SearchParameters(max_anagram_distance=2, max_edit_distance=2, max_matches=6, score_threshold=0.3, cutoff_threshold=0.0, max_ngram=3)
    with Decoded() as d:
        out = g.find_all_matches_ids(texts, gp)
    assert d.device > 0 and d.rules == 0 and d.host == 0 and d.onepass == 1
    assert all(not m["tag"] for ms in out for m in ms)
    with switch("ANX_LATTICE", "host"):
        assert flat(g.find_all_matches_ids(texts, gp)) == flat(out)
