"""The small call on models with a confusable list (small_path.hpp + conf_launch_small of conf.hip: k_conf_screen, k_small_conf_order,
k_conf_script, k_conf_apply_late / _early inside the one-wait chain): taken at all, equal to the batch path (ANX_SMALL=0) row for row
with `==`, equal to the host-side weighting (ANX_CONFUSABLES=host, which the small path never takes) and to oracle/twin.py (ids and
order exact, scores within 1e-6); the borders of the order kernel (an empty list, one entry, more entries than its block has threads);
a row the device cannot weight; variant lists and confusables together; a model that changes between calls; contexts shared by
threads and models; the fixed capacities."""
import ctypes as C
import os
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import synth
from oracle import twin as T
from variant_models_common import small_stats, via_batch_path

TEST_ALPHABET_TSV = "\n".join(f"{c}\t{c.upper()}" for c in "abcdefghijklmnopqrstuvwxyz") + "\n.\t,\n"
SEVEN = "-[y]+[i]\t1.1\n-[a]+[e]\t1.05\n=[c|k]-[s]\t0.9\n+[e]$\t0.95\n^-[k]\t0.8\n-[e]=[r]\n+[s]\t0.97\n"
CONF10 = os.path.join(synth.GOLDEN_DATA, "confusables10.tsv")
ORDER_THREADS = 1024     # threads of k_small_conf_order's one block (conf.hip CF_ORDER_T): a longer list takes several passes
PARAM_SETS = ((0.0, 5, 2.0), (0.5, 3, 1.5), (0.0, 0, 0.0))   # freq_weight, max_matches, cutoff_threshold


def conf_stats():
    out = (C.c_uint64 * 3)()
    assert L.lib().anx_debug_small_conf_stats(out) == 0
    return out[0], out[1], out[2]


def call(model, qs, params):
    return model.find_variants_ids(qs, params, with_via=True)


def via_host_weighting(model, qs, params):
    A.set_switch("ANX_CONFUSABLES", "host")
    try:
        t0 = small_stats()
        got = call(model, qs, params)
        assert small_stats() == t0, "the small path took a call whose confusables are weighted on the host"
        return got
    finally:
        A.set_switch("ANX_CONFUSABLES", None)


def taken(model, qs, params):
    """One call the small path must answer: -> rows, edit scripts run"""
    t0, c0 = small_stats(), conf_stats()
    got = call(model, qs, params)
    t1, c1 = small_stats(), conf_stats()
    assert t1 == (t0[0] + 1, t0[1]), "the small path did not take the call"
    assert c1[0] == c0[0] + 1 and c1[2] == c0[2]
    return got, c1[1] - c0[1]


def words2000():
    return [w for w in synth.load_lexicon_words(os.path.join(synth.GOLDEN_DATA, "eng_aspell.lexicon.gz")) if w.isascii() and w.isalpha()][::53][:2000]


def model2(early, patterns=SEVEN, extra_words=(), twin=False):
    """The model of test_gpu_confusables.test_random_vs_twin: every 53rd ASCII word of the golden eng lexicon, frequencies from
    Random(3), its seven patterns."""
    rng = random.Random(3)
    g = A.VariantModel("", alphabet_text=TEST_ALPHABET_TSV, device=0)
    tw = T.VariantModel(T.TEST_ALPHABET) if twin else None
    for w in words2000():
        f = rng.randrange(1, 30)
        g.add_to_vocabulary(w, f)
        if tw:
            tw.add_to_vocabulary(w, f)
    for w in extra_words:
        g.add_to_vocabulary(w, 1)
    for line in patterns.split("\n"):
        if line:
            script, _, w = line.partition("\t")
            g.add_to_confusables(script, float(w) if w else 1.0)
            if tw:
                tw.add_to_confusables(script, float(w) if w else 1.0)
    if early:
        g.set_confusables_before_pruning()
        if tw:
            tw.set_confusables_before_pruning()
    g.build()
    if tw:
        tw.build()
    return g, tw


def gparams(fw, mm, cut, **kw):
    d = dict(max_anagram_distance=2, max_edit_distance=2, max_matches=mm, score_threshold=0.3, cutoff_threshold=cut, freq_weight=fw)
    d.update(kw)
    return A.SearchParameters(**d)


def assert_equals_twin(got, exp):
    for r, e in zip(got, exp):
        assert [v for v, _d, _f, _via in r] == [x.vocab_id for x in e]
        for (v, d, f, _via), x in zip(r, e):
            assert abs(d - x.dist_score) < 1e-6 and abs(f - x.freq_score) < 1e-6


# ---- 1. taken at all -----------------------------------------------------------------------------------------------------------------
def huis_model(script):
    g = A.VariantModel("", alphabet_text=TEST_ALPHABET_TSV, device=0)
    tw = T.VariantModel(T.TEST_ALPHABET)
    for w in ("huis", "huls"):
        g.add_to_vocabulary(w)
        tw.add_to_vocabulary(w)
    g.add_to_confusables(script, 1.1)
    tw.add_to_confusables(script, 1.1)
    g.build()
    tw.build()
    return g, tw


def test_one_string_is_taken():
    g, tw = huis_model("-[y]+[i]")
    p = A.SearchParameters(max_anagram_distance=2, max_edit_distance=2, max_matches=10, score_threshold=0.0, cutoff_threshold=0.0)
    got, scripts = taken(g, ["huys"], p)
    assert scripts == 1      # `huis` has an i for -[y]+[i]; `huls` is decided by the screen
    assert got == via_batch_path(g, ["huys"], p)
    assert_equals_twin(got, [tw.find_variants("huys", T.SearchParameters(("abs", 2), ("abs", 2), 10, 0.0, 0.0, False, 0.0))])
    assert len(got[0]) == 2 and got[0][0][1] > got[0][1][1]      # the reference's test 0502: huis before huls


# ---- 2. twin parity, late and early ------------------------------------------------------------------------------------------------------
_twin_cache = {}


def twin_case(early):
    """model, queries, per parameter set the twin's rows of the 300 queries (computed once per mode, left unchanged)"""
    if early not in _twin_cache:
        g, tw = model2(early, twin=True)
        qs = synth.make_queries(words2000(), 300, max_len=16, seed=21)
        exp = {}
        for fw, mm, cut in PARAM_SETS:
            tp = T.SearchParameters(("abs", 2), ("abs", 2), mm, 0.3, cut, False, fw)
            rows = [tw.find_variants(q, tp) for q in qs]
            changed = sum(any(tw.compute_confusable_weight(q, x.vocab_id) != 1.0 for x in r) for q, r in zip(qs, rows))
            exp[(fw, mm, cut)] = (rows, changed)
        _twin_cache[early] = (g, qs, exp)
    return _twin_cache[early]


@pytest.mark.parametrize("early", [False, True])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 300])
def test_twin_parity(early, n):
    g, qs, exp = twin_case(early)
    for fw, mm, cut in PARAM_SETS:
        p = gparams(fw, mm, cut)
        t0 = small_stats()
        got = call(g, qs[:n], p)
        assert sum(small_stats()) == sum(t0) + 1 and small_stats()[0] == t0[0] + 1
        assert got == via_batch_path(g, qs[:n], p)
        rows, changed = exp[(fw, mm, cut)]
        assert_equals_twin(got, rows[:n])
        if n == 300:
            assert changed > 10      # the patterns did fire


# ---- 3. nld.aspell with confusables10.tsv ---------------------------------------------------------------------------------------------------
EXTRA = (("-[ij]+[y]", 1.07), ("=[e]-[ë]+[e]", 1.03), ("^-[s]+[z]", 0.93), ("-[en]$", 0.9))   # multi-character, non-ASCII, `^`, `$`


@pytest.fixture(scope="module")
def nld(data_dir):
    out = {}
    for early in (False, True):
        g = A.VariantModel(os.path.join(data_dir, "simple.alphabet.tsv"), A.Weights(), device=0)
        g.read_lexicon(os.path.join(data_dir, "nld.aspell.lexicon"))
        g.read_confusablelist(CONF10)
        for script, w in EXTRA:
            g.add_to_confusables(script, w)
        if early:
            g.set_confusables_before_pruning()
        g.build()
        out[early] = g
    return out, synth.load_lexicon_words(os.path.join(data_dir, "nld.aspell.lexicon"))


@pytest.mark.parametrize("early", [False, True])
@pytest.mark.parametrize("n", [1000, 4096])
def test_nld_equals_batch_path_and_host_weighting(nld, early, n):
    models, words = nld
    g = models[early]
    special = ["", "ijsvrij", "zeeën", "naïve", "x" * 64]
    qs = synth.make_queries(words, n - len(special), max_len=24, seed=900 + n) + special
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
    got, scripts = taken(g, qs, p)
    assert got == via_batch_path(g, qs, p)
    assert got == via_host_weighting(g, qs, p)
    assert scripts > 0
    if n == 4096:
        assert scripts > ORDER_THREADS     # the order kernel's block went over the list more than once


# ---- 4. the order kernel's borders --------------------------------------------------------------------------------------------------------
def test_order_kernel_borders():
    words = words2000()
    # (a) an empty list: lexicon words, candidates within one edit, and a pattern no row can match (no q in the inputs)
    g, _ = model2(False, patterns="-[q]+[x]\t1.2\n")
    qs = [w for w in words if "q" not in w and 4 <= len(w) <= 10][:40]
    p = gparams(0.0, 5, 0.0, max_edit_distance=1)
    got, scripts = taken(g, qs, p)
    assert scripts == 0 and got == via_batch_path(g, qs, p) and all(r for r in got)
    # (b) exactly one entry (test_one_string_is_taken: `huis`, not `huls`), here with the cutoff applied afterwards
    h, _tw = huis_model("-[y]+[i]")
    ph = A.SearchParameters(max_anagram_distance=2, max_edit_distance=2, max_matches=10, score_threshold=0.0, cutoff_threshold=1.05)
    got, scripts = taken(h, ["huys"], ph)
    assert scripts == 1 and got == via_batch_path(h, ["huys"], ph)
    # (c) a few dozen entries, late and early
    for early in (False, True):
        g7, _ = model2(early)
        qs = synth.make_queries(words, 120, max_len=16, seed=5)
        p = gparams(0.0, 5, 2.0)
        got, scripts = taken(g7, qs, p)
        print(f"early={early}: {scripts} edit scripts for {len(qs)} queries")
        assert 12 <= scripts < ORDER_THREADS and got == via_batch_path(g7, qs, p)


# ---- 5. a row the device cannot weight ------------------------------------------------------------------------------------------------------
def test_unweightable_row_hands_the_call_over():
    long_word = ("abcdefghijklmnopqrstuvwxyz" * 3)[:66]            # 66 code points: beyond the 64 of conf.hip's lane memory
    query = long_word.replace("s", "", 1).replace("e", "", 1)      # 64 bytes, two deletions: +[s] may match, so the row needs an edit script
    assert len(query) == 64
    g, _ = model2(False, extra_words=(long_word,))
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
    t0, c0 = small_stats(), conf_stats()
    got = call(g, [query], p)
    t1, c1 = small_stats(), conf_stats()
    assert t1 == (t0[0], t0[1] + 1) and c1 == (c0[0], c0[1], c0[2] + 1)
    assert got == via_host_weighting(g, [query], p)
    assert got[0] and long_word in [x["text"] for x in g.find_variants(query, p)]


# ---- 6. variant lists and confusables together ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("early", [False, True])
def test_variant_lists_and_confusables(early):
    words = words2000()
    rng = random.Random(17)
    g = A.VariantModel("", alphabet_text=TEST_ALPHABET_TSV, device=0)
    frng = random.Random(3)
    ids = {w: g.add_to_vocabulary(w, frng.randrange(1, 30)) for w in words}
    refs = rng.sample([w for w in words if 5 <= len(w) <= 10], 12)
    variants = []
    for k, w in enumerate(refs):          # a misspelling per reference (y for i / a dropped e / a doubled letter), and an indexed word as a variant
        v = w.replace("i", "y", 1) if "i" in w else w.replace("e", "", 1) if "e" in w else w + w[-1]
        if v != w and v not in ids:
            g.add_variant(ids[w], v, 0.6 + 0.03 * k)
            variants.append(v)
    for a, b in zip(refs[:4], refs[4:8]):
        g.add_variant(ids[a], b, 0.8)   # an INDEXED entry with a VariantOf link: the lexicon has variant lists (rows with a `via` below)
    for line in SEVEN.split("\n"):
        if line:
            script, _, w = line.partition("\t")
            g.add_to_confusables(script, float(w) if w else 1.0)
    if early:
        g.set_confusables_before_pruning()
    g.build()
    qs = (variants + refs[4:8] + synth.make_queries(words, 64, max_len=16, seed=23))[:64]
    p = gparams(0.0, 5, 2.0)
    got, scripts = taken(g, qs, p)
    assert got == via_batch_path(g, qs, p)
    assert scripts > 0 and any(via is not None for r in got for *_x, via in r)


# ---- 7. the model changes between calls -------------------------------------------------------------------------------------------------------
def test_model_changes_between_calls():
    g, _ = model2(False)
    qs = synth.make_queries(words2000(), 300, max_len=16, seed=21)
    p = gparams(0.0, 5, 2.0)
    first, _s = taken(g, qs, p)
    g.add_to_confusables("+[e]", 0.5)      # a candidate with an e the input lacks: common among the misspellings
    g.build()
    second, _s = taken(g, qs, p)
    assert second == via_batch_path(g, qs, p)
    assert second != first


# ---- 8. contexts shared by threads and by models with and without confusables ------------------------------------------------------------------
def test_shared_contexts():
    words = words2000()
    gc, _ = model2(False)
    gp = A.VariantModel("", alphabet_text=TEST_ALPHABET_TSV, device=0)
    rng = random.Random(3)
    for w in words:
        gp.add_to_vocabulary(w, rng.randrange(1, 30))
    gp.build()
    qs = synth.make_queries(words, 1000, max_len=16, seed=31)
    p = gparams(0.0, 5, 2.0)
    sizes = [1, 2, 17, 64, 100, 257, 500, 1000]
    want = {(k, n): via_batch_path(m, qs[:n], p) for k, m in enumerate((gc, gp)) for n in sizes}
    assert want[(0, 1000)] != want[(1, 1000)]
    bad = []

    def worker(t):
        try:
            for it in range(10):
                k, n = (t + it) & 1, sizes[(t + 3 * it) % len(sizes)]
                if call((gc, gp)[k], qs[:n], p) != want[(k, n)]:
                    bad.append((t, it, k, n))
        except Exception as e:  # noqa: BLE001
            bad.append((t, repr(e)))

    t0 = small_stats()
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not bad
    assert small_stats()[0] == t0[0] + 80


# ---- 9. the fixed capacities --------------------------------------------------------------------------------------------------------------------
def test_capacity():
    g, _ = model2(True)
    rng = random.Random(9)
    qs = ["".join(rng.choice("aeiorstnl") for _ in range(rng.choice((3, 4)))) for _ in range(4096)]
    p = A.SearchParameters(max_anagram_distance=2, max_edit_distance=2, max_matches=0, score_threshold=0.0)
    t0 = small_stats()
    got = call(g, qs, p)
    t1 = small_stats()
    assert sum(t1) == sum(t0) + 1      # taken, or discarded after an overflow and answered by the batch path
    print("taken" if t1[0] > t0[0] else "discarded", sum(len(r) for r in got), "rows")
    assert got == via_batch_path(g, qs, p)
