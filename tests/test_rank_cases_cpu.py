"""Two conditions on the inputs of tests/test_gpu_rank_rows.py, checked without a GPU.

(a) The census: which branches of k_rank (kernels_rank.hpp) the hand-made batches of tests/rank_cases.py reach, derived from the rows and
    the parameters by the conditions written in the kernel.  Every class must be populated under both kernel instances, and every
    reachable combination of group width x crop outcome x cutoff outcome; what is held unreachable is listed here with the reason.
    Nothing is measured: this keeps the GPU test from silently missing a branch.
(b) rank_tail, the tail factored out of the twin's score_and_rank (oracle/twin.py), on score_and_rank's own candidate rows for golden-
    lexicon queries: it must reproduce find_variants of the twin and of the C oracle, with and without a frequency weight and a
    variant list."""
import collections
import copy
import itertools
import random

import pytest

import rank_cases as R
from analiticcl_amd import synth
from oracle import cwrap as O
from oracle import twin as T


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tally():
    """per kernel instance (True = k_rank<true>): Counter of (class, value) and of (width, crop, cut)"""
    t = {True: collections.Counter(), False: collections.Counter()}
    for name, b in R.all_batches():
        c = t[b.params.simple]
        for q in R.census(b):
            c[("width", q["width"])] += 1
            if q["empty"]:
                c[("empty", q["width"])] += 1
                continue
            for k in ("prune", "pruned_rows", "quickselect", "tau", "lds", "compare", "parallel_tail", "expanded", "dups"):
                c[(k, q[k])] += 1
            c[("path", q["width"], "lds" if q["lds"] else "all", q["compare"], "parallel" if q["parallel_tail"] else "serial")] += 1
            c[("combo", q["width"], q["crop"], q["cut"])] += 1
            if name == "long" and q["width"] == 64:
                c[("long", q["quickselect"] and q["tau"] and q["lds"])] += 1
    return t


CLASSES = [("width", 16), ("width", 32), ("width", 64), ("empty", 16), ("prune", True), ("prune", False), ("pruned_rows", True),
           ("quickselect", True), ("quickselect", False), ("tau", True), ("tau", False), ("lds", True), ("lds", False),
           ("compare", "packed"), ("compare", "weighted"), ("compare", "plain"), ("parallel_tail", True), ("parallel_tail", False),
           ("expanded", True), ("expanded", False), ("dups", True), ("dups", False), ("long", True)]
# k_rank<true> runs only without variant lists at freq_weight 0: no weighted sort key, no expanded query, no duplicate removal
UNREACHABLE_SIMPLE = {("compare", "weighted"), ("expanded", True), ("dups", True)}


@pytest.mark.parametrize("simple", [True, False], ids=["k_rank_true", "k_rank_false"])
def test_every_branch_class_is_populated(tally, simple):
    missing = [c for c in CLASSES if tally[simple][c] == 0 and not (simple and c in UNREACHABLE_SIMPLE)]
    assert not missing, missing
    assert tally[simple][("long", False)] == 0  # the long lists all stay on the quickselect + LDS path (no O(n^2) pass over 65 k rows)
    if simple:
        assert all(tally[True][c] == 0 for c in UNREACHABLE_SIMPLE)


def test_paths_of_each_group_width(tally):
    """the combinations of width x LDS / all rows x compare x tail that the code can take"""
    for simple in (True, False):
        t = tally[simple]
        for width in (16, 32, 64):
            for compare in ("packed", "plain", "weighted"):
                if simple and compare != "packed":
                    continue
                for tail in ("parallel", "serial"):
                    # serial without an expanded query needs more than `width` ranks: impossible with <= 16 / <= 32 rows ...
                    if tail == "serial" and width < 64 and compare == "packed":
                        continue  # ... and packed keys mean no variant lists, hence no expanded query
                    assert t[("path", width, "lds", compare, tail)] > 0, (simple, width, compare, tail)
        # only the 64-lane path can keep more than its LDS holds; rank_query_all has no packed compare
        assert t[("path", 64, "all", "plain", "parallel")] > 0, simple
        assert t[("path", 64, "all", "plain", "serial")] > 0, simple
        if not simple:
            assert t[("path", 64, "all", "weighted", "serial")] > 0
        assert not [k for k in t if k[0] == "path" and k[2] == "all" and (k[1] != 64 or k[3] == "packed")]


def test_width_crop_cutoff_combinations(tally):
    """Unreachable, both under k_rank<true> only:
    * `late` and `neither`.  The crop's tie branch compares each row's dist_score with the result score of row max_matches; at
      freq_weight 0 that row's own dist_score IS that score and max_matches >= 1, so `early` is always found.  With a frequency weight the
      two differ and all five outcomes occur at every width.
    * `cropped < last` together with a cut at 16 and 32 lanes.  Without variant lists at freq_weight 0 every list of <= 65 535 rows is
      pruned when the cutoff applies: what the tail sees are rows above best / cutoff and rows equal to the best.  A cut among those needs
      best <= best / cutoff, i.e. cutoff 1.0 (or best 0), and then every row left equals the best: no `cropped < last`.  Only the lists
      beyond 65 535 rows (64 lanes) are not pruned and reach it.  (The census follows the kernel's working list, not the reference's.)"""
    for simple in (True, False):
        for width, crop, cut in itertools.product((16, 32, 64), R.CROP_OUTCOMES, (False, True)):
            n = tally[simple][("combo", width, crop, cut)]
            if simple and (crop in ("late", "neither") or (crop == "cropped_lt_last" and cut and width < 64)):
                assert n == 0, (width, crop, cut)
            else:
                assert n > 0, (simple, width, crop, cut)


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------
def _models(tmp_path, words, with_freq, with_variants, rng):
    alphabet = str(tmp_path / "alphabet.tsv")
    lex = str(tmp_path / ("lex%d%d.tsv" % (with_freq, with_variants)))
    with open(lex, "w", encoding="utf-8") as f:
        for w in words:
            f.write(w + ("\t%d\n" % rng.choice([1, 1, 2, 5, 40, 1000, 70000]) if with_freq else "\n"))
    tm = T.VariantModel(T.read_alphabet(alphabet))
    om = O.OracleModel(alphabet_path=alphabet)
    tm.read_vocabulary(lex)
    om.read_lexicon(lex)
    if with_variants:
        vl = str(tmp_path / "variants.tsv")
        lines = []
        for w in rng.sample(words, 300):
            fields = [w] + (["%d" % rng.randrange(1, 90)] if with_freq else [])
            for _ in range(rng.randrange(1, 4)):
                cs = list(w)
                cs[rng.randrange(len(cs))] = rng.choice("aeiouy")
                fields += ["".join(cs), str(rng.choice([1.0, 0.9, 0.75, 0.5]))] + (["%d" % rng.randrange(1, 50)] if with_freq else [])
            lines.append("\t".join(fields))
        open(vl, "w", encoding="utf-8").write("\n".join(lines) + "\n")
        tm.read_variants(vl, True)
        om.read_variants(vl, True)
    tm.build()
    om.build()
    return tm, om


@pytest.mark.parametrize("with_freq,with_variants", [(0, 0), (1, 1)])
def test_rank_tail_reproduces_find_variants(data_dir, tmp_path, monkeypatch, with_freq, with_variants):
    rng = random.Random(20 + 2 * with_freq + with_variants)
    open(tmp_path / "alphabet.tsv", "w", encoding="utf-8").write(open(data_dir + "/simple.alphabet.tsv", encoding="utf-8").read())
    words = [w for w in synth.load_lexicon_words(data_dir + "/eng.aspell.lexicon") if "\t" not in w][::4]
    tm, om = _models(tmp_path, words, with_freq, with_variants, rng)
    queries = synth.make_queries(words, 75, max_len=14, seed=5 + with_freq)
    seen = []
    real = T.rank_tail

    def recorder(results, *args):
        seen.append((copy.deepcopy(results), args[:5]))  # late confusables (the sixth) are not part of this
        assert args[5] is None
        return real(results, *args)

    monkeypatch.setattr(T, "rank_tail", recorder)
    nrows = 0
    for mm, thr, cutoff, fw in ((10, 0.25, 2.0, 0.0), (0, 0.0, 0.0, 0.0), (3, 0.1, 1.5, 0.7), (2, 0.0, 0.0, 1.0)):
        tp = T.SearchParameters(("abs", 3), ("abs", 3), mm, thr, cutoff, False, fw)
        op = O.make_params(("abs", 3), ("abs", 3), mm, thr, cutoff, False, fw)
        for q in queries:
            del seen[:]
            twin = [(x.vocab_id, x.dist_score, x.freq_score, x.via) for x in tm.find_variants(q, tp)]
            rows, args = seen[0]
            assert len(seen) == 1 and args[2:] == (mm, cutoff, fw)
            nrows += len(rows)
            mine = [(x.vocab_id, x.dist_score, x.freq_score, x.via) for x in real(rows, *args)]
            assert mine == twin, (q, mm, fw)
            assert mine == om.find_variants_via(q, op), (q, mm, fw)
    print("candidate rows:", nrows)
    assert nrows > 4 * len(queries)  # more than one candidate row per call on average: the tail had something to rank
