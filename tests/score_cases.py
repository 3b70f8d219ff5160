"""Hand-laid pair lists for the scoring stage by itself (kernels_score.hpp: k_filter_score, k_filter_wide, k_score_fast8, k_score_pairs /
k_small_lists): the cases tests/test_gpu_score_slots.py sends through anx_debug_score_slots, their reference (the twin's measures and
pair_score, oracle/twin.py) and a census of the control flow each wave of the launch takes, derived from the inputs and the reference
alone (tests/test_score_cases_cpu.py asserts that the fixed seeds populate every class).  Plain Python and numpy, no GPU.

A case = a model (alphabet, entries, optional frequencies / variant list), a batch (queries, the edit-distance threshold, score_threshold,
StopAtExactMatch) and a pair list: 64 regions of slots, a slot = (query index, entry index | flags) or INVALID.  Entries are named by
their position in the model's vocabulary (vocabulary id - 3); the GPU test translates to entry ids.  The slots of a region are laid out
in CELLS of 64: a wave of k_filter_score handles slots base + r * 256 + 64 * w + lane in round r, so cell k of a block of 4096 slots is
(round k // 4, wave k % 4) and a wave's queue receives the survivors of its cells in round order.  Pairs may repeat: the survivor lists
are compared as multisets."""
import random
import zlib
from collections import Counter, defaultdict
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle import twin as T

REGIONS = 64
WAVE = 64
ROUND = 256
FS_BLK = 4096      # kernels_score.hpp
FS_SURV = 256
REGION_SHIFT = 13  # 8192 slots per region: a full block of 4096 and a partial second one
INVALID = 0xFFFFFFFF
PRE = 1 << 30      # RAW_PREFILTERED
EXACT = 1 << 31    # exact anagram class (StopAtExactMatch)
META_SKIPPED = 0xFFFFFFFF
META_NONE = 0x7F | 0x80   # ld = None, samecase = true
SEG_CAPS = (2, 32)
USED_REGIONS = (0, 5, 17, 40, 63)


# ---- models -----------------------------------------------------------------------------------------------------------------------------
def _alphabet(n_classes: int) -> List[List[str]]:
    """the first 26 classes are the Latin letters with their capitals, the others one character each (every character one code point)"""
    classes = [[c, c.upper()] for c in "abcdefghijklmnopqrstuvwxyz"]
    extra = [chr(c) for c in range(0x30, 0x3A)] + [chr(c) for c in range(0x3B1, 0x3CA) if c != 0x3C2] + [chr(c) for c in range(0x430, 0x450)]
    extra += [chr(c) for c in range(0xE0, 0x100) if c != 0xF7] + [chr(c) for c in range(0x561, 0x587)]
    classes += [[c] for c in extra[:n_classes - 26]]
    assert len(classes) == n_classes and len({c for cl in classes for c in cl}) == sum(len(cl) for cl in classes)
    return classes


@dataclass
class Model:
    name: str
    alphabet: List[List[str]]
    texts: List[str]                       # vocabulary items in vocabulary-id order (id = 3 + index)
    nwords: int                            # texts[:nwords] is the lexicon; the rest enters through the variant list
    freqs: Optional[List[int]] = None      # per lexicon word (model d)
    variants: List[Tuple[int, str, float]] = field(default_factory=list)   # (reference index, variant text, score): transparent variants
    transparent_only: List[str] = field(default_factory=list)              # transparent items without any reference
    weights: T.Weights = field(default_factory=T.Weights)
    twin: T.VariantModel = None
    norm: List[List[int]] = None
    _cache: Dict[Tuple[str, int], tuple] = field(default_factory=dict)

    @property
    def have_freq(self):
        return self.freqs is not None

    @property
    def any_variants(self):
        return bool(self.variants or self.transparent_only)

    @property
    def nclasses(self):
        return len(self.alphabet)

    @property
    def bit_planes(self):  # the scan's bit-plane tiles: at most 32 hash symbols, the classes and the unknown one (encode.hip bits_ok)
        return self.nclasses + 1 <= 32

    def alphabet_text(self) -> str:
        return "".join("\t".join(cl) + "\n" for cl in self.alphabet)

    def lexicon_text(self) -> str:
        return "".join(w + ("\t%d" % self.freqs[i] if self.have_freq else "") + "\n" for i, w in enumerate(self.texts[:self.nwords]))

    def finish(self):
        """the twin's model: same items in the same order as the device model gets them"""
        tm = T.VariantModel(self.alphabet, self.weights)
        tm.have_freq = self.have_freq
        for i, w in enumerate(self.texts[:self.nwords]):
            assert tm.add_to_vocabulary(w, self.freqs[i] if self.have_freq else None) == 3 + i, w
        for ref, text, score in self.variants:
            tm.add_variant(3 + ref, text, score, None, True)
        for text in self.transparent_only:
            tm.add_to_vocabulary(text, None, transparent=True)
        self.texts = [v.text for v in tm.decoder[3:]]
        self.twin = tm
        self.norm = [v.norm for v in tm.decoder[3:]]
        return self

    def rows_of(self, e: int) -> int:
        """result rows a kept survivor of entry e expands to (src/lib.rs:1677-1727): its references, plus itself unless transparent"""
        item = self.twin.decoder[3 + e]
        n = sum(1 for kind, _, _ in (item.variants or []) if kind == "variant_of")
        return n + (0 if item.transparent else 1)

    def measures(self, query: str, e: int):
        """(lq, lc, ld or None (beyond 12), lcs, prefix, suffix, samecase) from the twin, cached"""
        key = (query, e)
        r = self._cache.get(key)
        if r is None:
            s, t = T.normalize_to_alphabet(query, self.alphabet), self.norm[e]
            ld = T.damerau_levenshtein(s, t, T.MAX_EDIT_DISTANCE)
            if ld is None:
                r = (len(s), len(t), None, 0, 0, 0, True)
            else:
                r = (len(s), len(t), ld, T.longest_common_substring_length(s, t), T.common_prefix_length(s, t), T.common_suffix_length(s, t),
                     T.is_lowercase(self.texts[e][0]) == T.is_lowercase(query[0]))
            self._cache[key] = r
        return r


def _mutations(w: str, rng, letters: str, hi: str):
    """strings near w: the edits the kernels' DL forms must get right"""
    n = len(w)
    out = []
    pos = rng.randrange(n)
    out.append(w[:pos] + rng.choice(letters.replace(w[pos], "") or letters) + w[pos + 1:])      # substitution
    out.append(w[:pos] + rng.choice(letters) + w[pos:])                                        # insertion
    if n > 1:
        out.append(w[:pos] + w[pos + 1:])                                                      # deletion
        out.append(w[1] + w[0] + w[2:])                                                        # transposition at the first position
        out.append(w[:-2] + w[-1] + w[-2])                                                     # ... at the last
    if n >= 3:
        i = rng.randrange(n - 2)
        out.append(w[:i] + w[i + 2] + w[i] + w[i + 3:])                                        # transposition around a deleted symbol (1 + a + b, a = 1)
        out.append(w[:i] + w[i + 1] + rng.choice(letters) + w[i] + w[i + 2:])                  # ... around an inserted one (b = 1)
    if n >= 4:
        i = rng.randrange(n - 3)
        out.append(w[:i] + w[i + 3] + w[i] + w[i + 4:])                                        # a = 2
        out.append(w[:i] + w[i + 1] + rng.choice(letters) + rng.choice(letters) + w[i] + w[i + 2:])   # b = 2
        out.append(w[1] + w[0] + w[2:-2] + w[-1] + w[-2])                                      # two transpositions: distance 2 inside +-1
    if n >= 6:
        out.append(w[1] + w[0] + w[3] + w[2] + w[4:-2] + w[-1] + w[-2])                        # three: distance 3 inside +-1
        out.append(w[0] + rng.choice(letters) + w[2:-3] + rng.choice(letters) + w[-2] + hi[0])  # three substitutions, the highest code
    for k in (1, 2, 3):
        if n > k:
            out.append(w[:-k])                                                                 # the (lq, lc) grid: |lq - lc| = k
        out.append(w + "".join(rng.choice(letters) for _ in range(k)))
    out.append(w[0].upper() + w[1:])                                                           # samecase
    out.append(w[:pos] + "#" + w[pos + 1:])                                                    # a character outside the alphabet
    out.append(w[:pos] + hi[rng.randrange(len(hi))] + w[pos + 1:])
    return [x for x in out if x and x != w]


def _make_model(name, n_classes, seed, long_entries=False, freqs=False, variants=False) -> Model:
    rng = random.Random(seed)
    alphabet = _alphabet(n_classes)
    letters, hi = "abcde", alphabet[-1][0] + alphabet[-2][0]
    lengths = [n for n in range(1, 17) for _ in range(3)] + [17, 17, 18, 19, 20, 24, 30, 31, 32, 33, 34, 40]
    if long_entries:
        lengths = [n for n in range(1, 17)] + [17, 19, 24, 32, 33, 40, 100, 236, 240, 250, 255]
    bases = []
    for n in lengths:
        kind = rng.randrange(6)
        if kind == 0:
            w = "".join(rng.choice("ab") for _ in range(n))          # repeated symbols
        elif kind == 1:
            w = rng.choice(letters) * (n - 1) + rng.choice(letters)
        else:
            w = "".join(rng.choice(letters + (hi if rng.random() < 0.2 else "")) for _ in range(n))
        bases.append(w)
    entries, queries, border = [], [], []
    for w in bases:
        mu = _mutations(w, rng, letters, hi)
        rng.shuffle(mu)
        half = (len(mu) + 1) // 2
        entries += [w] + mu[:half] + [w + w[-1]]
        queries += [w] + mu[half:] + [w[0].upper() + w[1:] if w[0].islower() else w.lower()]
        if len(w) in (15, 16, 31, 32, 250):   # the length borders 16 / 17, 32 / 33 and 255, one and two symbols apart on either side
            border += [w + "a", w + "ba", w[:-1] + "cab", w + "abc"]
    entries += border

    def dedup(xs, cap):   # every base and border string, and an even sample of the strings around them
        xs = list(dict.fromkeys(x for x in xs if 0 < len(x) <= 255))
        keep = set(bases) | set(border) | set(rng.sample(xs, min(len(xs), cap)))
        return [x for x in xs if x in keep][:cap + len(bases) + len(border)]
    if long_entries:   # few, so that the 255-symbol distances stay cheap for the twin
        entries, queries = dedup(entries, 230), dedup([q for q in queries if len(q) <= 40 or rng.random() < 0.4], 70)
    else:
        entries, queries = dedup(entries, 500), dedup(queries, 220)
    m = Model(name, alphabet, entries, len(entries))
    if freqs:
        m.freqs = [rng.choice([1, 1, 2, 3, 7, 40, 1000, 70000, 4000000000]) for _ in entries]
    if variants:
        taken = set(entries)
        for ref in rng.sample(range(len(entries)), 60):
            for _ in range(rng.randrange(1, 3)):
                v = rng.choice(_mutations(entries[ref], rng, letters, hi))
                if v not in taken and len(v) <= 40:
                    taken.add(v)
                    m.variants.append((ref, v, rng.choice([1.0, 0.9, 0.75, 0.5])))
        # a variant of two references, a reference that is a variant itself, transparent items nobody refers to
        m.variants.append(((m.variants[0][0] + 1) % len(entries), m.variants[0][1], 0.8))
        for w in bases[6:40:4]:
            v = w + "e"
            if v not in taken:
                taken.add(v)
                m.transparent_only.append(v)
    m.queries = queries
    return m.finish()


_MODELS: Dict[str, Model] = {}


def model(name: str) -> Model:
    if name not in _MODELS:
        spec = {"a": dict(n_classes=26, seed=11), "b": dict(n_classes=70, seed=12), "c": dict(n_classes=130, seed=13),
                "d": dict(n_classes=26, seed=11, freqs=True), "e": dict(n_classes=26, seed=11, variants=True),
                "f": dict(n_classes=26, seed=16, long_entries=True)}[name]
        _MODELS[name] = _make_model(name, **spec)
    return _MODELS[name]


# ---- batches and their pair lists ---------------------------------------------------------------------------------------------------------
# name -> (model, max_edit_distance in the twin's form, StopAtExactMatch, score threshold: 0 or "cut" = the median survivor score)
BATCHES = {
    "a-abs1": ("a", ("abs", 1), False, 0.0), "a-abs2": ("a", ("abs", 2), False, "cut"), "a-abs3": ("a", ("abs", 3), False, 0.0),
    "a-abs3-cut": ("a", ("abs", 3), False, "cut"), "a-abs4": ("a", ("abs", 4), False, "cut"), "a-ratio": ("a", ("ratiolimit", 0.2, 3), False, "cut"),
    "a-stop": ("a", ("abs", 2), True, 0.0),
    # d = 3 up to 19 symbols, 4 and 5 beyond: no inline DL (D = 0), and k_filter_wide passes its pairs to the general list
    "a-ratio5": ("a", ("ratiolimit", 0.2, 5), False, 0.0),
    "b-abs2": ("b", ("abs", 2), False, "cut"), "b-ratio": ("b", ("ratiolimit", 0.2, 3), False, 0.0), "c-abs3": ("c", ("abs", 3), False, "cut"),
    "d-abs2": ("d", ("abs", 2), False, "cut"), "d-ratio": ("d", ("ratiolimit", 0.2, 3), False, 0.0),
    "e-abs2": ("e", ("abs", 2), False, "cut"), "e-abs3": ("e", ("abs", 3), False, 0.0),
    "f-abs3": ("f", ("abs", 3), False, 0.0), "f-abs4": ("f", ("abs", 4), False, "cut"), "f-abs12": ("f", ("abs", 12), False, 0.0),
}


# queries of at most this many symbols: two 16-byte words per query row leave k_score_pairs 128 threads beside a 255-symbol entry, 64 at d = 12
QMAX = {"f-abs3": 32, "f-abs4": 32}


def band_bound_rejects(s, t, d) -> bool:
    """kernels_swar.hpp band_bound_rejects: more than d symbols of either string without an equal symbol of the other within +-d positions"""
    una = sum(1 for i, x in enumerate(s) if x not in t[max(0, i - d):i + d + 1])
    unb = sum(1 for j, x in enumerate(t) if x not in s[max(0, j - d):j + d + 1])
    return una > d or unb > d


@dataclass
class Pair:   # one (query, entry) of a batch, everything the layout, the expectation and the census need
    q: int
    e: int
    lq: int
    lc: int
    dq: int
    ld: Optional[int]        # the twin's distance, None beyond the query's d
    ld_full: Optional[int]   # ... beyond 12
    meta: int
    score: float             # nan without a distance
    freq: int
    rows: int                # result rows if kept
    keep: bool               # score >= threshold and rows
    bandrej: bool
    flaggable: bool          # RAW_PREFILTERED allowed (the scan's contract)


@dataclass
class Case:
    name: str
    model: Model
    queries: List[str]
    threshold: tuple
    stop: bool
    score_threshold: float
    dq: List[int]
    D: int                                  # the batch's fastD (launch_plan.hpp): the largest d if it is 1..3, else 0
    qexact: List[bool]                      # the query has an exact anagram class in the lexicon
    fills: np.ndarray = None                # u32 [64]
    slots: np.ndarray = None                # u32 [total][2]: (query, entry index | flags) or (INVALID, 0)
    pairs: Dict[Tuple[int, int], Pair] = field(default_factory=dict)
    reserved: Dict[str, int] = field(default_factory=dict)

    def pair(self, q: int, e: int) -> Pair:
        p = self.pairs.get((q, e))
        if p is None:
            m = self.model
            lq, lc, ldf, lcs, pre, suf, same = m.measures(self.queries[q], e)
            dq = self.dq[q]
            ld = ldf if (ldf is not None and ldf <= dq) else None
            if ld is None:
                meta, score = META_NONE, float("nan")
            else:
                meta = ld | (int(same) << 7) | (lcs << 8) | (pre << 16) | (suf << 24)
                score = T.pair_score(m.weights, T.Distance(ld, lcs, pre, suf, same), lq)
            rows = m.rows_of(e)
            s, t = T.normalize_to_alphabet(self.queries[q], m.alphabet), m.norm[e]
            small = lq <= 16 and lc <= 16 and dq <= 3 and abs(lq - lc) <= dq
            brej = dq <= 3 and lq <= 32 and lc <= 32 and abs(lq - lc) <= dq and band_bound_rejects(s, t, dq)
            p = Pair(q, e, lq, lc, dq, ld, ldf, meta, score, m.freqs[e] if (m.have_freq and e < m.nwords) else 1, rows,
                     ld is not None and score >= self.score_threshold and rows > 0, brej,
                     m.bit_planes and not self.stop and small and not brej)
            self.pairs[(q, e)] = p
        return p


def _d_of(threshold, lq):
    return T.clamp_threshold(threshold, lq, T.MAX_EDIT_DISTANCE)


_CASES: Dict[str, Case] = {}


def case(name: str) -> Case:
    if name not in _CASES:
        _CASES[name] = _make_case(name)
    return _CASES[name]


def all_cases():
    return [case(n) for n in BATCHES]


def _make_case(name: str) -> Case:
    mname, threshold, stop, thr = BATCHES[name]
    m = model(mname)
    rng = random.Random(zlib.crc32(name.encode()))
    queries = [q for q in m.queries if len(q) <= QMAX.get(name, 255)]
    lqs = [len(T.normalize_to_alphabet(q, m.alphabet)) for q in queries]
    dq = [_d_of(threshold, n) for n in lqs]
    dmax = max(dq)
    sig = Counter(tuple(sorted(n)) for n in m.norm)
    qexact = [tuple(sorted(T.normalize_to_alphabet(q, m.alphabet))) in sig for q in queries]
    c = Case(name, m, queries, threshold, stop, 0.0, dq, dmax if 1 <= dmax <= 3 else 0, qexact)
    # candidate pairs: every query against the entries of similar length that share its first or last symbols, and a few others
    by_len = defaultdict(list)
    for e, n in enumerate(m.norm):
        by_len[len(n)].append(e)
    cand = []
    for q, text in enumerate(queries):
        s = T.normalize_to_alphabet(text, m.alphabet)
        near = [e for n in range(max(1, lqs[q] - 4), lqs[q] + 5) for e in by_len.get(n, ())]
        close = [e for e in near if m.norm[e][:2] == s[:2] or m.norm[e][-2:] == s[-2:] or m.norm[e][:1] == s[-1:]]
        cand += [(q, e) for e in close[:30]] + [(q, e) for e in rng.sample(near, min(3, len(near)))] + [(q, rng.randrange(len(m.norm)))]
    if thr == "cut":
        scores = sorted(c.pair(q, e).score for q, e in cand if c.pair(q, e).ld is not None)
        c.score_threshold = scores[len(scores) // 2]
        c.pairs.clear()
    c.cand = cand
    _layout(c, rng, small=mname == "f")
    return c


def _layout(c: Case, rng, small: bool):
    P = [c.pair(q, e) for q, e in c.cand]
    inline = lambda p: p.lq <= 16 and p.lc <= 16
    surv = [p for p in P if p.ld is not None and inline(p)]
    by_q = defaultdict(list)
    for p in surv:
        by_q[p.q].append(p)
    rich = sorted(by_q, key=lambda q: (-sum(p.keep for p in by_q[q]), -len(by_q[q])))
    # queries whose survivors are counted out by hand: they stay out of every random draw
    res = c.reserved
    nlen = Counter(p.lq for p in {p.q: p for p in P}.values())
    kept_q = [q for q in rich if any(p.keep for p in by_q[q]) and nlen[by_q[q][0].lq] > 3]   # (the grid keeps a query of every length)
    for key, q in zip(("one", "two", "thirtytwo"), kept_q[-3:] if len(kept_q) >= 8 else []):
        res[key] = q
    free = lambda p: p.q not in res.values()
    P = [p for p in P if free(p)]
    surv = [p for p in surv if free(p)]
    flag_ok = [p for p in P if p.flaggable]
    flag_surv = [p for p in flag_ok if p.ld is not None]
    flag_fail = [p for p in flag_ok if p.ld is None]
    flag_late = [p for p in flag_fail if p.ld_full is not None and p.ld_full <= c.D]   # queued by a byte-row short round, dropped at its drain
    unflag_fail = [p for p in P if p.ld is None and inline(p)]
    wide = [p for p in P if max(p.lq, p.lc) > 16 and abs(p.lq - p.lc) <= p.dq]   # past the length test: the slot lists' pairs
    short8 = [p for p in P if max(p.lq, p.lc) <= 8]
    mid12 = [p for p in P if 8 < max(p.lq, p.lc) <= 12]

    def word(p, flag=False, exact=False):
        return (p.q, p.e | (PRE if flag else 0) | (EXACT if exact else 0))

    def cell(ps, flag=False, n=WAVE):
        """n slots from the pairs ps (cycled), flagged where asked and allowed; a StopAtExactMatch batch marks a third of them exact"""
        out = []
        for i in range(n):
            p = ps[i % len(ps)]
            out.append(word(p, flag and p.flaggable, c.stop and (all_exact[0] or (i + p.e) % 3 == 0)))
        return out

    all_exact = [False]   # (the queue plan of a StopAtExactMatch batch: every pair of it in the exact class, nothing dropped)

    def draw(pool, n=WAVE):
        return [rng.choice(pool) for _ in range(n)] if pool else [rng.choice(P) for _ in range(n)]

    def grid_cells():
        """every (lq, lc) in 1..16 x 1..16 with |lq - lc| <= 3: one query per length against the nearest entry of each length"""
        m, out = c.model, []
        for lq in range(1, 17):
            qs = [q for q in range(len(c.queries)) if q not in res.values() and len(T.normalize_to_alphabet(c.queries[q], m.alphabet)) == lq]
            s = T.normalize_to_alphabet(c.queries[qs[0]], m.alphabet)
            for lc in range(max(1, lq - 3), min(16, lq + 3) + 1):
                es = [e for e in range(len(m.norm)) if len(m.norm[e]) == lc]
                out.append(c.pair(qs[0], max(es, key=lambda e: T.common_prefix_length(s, m.norm[e]))))
        out += draw(P, (-len(out)) % WAVE)
        return [cell(out[i:i + WAVE], i % 128 == 0) for i in range(0, len(out), WAVE)]

    def mixed_cells():
        """the wave classes: all-flagged, all-unflagged, mixed, invalid slots at lane 0 / lane 63 / in the middle / throughout, the prefilter forms"""
        cs = [cell(draw(P)), cell(draw(short8)), cell(draw(mid12) + draw(short8, 3), n=WAVE), cell(draw(wide or P)), cell(draw(P, 32) + draw(wide or P, 32))]
        if flag_ok:
            cs += [cell(draw(flag_ok), True), cell(draw(flag_surv or flag_ok), True), [w if i % 2 else word(rng.choice(flag_ok), True) for i, w in enumerate(cell(draw(P)))]]
            if flag_late:
                cs += [cell(draw(flag_late, 40) + draw(flag_surv, 24), True)]
        inv = (INVALID, 0)
        a, b, d, e = cell(draw(P)), cell(draw(P)), cell(draw(P)), cell(draw(flag_ok or P), bool(flag_ok))
        a[0] = inv
        b[63] = inv
        d[20:41] = [inv] * 21
        e[50:] = [inv] * 14      # an unused chunk tail behind prefiltered pairs
        cs += [a, b, d, e, [inv] * WAVE]
        rng.shuffle(cs)
        return cs

    regions: Dict[int, list] = {r: [] for r in USED_REGIONS}
    flat = lambda cells: [w for cl in cells for w in cl]
    xq = rich[0] if rich else 0                      # the query whose runs cross rounds, waves, blocks and regions
    xs = by_q.get(xq) or surv or P
    run_x = lambda flag: cell(sorted(xs, key=lambda p: p.e), flag)
    flagged_x = bool(flag_ok) and all(p.flaggable for p in xs)
    if small:
        regions[0] = flat(mixed_cells() + [run_x(flagged_x)] + mixed_cells())[:1000 - 37]
        regions[17] = flat(grid_cells() + mixed_cells())[:320]
        regions[63] = flat([run_x(False), cell(draw(P), n=6)])
    else:
        # region 0: two blocks, the second one ends in a partial round; X's run opens both blocks
        b0 = [run_x(flagged_x)] + mixed_cells() + mixed_cells() + mixed_cells()
        while len(b0) < 64:
            b0.append(cell(draw(P)))
        b1 = [run_x(flagged_x)] + mixed_cells()
        regions[0] = flat(b0[:64] + b1[:11]) + cell(draw(P), n=36)
        all_exact[0] = True
        regions[5] = _queue_region(c, rng, surv, unflag_fail, flag_surv, flag_fail, flag_late, xs, flagged_x, cell, draw, by_q)
        all_exact[0] = False
        regions[17] = flat([run_x(False)] + _segment_cells(c, by_q, cell, draw, P) + mixed_cells())
        regions[40] = flat(grid_cells() + mixed_cells()[:6])
        regions[63] = flat([run_x(flagged_x), cell(draw(P), n=6)])
    c.fills = np.zeros(REGIONS, dtype=np.uint32)
    rows = []
    for r in range(REGIONS):
        c.fills[r] = len(regions.get(r, ()))
        rows += regions.get(r, [])
    assert c.fills.max() <= 1 << REGION_SHIFT
    c.slots = np.array(rows, dtype=np.uint64).astype(np.uint32).reshape(-1, 2)


def _queue_region(c, rng, surv, fail, flag_surv, flag_fail, flag_late, xs, flagged_x, cell, draw, by_q):
    """One block of 12 rounds whose four waves fill their survivor queues by plan (S = 64 survivors, F = none, n = that many):
         wave 0: S S S S  S S S S  F F F F    192 without a drain, then exactly full (256); a second drain in the block
         wave 1: S S S 1  S 30 F F  F F F 7   a drain at 193, the smallest fill that drains, with a full round behind it; a small one in the last round
         wave 2: 5 F F F  F F F F  F F F F    a drain in the last round only (among its entries: pairs beyond the query's own d where a byte-row short round queues them)
         wave 3: the run shapes, 64 to a drain round: one run of 64 | q1 q2 q1 q2 .. (64 runs of 1) | .. X | X .. (a run across two drain
                 rounds) -> drain at 256; then the runs around the score threshold and the frequency maximum, drained at the end
       waves 0 and 3 are prefiltered (short rounds) where the model allows it, waves 1 and 2 are not (general rounds)."""
    sv = lambda flag: (flag_surv if flag and flag_surv else surv)
    fl = lambda flag: (flag_fail if flag and flag_fail else fail) or fail or flag_fail
    if not surv or not fl(False):
        return []
    f0 = bool(flag_surv) and bool(flag_fail)
    S = lambda flag: cell(draw(sv(flag)), flag)
    F = lambda flag: cell(draw(fl(flag)), flag)
    part = lambda k, flag, extra=(): cell(draw(sv(flag), k) + list(extra) + draw(fl(flag), WAVE - k - len(extra)), flag)
    w0 = [S(f0) for _ in range(8)] + [F(f0) for _ in range(4)]
    w1 = [S(False) for _ in range(3)] + [part(1, False), S(False), part(30, False)] + [F(False) for _ in range(5)] + [part(7, False)]
    late = draw(flag_late, 9) if flag_late else []
    w2 = [part(5, bool(late), late)] + [F(False) for _ in range(11)]
    # wave 3
    qs = [q for q in by_q if q not in c.reserved.values() and (not f0 or all(p.flaggable for p in by_q[q]))]
    qs.sort(key=lambda q: -len(by_q[q]))
    one = lambda q, i=0: by_q[q][i % len(by_q[q])]
    q1, q2 = (qs + qs)[1], (qs + qs)[2]
    alt = [one(q1, i // 2) if i % 2 == 0 else one(q2, i // 2) for i in range(WAVE)]
    many = [one(qs[i % len(qs)], i) for i in range(WAVE)]
    if len(qs) > 1:   # neighbours differ
        for i in range(1, WAVE):
            if many[i].q == many[i - 1].q:
                many[i] = one(qs[(i + 1) % len(qs)], i)
    xrun = sorted(xs, key=lambda p: p.e)
    xf = f0 and flagged_x
    tail_x = draw([p for p in sv(xf) if p.q != xrun[0].q] or sv(xf), 40) + [xrun[i % len(xrun)] for i in range(24)]
    head_x = [xrun[i % len(xrun)] for i in range(30)] + draw([p for p in sv(xf) if p.q != xrun[0].q] or sv(xf), 34)
    w3 = [cell([xrun[i % len(xrun)] for i in range(WAVE)], xf), cell(alt, f0), cell(tail_x, xf), cell(head_x, xf)]
    # runs of one query ordered by what the counters see: below-threshold survivors first / last / only, the largest frequency first / last
    shaped = []
    for q in qs[:40]:
        ps = by_q[q]
        lo, hi = [p for p in ps if not p.keep], [p for p in ps if p.keep]
        if lo and hi:
            shaped += [lo[:2] + hi[:3], hi[:3] + lo[:2]]
        if len(lo) >= 2:
            shaped += [lo[:4]]
        fs = sorted(ps, key=lambda p: p.freq)
        if len(fs) >= 2 and fs[-1].freq > fs[-2].freq:
            shaped += [[fs[-1]] + fs[:-1][:3], fs[:-1][:3] + [fs[-1]]]
    runs, prev = [], None
    for run in shaped:
        if run[0].q != prev and len(runs) + len(run) <= 4 * WAVE:
            runs += run
            prev = run[0].q
    runs += draw(sv(f0), (-len(runs)) % WAVE)
    w3 += [cell(runs[i:i + WAVE], f0) for i in range(0, len(runs), WAVE)] + [cell(many, f0)]
    w3 = (w3 + [F(f0) for _ in range(12)])[:12]
    out = []
    for r in range(12):
        for w in (w0, w1, w2, w3):
            out += w[r]
    return out


def _segment_cells(c, by_q, cell, draw, P):
    """the reserved queries: exactly 1, 2 and 32 kept survivors in the whole pair list (segments of 2 and 32: fewer, exactly, more --
    every other query with survivors supplies `more`)"""
    out = []
    for key, n in (("one", 1), ("two", 2), ("thirtytwo", 32)):
        if key in c.reserved:
            kept = [p for p in by_q[c.reserved[key]] if p.keep]
            out += [kept[i % len(kept)] for i in range(n)]
    # queries whose kept survivors come from two kernels: a string of 16 symbols beside one of 17 (inline + k_score_fast8), one of 32 beside
    # one of 33 (k_score_fast8 + k_score_pairs)
    kern = defaultdict(lambda: defaultdict(list))
    for p in P:
        if p.keep:
            kern[p.q]["inline" if max(p.lq, p.lc) <= 16 else "fast8" if max(p.lq, p.lc) <= 32 else "pairs"].append(p)
    for want in (("inline", "fast8"), ("fast8", "pairs")):
        for q in [q for q in kern if all(k in kern[q] for k in want)][:3]:
            out += [kern[q][k][0] for k in want]
    cells = []
    if out:
        out += draw(P, (-len(out)) % WAVE)
        cells = [cell(out[i:i + WAVE]) for i in range(0, len(out), WAVE)]
    return cells


# ---- expectation --------------------------------------------------------------------------------------------------------------------------
@dataclass
class Expect:
    meta: np.ndarray        # u32 per slot
    score: np.ndarray       # f64 per slot, nan where the slot has no distance
    skipped: np.ndarray     # bool per slot: StopAtExactMatch dropped the pair
    region: np.ndarray      # region of every slot
    qsurv: np.ndarray
    qmaxfreq: np.ndarray
    qexpand: np.ndarray
    kept: Counter           # (region, query, entry index, score) -> multiplicity
    n_skipped: int


def slot_pair(c: Case, i: int) -> Optional[Pair]:
    q, w = int(c.slots[i, 0]), int(c.slots[i, 1])
    return None if q == INVALID else c.pair(q, w & 0x3FFFFFF)


def is_skipped(c: Case, q: int, w: int) -> bool:
    """src/lib.rs:1164-1173 as the pair list carries it: a pair outside the exact class of a query that has one"""
    return c.stop and not (w & EXACT) and c.qexact[q]


def expect(c: Case) -> Expect:
    n, nq, m = len(c.slots), len(c.queries), c.model
    ex = Expect(np.full(n, META_SKIPPED, dtype=np.uint32), np.full(n, np.nan), np.zeros(n, dtype=bool), np.repeat(np.arange(REGIONS), c.fills),
                np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32), Counter(), 0)
    for i in range(n):
        q, w = int(c.slots[i, 0]), int(c.slots[i, 1])
        if q == INVALID:
            continue
        if is_skipped(c, q, w):
            ex.skipped[i] = True
            ex.n_skipped += 1
            continue
        p = c.pair(q, w & 0x3FFFFFF)
        ex.meta[i] = p.meta
        if p.ld is None:
            continue
        ex.score[i] = p.score
        ex.qmaxfreq[q] = max(int(ex.qmaxfreq[q]), p.freq)          # before the threshold (src/lib.rs:1454-1462)
        if m.twin.decoder[3 + p.e].variants is not None:
            ex.qexpand[q] = 1
        if p.keep:
            ex.qsurv[q] += p.rows
            ex.kept[(int(ex.region[i]), q, p.e, p.score)] += 1
    return ex


# ---- census -------------------------------------------------------------------------------------------------------------------------------
def route(c: Case, p: Pair, w: int, general: bool) -> str:
    """where k_filter_score sends a live, valid, unskipped slot: `short` (inline, short round), `inline`, `lenrej`, `bandrej`, `list8`,
    `listg`, `listw>bandrej` / `listw>list8` / `listw>listg` (k_filter_wide's verdict)"""
    pre = bool(w & PRE)
    D = c.D
    if pre and not general and D > 0:
        return "short"
    if not pre and abs(p.lq - p.lc) > p.dq:
        return "lenrej"
    filt = not pre and p.dq <= 3 and p.lq <= 32 and p.lc <= 32
    use8 = D > 0 and p.lq <= 32 and p.lc <= 32 and p.dq <= D
    if filt and (p.lq > 16 or p.lc > 16):
        return "listw>" + ("bandrej" if p.bandrej else "list8" if use8 else "listg")
    if filt and p.bandrej:
        return "bandrej"
    if D > 0 and (pre or (p.lq <= 16 and p.lc <= 16 and p.dq <= D)):
        return "inline"
    return "list8" if use8 else "listg"


def census(c: Case, blk: int = FS_BLK, planes: Optional[bool] = None) -> Counter:
    """Counter of the classes the launch takes with blocks of blk slots.  planes: the short round tests the query's own d (symbol planes,
    MODE 2) instead of the batch's D (byte rows); default: what the model's alphabet selects."""
    planes = c.model.nclasses <= 61 and c.model.nclasses + 1 < 0x7E if planes is None else planes
    t = Counter()
    D = c.D
    off = [0] + [int(x) for x in np.cumsum(c.fills.astype(np.int64))]
    where = defaultdict(set)      # query -> (region, block, wave) of the drains its runs lie in
    kernels = defaultdict(set)    # query -> kernels its kept survivors come from
    nkept = Counter()
    lists = Counter()
    for region in range(REGIONS):
        fill = int(c.fills[region])
        t["region_empty" if fill == 0 else "region_used"] += 1
        if fill:
            t["region_%d" % region if region in (0, 63) else "region_between"] += 1
        if fill > blk:
            t["region_blocks>1"] += 1
        for base in range(0, fill, blk):
            lim = min(fill, base + blk)
            nrounds = (lim - base + ROUND - 1) // ROUND
            if (lim - base) % ROUND:
                t["block_partial_round"] += 1
            for w in range(4):
                queue, drains, drained_193 = [], [], False
                for r in range(nrounds):
                    lanes = []
                    for lane in range(WAVE):
                        idx = base + r * ROUND + WAVE * w + lane
                        if idx >= lim:
                            lanes.append(None)
                            continue
                        q, word = int(c.slots[off[region] + idx, 0]), int(c.slots[off[region] + idx, 1])
                        lanes.append(("inv",) if q == INVALID else (q, word, c.pair(q, word & 0x3FFFFFF)))
                    live = [x for x in lanes if x is not None]
                    valid = [x for x in live if x[0] != "inv"]
                    last = r == nrounds - 1
                    if live:
                        npre = sum(1 for x in valid if x[1] & PRE)
                        if not valid:
                            t["wave_invalid_only"] += 1
                        else:
                            t["wave_all_flagged" if npre == len(valid) else "wave_unflagged" if npre == 0 else "wave_mixed"] += 1
                            if len(live) == WAVE:
                                inv = [i for i, x in enumerate(lanes) if x[0] == "inv"]
                                for name, hit in (("invalid_lane0", 0 in inv), ("invalid_lane63", 63 in inv), ("invalid_middle", any(0 < i < 63 for i in inv))):
                                    t[name] += hit
                        general = npre < len(valid)
                        added = 0
                        forms = []
                        for x in valid:
                            q, word, p = x
                            if is_skipped(c, q, word):
                                t["route_skipped"] += 1
                                continue
                            ro = route(c, p, word, general)
                            t["route_" + ro] += 1
                            lists["w"] += ro.startswith("listw")
                            lists["8"] += ro.endswith("list8")
                            lists["g"] += ro.endswith("listg")
                            lists["selected"] += ro in ("short", "inline", "list8", "listg", "listw>list8", "listw>listg")
                            if general and not (word & PRE) and ro in ("bandrej", "inline", "list8", "listg"):
                                if p.dq <= 3 and p.lq <= 16 and p.lc <= 16:
                                    forms.append(max(p.lq, p.lc))
                            kern = "inline" if ro in ("short", "inline") else "fast8" if ro.endswith("list8") else "pairs" if ro.endswith("listg") else None
                            if kern and p.keep:
                                kernels[q].add(kern)
                                nkept[q] += 1
                            if ro == "short":
                                bound = p.dq if planes else D
                                if p.ld_full is not None and p.ld_full <= bound:
                                    queue.append(p)
                                    added += 1
                            elif ro == "inline" and p.ld is not None:
                                queue.append(p)
                                added += 1
                        if forms:
                            t["form_le8" if max(forms) <= 8 else "form_9_12" if max(forms) <= 12 else "form_13_16"] += 1
                        if D > 0 and len(queue) == FS_SURV and added == WAVE and len(queue) - added == FS_SURV - WAVE:
                            t["queue_192_then_full"] += 1
                        t["drain_at_193_then_full_round"] += drained_193 and added == WAVE
                    drained_193 = D > 0 and len(queue) == FS_SURV - WAVE + 1 and not last
                    if D > 0 and (len(queue) > FS_SURV - WAVE or last):
                        assert len(queue) <= FS_SURV
                        if queue:
                            drains.append((len(queue), last))
                            if FS_SURV - WAVE < len(queue) < FS_SURV and not last:
                                t["drain_193_255"] += 1
                            _census_drain(c, t, queue, where, (region, base // blk, w))
                        queue = []
                if len(drains) >= 2:
                    t["drains>=2_in_block"] += 1
                if len(drains) == 1 and drains[0][1] and nrounds > 1:
                    t["drain_last_round_only"] += 1
    for q, ws in where.items():
        t["run_next_wave"] += len({(r, b) for r, b, _ in ws}) < len(ws)
        t["run_next_block"] += len({r for r, _, _ in ws}) < len({(r, b) for r, b, _ in ws})
        t["run_other_region"] += len({r for r, _, _ in ws}) > 1
    for C in SEG_CAPS:
        for q, n in nkept.items():
            t["seg%d_%s" % (C, "lt" if n < C else "eq" if n == C else "gt")] += 1
    for q, ks in kernels.items():
        if len(ks) > 1:
            t["kernels_" + "+".join(sorted(ks))] += 1
    t["need_listw"], t["need_list8"], t["need_listg"], t["need_selected"] = lists["w"], lists["8"], lists["g"], lists["selected"]
    return t


def _census_drain(c, t, queue, where, at):
    """the runs of equal queries survivor_counts sees in each dense round of 64 of a drain"""
    has = [p.ld is not None for p in queue]
    t["drain_fails_own_d"] += sum(1 for h in has if not h)
    for r0 in range(0, len(queue), WAVE):
        keys = [(p.q if h else None) for p, h in zip(queue[r0:r0 + WAVE], has[r0:r0 + WAVE])]
        keys += [None] * (WAVE - len(keys))
        runs, i = [], 0
        while i < WAVE:
            j = i
            while j + 1 < WAVE and keys[j + 1] == keys[i]:
                j += 1
            if keys[i] is not None:
                runs.append((i, j))
                where[keys[i]].add(at)
            i = j + 1
        t["run_start_lane0"] += any(a == 0 for a, _ in runs)
        t["run_end_lane63"] += any(b == 63 for _, b in runs)
        t["run_of_64"] += (0, 63) in runs
        t["runs_64_of_1"] += len(runs) == WAVE
        t["runs_interleaved"] += any(keys[i] is not None and keys[i + 1] is not None and keys[i] == keys[i + 2] != keys[i + 1] for i in range(WAVE - 2))
        if r0 + WAVE < len(queue) and keys[63] is not None and has[r0 + WAVE] and queue[r0 + WAVE].q == keys[63]:
            t["run_next_drain_round"] += 1
        for a, b in runs:
            ps = queue[r0 + a:r0 + b + 1]
            if len(ps) < 2:
                continue
            keep = [p.keep for p in ps]
            t["run_below_head"] += (not keep[0]) and any(keep)
            t["run_below_tail"] += (not keep[-1]) and any(keep)
            t["run_below_all"] += not any(keep)
            fr = [p.freq for p in ps]
            t["run_maxfreq_first"] += fr[0] > max(fr[1:])
            t["run_maxfreq_last"] += fr[-1] > max(fr[:-1])


def coverage(c: Case) -> Counter:
    """the pair classes among the slots (skipped and invalid ones aside): lengths, distances at the query's d and just beyond it, what the
    band-match bound rejects, the symbol codes, case"""
    t = Counter()
    m = c.model
    unk, top = m.nclasses + 1, m.nclasses - 1
    seen = set()
    for i in range(len(c.slots)):
        q, w = int(c.slots[i, 0]), int(c.slots[i, 1])
        if q == INVALID or is_skipped(c, q, w) or (q, w) in seen:
            continue
        seen.add((q, w))
        p = c.pair(q, w & 0x3FFFFFF)
        s, e = T.normalize_to_alphabet(c.queries[q], m.alphabet), m.norm[p.e]
        t[("len", p.lq, p.lc)] += 1
        hit = p.ld is not None
        for a, b in ((16, 17), (32, 33)):
            t["border_%d_%d" % (a, b)] += hit and min(p.lq, p.lc) <= a < b <= max(p.lq, p.lc)
        t["len_240_255"] += hit and max(p.lq, p.lc) >= 240
        t["len_255"] += hit and max(p.lq, p.lc) == 255
        t["equal"] += s == e
        t["ld_eq_d"] += hit and p.ld == p.dq and p.dq > 0
        t["ld_eq_d+1"] += p.ld_full == p.dq + 1
        t["d%d" % p.dq] += 1
        if p.dq == 1 and c.D == 3 and (w & PRE):
            t["d1_in_D3_ld%s" % p.ld_full] += 1
        t["bandrej"] += p.bandrej
        t["unk_query"] += unk in s
        t["unk_entry"] += hit and unk in e
        t["top_code"] += hit and top in s and top in e
        t["samecase_false"] += hit and not (p.meta >> 7) & 1
        t["upper_query"] += hit and c.queries[q][0].isupper()
        t["upper_entry"] += hit and m.texts[p.e][0].isupper()
        t["transparent"] += hit and m.twin.decoder[3 + p.e].transparent
        t["no_rows"] += hit and p.rows == 0
        t["rows>1"] += hit and p.rows > 1
        t["repeated"] += hit and p.ld > 0 and len(set(s)) <= 2 and len(s) >= 4
        if hit and p.ld >= 2 and p.ld < levenshtein_plain(s, e):
            t["transposition_with_gap"] += _osa(s, e) > p.ld     # cheaper than the restricted distance: the 1 + a + b term
            t["transposition"] += 1
        if hit and p.ld == 1 and len(s) == len(e) and len(s) >= 2:
            t["transposition_first"] += s[:2] == e[1::-1] and s[0] != s[1] and s[2:] == e[2:]
            t["transposition_last"] += s[-2:] == e[:-3:-1] and s[-1] != s[-2] and s[:-2] == e[:-2]
    return t


def levenshtein_plain(s, t) -> int:
    prev = list(range(len(t) + 1))
    for i, a in enumerate(s, 1):
        cur = [i]
        for j, b in enumerate(t, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a != b)))
        prev = cur
    return prev[-1]


def _osa(s, t) -> int:
    """the restricted (optimal string alignment) distance: adjacent transpositions only"""
    d = [[max(i, j) if min(i, j) == 0 else 0 for j in range(len(t) + 1)] for i in range(len(s) + 1)]
    for i in range(1, len(s) + 1):
        for j in range(1, len(t) + 1):
            d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (s[i - 1] != t[j - 1]))
            if i > 1 and j > 1 and s[i - 1] == t[j - 2] and s[i - 2] == t[j - 1]:
                d[i][j] = min(d[i][j], d[i - 2][j - 2] + 1)
    return d[len(s)][len(t)]
