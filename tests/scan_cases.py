"""Cases and reference for the scan stage by itself (kernels_scan.hpp: k_scan_adj, k_scan_bits, k_scan_sad, k_scan_small), as
tests/test_gpu_scan_door.py sends them through anx_debug_scan_pairs.  Plain Python and numpy, no GPU.

The reference is the set the kernel's header states, computed from the strings alone: for a query q with clamped anagram distance k the
ENTRIES whose class c has L1(cv_q, cv_c) <= k, |len_c - len_q| <= k and a symbol in common with q (cv = the count vector over the
alphabet's classes and the unknown symbol; k and d clamped per query length by the twin's clamp_threshold).  Per reference pair three
properties follow from the strings and the stage's plain arguments:

  * materialised: drop_len off, or |lc - lq| <= d;
  * band-rejected: the tile fuses (bit-plane tile, fuse on, lq <= 16, d <= 3), the pair passed the length test, lc <= 16 and
    score_cases.band_bound_rejects says the distance is beyond d;
  * the flag bits of a written pair: RAW_PREFILTERED iff the tile fuses and lc <= 16; bit 31 iff want_exact and the entry's class is the
    query's exact class (equal count vectors).

tests/test_scan_cases_cpu.py ties this statement to the twin's find_nearest_anahashes and the C oracle's n_pairs, and asserts that the
classes of inputs the GPU test relies on are populated.  Entries are named by their position in the vocabulary (vocabulary id - 3)."""
import random
from collections import Counter
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

import score_cases as SC
from oracle import twin as T

REGIONS = 64
RC_STRIDE = 32
RC_RAW, RC_VALID, RC_FUSED, RC_TESTS, RC_ADJ, RC_ADJ_FIRST = 0, 1, 2, 4, 14, 15   # kernels_scan.hpp
INVALID = 0xFFFFFFFF
FILL = 0xFEFEFEFE      # what the door's buffers start as: neither RAW_INVALID nor a pair
PRE = 1 << 30          # RAW_PREFILTERED
EXACT = 1 << 31
ENTRY_MASK = (1 << 30) - 1
SCAN_MASKW = 2048      # kernels_common.hpp
SCAN_HITS = 512
SCAN_PBUF = 128
TILE_WORDS = 15
T_Q0, T_NQ, T_S0, T_S1, T_K, T_LQ, T_SIGLO, T_SIGHI, T_KIND, T_D, T_KEND, T_BALL0, T_BALLN, T_ADJ, T_FLAGS = range(15)

# the lexicon of tests/test_gpu_scan_twins.py: anagram sets of six letters, kind 1 (no letter twice) and kind 2 (a doubled letter)
LISTEN = ["listen", "silent", "enlist", "tinsel", "inlets"]
MASTER = ["master", "stream", "tamers"]
DANGER = ["danger", "garden", "gander"]
DETEST = ["detest", "tested"]
LETTER = ["letter"]
SINGLES = ["planet", "forest", "bridge", "copied", "jumble"]
KIND1 = LISTEN + MASTER + DANGER + SINGLES                      # six different letters
KIND2 = ["detest", "tested", "letter", "tester", "litter"]    # a doubled letter
KEND_CASES = {"lex1-kend32": (32, 10), "lex1-kend31": (31, 10), "lex1-kend33": (33, 10), "lex1-kend-last": (41, 1), "lex1-kend-last-of-pass": (31, 1)}
LEXICON = LISTEN + MASTER + DANGER + DETEST + LETTER + SINGLES + [
    "listens", "listed", "list", "lists", "inlet", "stone", "notes", "onset", "liste", "silents", "tinsels", "masters", "streams",
    "dangers", "gardens", "tester", "detests", "letters", "latter", "litter", "planets", "forests", "bridges", "lister", "linted",
    "minted", "salted", "tilted", "sifted", "lasted", "mister", "muster", "garner", "grader", "danker", "hanger", "ranged"]


WIDE_CENTER_IDX = (0, 1, 2, 3, 4, 5, 6, 7)   # the "wide" model's dense neighbourhood: eight different symbols of its pool of ten


# ---- models -----------------------------------------------------------------------------------------------------------------------------
@dataclass
class Model:
    name: str
    alphabet: List[List[str]]
    texts: List[str]
    switches: Tuple[Tuple[str, str], ...] = ()     # read when the model is built (ANX_SIG_GROUPS)
    twin: T.VariantModel = None
    norm: List[List[int]] = None
    cv: np.ndarray = None        # [entries, classes + 1] count vectors
    lens: np.ndarray = None
    cls: np.ndarray = None       # class number of every entry (equal count vectors = equal number)

    @property
    def nclasses(self):
        return len(self.alphabet)

    @property
    def bit_planes(self):   # encode.hip bits_ok: at most 32 hash symbols, the classes and the unknown one
        return self.nclasses + 1 <= 32

    def alphabet_text(self) -> str:
        return "".join("\t".join(cl) + "\n" for cl in self.alphabet)

    def lexicon_text(self) -> str:
        return "".join(w + "\n" for w in self.texts)

    def finish(self):
        tm = T.VariantModel(self.alphabet, T.Weights())
        for i, w in enumerate(self.texts):
            assert tm.add_to_vocabulary(w) == 3 + i, w
        tm.build()
        self.twin = tm
        self.norm = [v.norm for v in tm.decoder[3:]]
        self.cv = np.stack([self.count_vector(s) for s in self.norm])
        self.lens = np.array([len(s) for s in self.norm], dtype=np.int64)
        ids: Dict[bytes, int] = {}
        self.cls = np.array([ids.setdefault(v.tobytes(), len(ids)) for v in self.cv], dtype=np.int64)
        return self

    def count_vector(self, codes) -> np.ndarray:
        return np.bincount(np.asarray(codes, dtype=np.int64), minlength=self.nclasses + 1).astype(np.int16)


def _unique(xs):
    return list(dict.fromkeys(x for x in xs if x))


def _five_strings(rng, n, lengths, letters="abcde"):
    out = []
    while len(out) < n:
        ln = rng.choice(lengths)
        mode = rng.randrange(4)
        if mode == 0 and ln <= len(letters):
            w = "".join(rng.sample(letters, ln))                       # no letter twice: kind 1
        elif mode == 1:
            w = "".join(rng.choice(letters[:3]) for _ in range(ln))    # few letters: high multiplicities
        else:
            w = "".join(rng.choice(letters) for _ in range(ln))
        out.append(w)
    return out


def _make_model(name: str) -> Model:
    a26, rng = SC._alphabet(26), random.Random(sum(map(ord, name)))
    if name in ("lex", "lex1"):
        return Model(name, a26, list(LEXICON), (("ANX_SIG_GROUPS", "1"),) if name == "lex1" else ()).finish()
    if name == "five":
        # a few hundred strings over five letters, lengths 1 .. 18: dense lists and hit masks; kinds 1 .. 4 and count vectors (a letter
        # five times and more) in one model; entries of 17 symbols next to 16-symbol ones, and one of 255
        ws = _five_strings(rng, 520, [1, 2, 3, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 10, 11, 12, 13, 14, 15, 16, 16, 17, 17, 18])
        base16 = ["abcdeabcdeabcdea", "aabbccddeeabcdab", "abcabcabcabcdede"]
        ws += base16 + [w + "b" for w in base16] + [w[:8] + "c" + w[8:] for w in base16] + [w[:-1] for w in base16] + ["abcde" * 51]
        ws += ["a", "b", "ab", "ba", "abc", "cab", "aab", "abcd", "abdc"]
        return Model(name, a26, _unique(ws)).finish()
    if name == "five1":
        # ONE signature group (the signature is the length) and more than SCAN_MASKW entries of one length: one run of two windows
        ws = _five_strings(rng, 4400, [7]) + _five_strings(rng, 300, [5, 6, 8, 9]) + _five_strings(rng, 1150, [11])   # (length 11: a list of about twenty rows)
        m = Model(name, a26, _unique(ws), (("ANX_SIG_GROUPS", "1"),)).finish()
        assert int((m.lens == 7).sum()) > SCAN_MASKW
        return m
    if name == "wide":
        # 70 classes: every tile compares count vectors, and the count-vector kernel's instance is the wider one
        a70 = SC._alphabet(70)
        sym = [cl[0] for cl in a70]
        ws = []
        for _ in range(420):
            ln = rng.choice([1, 2, 3, 4, 5, 6, 6, 7, 8, 9, 10, 12])
            pool = sym[:6] if rng.random() < 0.7 else sym
            ws.append("".join(rng.choice(pool) for _ in range(ln)))
        # every class within L1 distance 3 of WIDE_CENTER over ten symbols: one query hits more classes than the hit list of a
        # count-vector tile holds between two expansions
        pool = sym[10:20]
        near = {tuple(sorted(WIDE_CENTER_IDX))}
        for _ in range(3):
            step = set()
            for c in near:
                for i in range(len(c)):
                    step.add(c[:i] + c[i + 1:])
                for x in range(len(pool)):
                    step.add(tuple(sorted(c + (x,))))
            near |= step
        ws += ["".join(pool[i] for i in c) for c in sorted(near) if c]
        return Model(name, a70, _unique(ws)).finish()
    raise KeyError(name)


_MODELS: Dict[str, Model] = {}


def model(name: str) -> Model:
    if name not in _MODELS:
        _MODELS[name] = _make_model(name)
    return _MODELS[name]


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    model: Model
    queries: List[str]
    kth: tuple
    dth: tuple
    stop: bool = False
    switches: Tuple[Tuple[str, str], ...] = ()   # read when the batch is encoded
    small_slots: int = 0                         # > 0: the small form with this many tile slots per query
    _ref: list = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = reference(self.model, self.queries, self.kth, self.dth)
        return self._ref


def _mutants(rng, words, n, letters):
    out = []
    for _ in range(n):
        w = rng.choice(words)
        r = rng.randrange(6)
        p = rng.randrange(len(w))
        if r == 0:
            w = w[:p] + rng.choice(letters) + w[p + 1:]
        elif r == 1:
            w = w[:p] + rng.choice(letters) + w[p:]
        elif r == 2 and len(w) > 1:
            w = w[:p] + w[p + 1:]
        elif r == 3 and len(w) > 1:
            p = min(p, len(w) - 2)
            w = w[:p] + w[p + 1] + w[p] + w[p + 2:]
        elif r == 4:
            w = w + rng.choice(letters) + rng.choice(letters)
        out.append(w)
    return out


def _five_queries(rng, m, n):
    short = [w for w in m.texts if len(w) <= 20]
    qs = rng.sample(short, min(len(short), n // 3)) + _mutants(rng, short, n - n // 3 - 12, "abcde")
    # the length borders of the fused filter and the clamps: lq = 1, 2, 3, 16, 17
    qs += ["a", "c", "ab", "ca", "abc", "bca", "abcdeabcdeabcdea", "abcdeabcdeabcdeab", "aabbccddeeabcdab", "aabbccddeeabcdabc", "abcabcabcabcdede", "bacabcabcabcdede"]
    return qs


def _make_cases() -> Dict[str, Case]:
    rng = random.Random(20)
    lex, lex1, five, five1, wide = model("lex"), model("lex1"), model("five"), model("five1"), model("wide")
    K3, D2 = ("abs", 3), ("abs", 2)
    cs = [
        # tile sizes and twins (tests/test_gpu_scan_twins.py's tiles)
        Case("lex-1", lex, ["listen"], K3, D2),
        Case("lex-31", lex, ["listen"] * 31, K3, D2),
        Case("lex-32", lex, ["listen"] * 32, K3, D2),
        Case("lex-33", lex, ["listen"] * 33, K3, D2),
        Case("lex-40-tq64", lex, ["listen"] * 40, K3, D2, switches=(("ANX_SCAN_TQ", "64"),)),
        Case("lex-anagrams", lex, LISTEN + ["lisetn", "isletn", "tinsle", "enlits", "slient"], K3, D2),
        Case("lex1-twins-first-last", lex1, [w for ws in zip(LISTEN, MASTER + MASTER[:2], DANGER + DANGER[:2]) for w in ws], K3, D2),
        Case("lex1-no-twins", lex1, ["listen", "master", "danger"] + SINGLES, K3, D2),
        Case("lex1-all-twins", lex1, ["detest"] * 7 + ["listen"] * 9, K3, D2),
        Case("lex1-kind-boundary", lex1, ["silent", "detest", "listen", "tested", "enlist", "detest", "letter", "planet", "letter", "forest"], K3, D2),
        # 33 .. 64 queries in one tile, two passes, kinds 1 and 2 in both
        Case("lex1-50-tq64", lex1, (LISTEN + DETEST + SINGLES + MASTER + LETTER + DANGER + ["tester", "litter"]) * 2 + ["listen"] * 8, K3, D2, switches=(("ANX_SCAN_TQ", "64"),)),
    ]
    # a kind boundary AT the border of the passes (kend0 = 32), one query before and behind it, and at the tile's last query: the twin mask
    # is cut at (lane & 31) == 0 and at every kend, both at once here.  One group and tiles of 64: the tile is the length's queries, kind 1 first.
    for nm, (n1, n2) in KEND_CASES.items():
        cs.append(Case(nm, lex1, (KIND1 * 3)[:n1] + (KIND2 * 3)[:n2], K3, D2, switches=(("ANX_SCAN_TQ", "64"),)))
    # many tiles: more than 256, more than 64 in a launch, signatures beyond the closure of the lexicon (ball probes), short queries
    many = list(LEXICON) + _mutants(rng, LEXICON, 150, "abcdefghijklmnopqrstuvwxyz")
    many += ["".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 9, 10]))) for _ in range(330)]
    cs.append(Case("lex-many", lex, many, K3, D2))
    fq = _five_queries(rng, five, 330)
    f1q = rng.sample(five1.texts, 20) + _mutants(rng, five1.texts, 16, "abcde")   # (one list for the three walks: their pairs are the same)
    # five symbols: kinds 1 .. 4 in the one tile of the length; 11 .. 13: a short list
    f1q += ["abcde", "bacde", "aabcd", "abbcd", "aaabc", "abbbc", "aaaab", "abbbb", "abcdeabcdea", "aabbccddeea", "abcdeabcdeab", "abcdeabcdeabc"]
    for k, d in ((3, 2), (3, 3), (2, 2), (2, 1), (1, 1), (0, 0), (3, 1)):
        cs.append(Case("five-k%dd%d" % (k, d), five, fq, ("abs", k), ("abs", d)))
    # bit-plane queries only: no tile is cut into parts, so every region counter is exact
    cs.append(Case("five-bits", five, [q for q in fq if 1 <= max(Counter(q).values()) <= 4], K3, D2))
    cs += [
        Case("five-flat", five, fq, K3, D2, switches=(("ANX_SCAN_WALK", "flat"), ("ANX_SCAN_ADJ", "0"))),
        Case("five-noadj", five, fq, K3, D2, switches=(("ANX_SCAN_ADJ", "0"),)),
        Case("five-host", five, fq, K3, D2, switches=(("ANX_ENCODE", "host"),)),
        Case("five-tq64", five, fq, K3, D2, switches=(("ANX_SCAN_TQ", "64"),)),
        Case("five-stop", five, fq, K3, D2, stop=True),
        # one group: the tiles are the lengths; a run of more than SCAN_MASKW ids, dense hit lists, the ring wraps
        Case("five1-run", five1, f1q, K3, D2),
        Case("five1-run-noadj", five1, f1q, K3, D2, switches=(("ANX_SCAN_ADJ", "0"),)),
        Case("five1-run-flat", five1, f1q, K3, D2, switches=(("ANX_SCAN_ADJ", "0"), ("ANX_SCAN_WALK", "flat"))),
        Case("wide", wide, ["".join(SC._alphabet(70)[10 + i][0] for i in WIDE_CENTER_IDX)] * 2 + rng.sample(wide.texts, 150) + _mutants(rng, wide.texts, 150, "".join(cl[0] for cl in wide.alphabet[:8])), K3, D2),
        Case("wide-k1", wide, rng.sample(wide.texts, 60) + _mutants(rng, wide.texts, 60, "".join(cl[0] for cl in wide.alphabet[:8])), ("abs", 1), ("abs", 1)),
    ]
    # a threshold that exceeds the strings: k = 3 for a query of one symbol, so lq + lc - 1 < k and the count-vector test takes its
    # threshold from `share` (a ratio above 1 with a limit; an absolute k is clamped to lq / 2 and never gets there)
    short = [w for w in wide.texts if len(w) <= 3]
    cs.append(Case("wide-share", wide, rng.sample(short, min(len(short), 50)) + [cl[0] for cl in wide.alphabet[:12]] + [cl[0] * 2 for cl in wide.alphabet[:4]],
                   ("ratiolimit", 3.0, 3), ("ratiolimit", 3.0, 3)))
    # the small form: 1, 64, 129 and 600 inputs with 32, 32, 16 and 8 tile slots per query
    sq = ["qrstuv", "xyzzyx", "mnopq", "abcxyz"] + [q for q in fq if len(q.encode()) <= 64]   # (the first: signatures no list covers)
    sq = (sq * 3)[:600]
    for n, slots in ((1, 32), (64, 32), (129, 16), (600, 8)):
        cs.append(Case("small-%d" % n, five, sq[7:8] if n == 1 else sq[:n], K3, D2, small_slots=slots))
    cs.append(Case("small-five1", five1, f1q, K3, D2, small_slots=32))
    cs.append(Case("small-wide", wide, rng.sample(wide.texts, 40), K3, D2, small_slots=32))
    return {c.name: c for c in cs}


_CASES: Optional[Dict[str, Case]] = None


def cases() -> Dict[str, Case]:
    global _CASES
    if _CASES is None:
        _CASES = _make_cases()
    return _CASES


def case(name: str) -> Case:
    return cases()[name]


BATCH_CASES = ["lex-1", "lex-31", "lex-32", "lex-33", "lex-40-tq64", "lex-anagrams", "lex1-twins-first-last", "lex1-no-twins", "lex1-all-twins",
               "lex1-kind-boundary", "lex1-50-tq64", "lex1-kend32", "lex1-kend31", "lex1-kend33", "lex1-kend-last", "lex1-kend-last-of-pass", "lex-many", "five-bits", "five-k3d2", "five-k3d3", "five-k2d2", "five-k2d1", "five-k1d1", "five-k0d0", "five-k3d1",
               "five-flat", "five-noadj", "five-host", "five-tq64", "five1-run", "five1-run-noadj", "five1-run-flat", "wide", "wide-k1", "wide-share"]
STOP_CASES = ["five-stop"]   # a batch encoded for StopAtExactMatch (want_exact)
SMALL_CASES = ["small-1", "small-64", "small-129", "small-600", "small-five1", "small-wide"]


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
@dataclass
class QueryRef:
    text: str
    norm: List[int]
    lq: int
    k: int
    d: int
    kind: int              # planes the scan compares: the largest multiplicity of a symbol (1 .. 4), 0 = count vectors
    ents: np.ndarray       # vocabulary positions of the reference pairs' entries, ascending
    exact_cls: int         # class number of the query's own count vector, -1 = no such class in the lexicon


def reference(m: Model, queries: List[str], kth, dth) -> List[Optional[QueryRef]]:
    """per query (None: nothing to encode) the reference pairs, from the count vectors alone"""
    out, cache = [], {}
    for q in queries:
        if q in cache:
            out.append(cache[q])
            continue
        s = T.normalize_to_alphabet(q, m.alphabet)
        lq = len(s)
        if lq == 0 or lq > 255:
            out.append(None)
            continue
        k = T.clamp_threshold(kth, lq, T.MAX_ANAGRAM_DISTANCE)
        d = T.clamp_threshold(dth, lq, T.MAX_EDIT_DISTANCE)
        cvq = m.count_vector(s)
        l1 = np.abs(m.cv - cvq).sum(axis=1)
        share = np.minimum(m.cv, cvq).sum(axis=1) > 0
        ok = (l1 <= k) & (np.abs(m.lens - lq) <= k) & share
        mult = int(cvq.max())
        kind = mult if (m.bit_planes and mult <= 4) else 0
        same = np.nonzero(l1 == 0)[0]
        r = QueryRef(q, s, lq, k, d, kind, np.nonzero(ok)[0], int(m.cls[same[0]]) if same.size else -1)
        cache[q] = r
        out.append(r)
    return out


@dataclass
class Expected:
    written: Counter       # (vocabulary position, flag bits >> 30) -> count (1: no pair twice)
    n_ref: int             # every reference pair: one DL invocation of the reference each
    n_lendrop: int         # counted, not written: |lc - lq| > d under drop_len
    n_bandrej: int         # counted, not written: the fused filter's bound rejected them
    n_fused: int           # pairs the fused filter tested
    n_counted: int         # what qpairs holds for the query (want_exact: the exact class alone when there is one)


def fuses(r: QueryRef, fuse: bool) -> bool:
    return bool(fuse) and r.kind != 0 and r.lq <= 16 and r.d <= 3


_BAND: Dict[tuple, bool] = {}


def band_rejects(m: Model, r: QueryRef, e: int) -> bool:
    key = (m.name, r.text, e, r.d)
    v = _BAND.get(key)
    if v is None:
        v = _BAND[key] = SC.band_bound_rejects(r.norm, m.norm[e], r.d)
    return v


def expected(m: Model, r: QueryRef, drop_len: bool, fuse: bool, want_exact: bool) -> Expected:
    f = fuses(r, fuse)
    w = Counter()
    n_len = n_band = n_fused = 0
    for e in r.ents.tolist():
        lc = int(m.lens[e])
        if drop_len and abs(lc - r.lq) > r.d:
            n_len += 1
            continue
        flags = 0
        if f:
            n_fused += 1
            if lc <= 16:
                if band_rejects(m, r, e):
                    n_band += 1
                    continue
                flags |= 1
        if want_exact and int(m.cls[e]) == r.exact_cls:
            flags |= 2
        w[(e, flags)] += 1
    n_counted = len(r.ents)
    if want_exact and r.exact_cls >= 0:
        n_counted = int((m.cls[r.ents] == r.exact_cls).sum())
    return Expected(w, len(r.ents), n_len, n_band, n_fused, n_counted)


# ---- what the tiles of a launch say (the GPU test asserts the tile-side classes from these) -----------------------------------------------
def launch_regions(ntiles: int, nadj: int, nbits: int, nsad: int, small: bool) -> np.ndarray:
    """region of every tile: its index within its launch % 64 (the small form: one launch over every slot)"""
    if small:
        return np.arange(ntiles) % REGIONS
    assert nadj + nbits + nsad == ntiles
    return np.concatenate([np.arange(nadj), np.arange(nbits), np.arange(nsad)]).astype(np.int64) % REGIONS


def adj_rows(k: int, cum) -> Tuple[int, int]:
    """rows [rbeg, rend) of a list a tile with anagram distance k streams: sections lq - k .. lq + k of the seven (cum = their cumulative rows)"""
    c = [int(x) for x in cum]
    return (0 if k >= 3 else c[2 - k]), c[3 + min(k, 3)]
