"""Hand-made candidate rows for k_rank (kernels_rank.hpp) by itself: the batches tests/test_gpu_rank_rows.py sends through
anx_debug_rank_rows, their reference (the tail of the twin's score_and_rank, oracle/twin.py rank_tail) and a census of the kernel's
branches each query takes, derived from the inputs alone (tests/test_rank_cases_cpu.py asserts that the fixed seeds populate them all).

A batch holds its rows in the REFERENCE's enumeration order -- per query sorted by (entry order, expansion position), which the stable
sort preserves among ties -- and a permutation `phys`: the device gets row phys[j] at physical index j (the
physical order inside a query is free)."""
import itertools
import zlib
from dataclasses import dataclass

import numpy as np

from oracle import twin as T

MAX_MATCHES = (0, 1, 2, 10, 15, 16, 17, 31, 32, 63, 64, 200)
CUTOFFS = (0.0, 0.5, 1.0, 1.5, 2.0, 1e9)
FREQ_WEIGHTS = (0.0, 0.5, 1.0, -0.25)
LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 1000)
SEG_CAPS = (2, 16, 32)
SMALL_NQ = (1, 3, 4, 5, 15, 16, 17)
LONG_LISTS = (65535, 65536, 65537, 70000)
NONE = 0xFFFFFFFF
U32MAX = 0xFFFFFFFF
RANK_LCAP = 128  # kernels_rank.hpp
# every quadruple of consecutive queries is one wave's work: the compositions the kernel distinguishes
FIXED_QUADS = ((3, 16, 1, 9), (5, 17, 16, 2), (16, 17, 33, 0), (32, 32, 32, 129), (17, 0, 0, 0), (17, 32, 25, 4), (20, 31, 18, 70),
               (5, 20, 70, 9), (0, 0, 0, 0), (64, 65, 63, 15), (127, 128, 33, 1), (12, 40, 7, 22))


@dataclass(frozen=True)
class Params:
    max_matches: int
    cutoff: float
    freq_weight: float
    have_freq: int
    any_variants: int

    @property
    def simple(self):  # launch_rank's choice of k_rank<true>
        return not self.any_variants and self.freq_weight == 0.0


@dataclass
class Batch:
    params: Params
    counts: np.ndarray    # u32 [nq]
    maxfreq: np.ndarray   # u32 [nq]
    qexpand: np.ndarray   # u32 [nq]
    score: np.ndarray     # f64 [rows], reference order
    order: np.ndarray     # u32
    position: np.ndarray  # u32
    vocab: np.ndarray     # u32
    freq: np.ndarray      # u32
    via: np.ndarray       # u32, NONE = none
    phys: np.ndarray      # i64 [rows]: the device's row j is reference row phys[j]

    @property
    def soff(self):
        s = np.zeros(self.counts.size + 1, dtype=np.int64)
        np.cumsum(self.counts, out=s[1:])
        return s


# ---- keys and ranking as the kernel's contract states them (used to PLACE rows and for the census, never as the reference) -----------
def _keys(P, maxfreq, score, freq):
    """(sort key, result score, normalised frequency) per row: src/types.rs:335-341, src/lib.rs:1521-1525 with the kernel's max_freq."""
    fw = float(np.float32(P.freq_weight))
    max_freq = float(maxfreq) if P.have_freq else (1.0 if maxfreq else 0.0)
    fs = freq.astype(np.float64)
    if max_freq > 0.0:
        fs = fs / max_freq
    ws = score if fw == 0.0 else (score + (fw * fs)) / (1.0 + fw)
    return (ws if fw > 0.0 else score), ws, fs


def _ranking(P, key, freq, order, position):
    """rank_cmp as a total order (src/types.rs:344-365; the last keys are the enumeration order)."""
    if P.freq_weight > 0.0:
        return np.lexsort((position, order, -key))
    return np.lexsort((position, order, -freq.astype(np.int64), -key))


# ---- populations ---------------------------------------------------------------------------------------------------------------------
SCORE_POPS = ("lattice", "equal", "distinct", "zeros", "best_repeated", "cutoff_edge", "crop_edge", "crop_edge_distinct")
FREQ_POPS = ("ones", "equal", "small", "withmax", "big", "zero")
VOCAB_POPS = ("unique", "pool", "pairs", "runs")


def _lattice(rng, n):
    L = int(rng.integers(1, 17))
    return rng.integers(0, L + 1, n).astype(np.float64) / L


def _scores(rng, n, P, pop):
    if pop == "lattice":
        return _lattice(rng, n)
    if pop == "equal":
        L = int(rng.integers(1, 17))
        return np.full(n, float(rng.integers(0, L + 1)) / L)
    if pop == "distinct":
        return (rng.permutation(n) + 1.0) / (n + 1.0)
    if pop == "zeros":
        L = int(rng.integers(1, 17))
        return rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0 / L, float(L - 1) / L]), n)
    if pop == "best_repeated":
        s = _lattice(rng, n)
        if n:
            s[rng.random(n) < 0.3] = s.max()
        return s
    if pop == "cutoff_edge" and 1.0 <= P.cutoff:
        L = int(rng.integers(1, 17))
        b = float(rng.integers(1, L + 1)) / L
        e = b / P.cutoff  # the kernel's and the twin's expression
        vals = np.array([b, e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf), float(rng.integers(0, L + 1)) / L * b])
        s = rng.choice(vals, n, p=[0.2, 0.2, 0.25, 0.25, 0.1])
        if n:
            s[int(rng.integers(0, n))] = b
        return s
    # rows equal to the row at index max_matches, before and after index max_matches - 1
    s = np.sort((rng.permutation(n) + 1.0) / (n + 1.0) if pop == "crop_edge_distinct" else _lattice(rng, n))[::-1].copy()
    mm = P.max_matches
    if 0 < mm < n:
        lo, hi = max(0, mm - int(rng.integers(1, 4))), min(n, mm + 1 + int(rng.integers(0, 3)))
        if rng.random() < 0.5:
            lo = mm  # ... or only behind it: then the crop is clean (cropped < last) where the values are distinct
        s[lo:hi] = s[mm]
    return rng.permutation(s)


def _freqs(rng, n, P, pop):
    """(freq[n], maxfreq)"""
    if not P.have_freq:  # the kernel's contract: all 1, maxfreq only says whether there was any candidate
        return np.ones(n, dtype=np.uint32), int(rng.choice([1, 1, 1, 0, 77])) if n else int(rng.choice([0, 5]))
    if pop == "zero" or n == 0:
        return np.zeros(n, dtype=np.uint32), 0 if pop == "zero" else int(rng.choice([0, 3, U32MAX]))
    if pop == "ones":
        f = np.ones(n, dtype=np.uint64)
    elif pop == "equal":
        f = np.full(n, int(rng.choice([2, 1000, U32MAX])), dtype=np.uint64)
    elif pop == "small":
        f = rng.integers(1, 5, n).astype(np.uint64)
    elif pop == "withmax":
        f = rng.integers(1, 1000, n).astype(np.uint64)
        f[rng.random(n) < 0.2] = f.max()
    else:
        f = rng.choice(np.array([1, U32MAX, 1 << 31, 12345, U32MAX - 1], dtype=np.uint64), n)
    mx = int(f.max())
    if rng.random() < 0.35:  # rows below the score threshold raise max_freq in a real run
        mx = min(U32MAX, int(rng.choice([mx + 1, mx * 3, U32MAX])))
    return f.astype(np.uint32), mx


def _orders(rng, n, expanded_shape):
    """(order[n], position[n]) with distinct (order, position): entry orders up to 2^32 - 1; with expanded_shape several positions per entry."""
    if expanded_shape:
        ends = np.minimum(np.cumsum(rng.integers(1, 4, n)), n)
        ends = ends[:int(np.searchsorted(ends, n)) + 1] if n else ends
        sizes = np.diff(np.concatenate([[0], ends]))
    else:
        sizes = np.ones(n, dtype=np.int64)
    m = len(sizes)
    mode = int(rng.integers(0, 3))
    if mode == 0:
        o = rng.permutation(4 * m + 4)[:m].astype(np.uint64)
    elif mode == 1:
        o = U32MAX - rng.permutation(4 * m + 4)[:m].astype(np.uint64)
    else:
        o = np.unique(np.concatenate([rng.integers(0, 1 << 32, 2 * m + 8, dtype=np.uint64), np.array([0, U32MAX], dtype=np.uint64)]))
        o = rng.permutation(o)[:m]
    order = np.repeat(o, sizes).astype(np.uint32)
    if expanded_shape:
        base = rng.integers(0, (1 << 20) - 3, m) * (rng.random(m) < 0.2)  # positions start at 0 mostly, near 2^20 sometimes
        starts = np.cumsum(sizes) - sizes
        position = (np.repeat(base, sizes) + np.arange(n) - np.repeat(starts, sizes)).astype(np.uint32)
    else:
        position = np.zeros(n, dtype=np.uint32)
    return order, position


def _vocabs(rng, n, P, pop, rank):
    """vocab[n]; `rank`: the rows' indices in ranked order -- 'pairs' and 'runs' place equal ids in consecutive / non-consecutive ranks"""
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    ids = rng.permutation(np.unique(rng.integers(0, 1 << 31, 2 * n + 4, dtype=np.uint64)))
    if pop == "unique":
        return ids[:n].astype(np.uint32)
    if pop == "pool":
        return rng.choice(ids[:max(1, n // 3)], n).astype(np.uint32)
    v = np.zeros(n, dtype=np.uint32)
    if pop == "pairs":  # a a b b c c ..: every second rank is a duplicate, also the one behind index max_matches - 1
        off = int(rng.integers(0, 2))
        v[rank] = ids[(np.arange(n) + off) // 2].astype(np.uint32)
        return v
    pool, seq, prev = ids[:max(2, n // 4)], [], None  # runs of 1..3 equal ids; an id may come back later (and must then stay)
    while len(seq) < n:
        x = int(rng.choice(pool))
        if x == prev:
            continue
        seq += [x] * int(rng.integers(1, 4))
        prev = x
    v[rank] = np.array(seq[:n], dtype=np.uint32)
    return v


def _query(rng, n, P, pops=None):
    spop, fpop, vpop = pops or (str(rng.choice(SCORE_POPS)), str(rng.choice(FREQ_POPS)), str(rng.choice(VOCAB_POPS)))
    qex = (int(rng.choice([1, 7, 0x80000000])) if rng.random() < 0.5 else 0) if P.any_variants else int(rng.integers(0, 2))
    score = _scores(rng, n, P, spop)
    freq, maxfreq = _freqs(rng, n, P, fpop)
    order, position = _orders(rng, n, bool(P.any_variants))
    idx = np.lexsort((position, order))  # reference order
    order, position = order[idx], position[idx]
    key, _, _ = _keys(P, maxfreq, score, freq)
    vocab = _vocabs(rng, n, P, vpop, _ranking(P, key, freq, order, position))
    if P.any_variants:
        via = np.where(rng.random(n) < 0.5, NONE, rng.integers(0, 1 << 31, n)).astype(np.uint32)
    else:
        via = np.full(n, NONE, dtype=np.uint32)
    return dict(n=n, maxfreq=maxfreq, qexpand=qex, score=score, order=order, position=position, vocab=vocab, freq=freq, via=via,
                phys=rng.permutation(n))


def _assemble(P, queries):
    soff = np.cumsum([0] + [q["n"] for q in queries])
    cat = lambda k, dt: np.concatenate([q[k] for q in queries]).astype(dt) if queries else np.zeros(0, dtype=dt)
    return Batch(P, np.array([q["n"] for q in queries], dtype=np.uint32), np.array([q["maxfreq"] for q in queries], dtype=np.uint32),
                 np.array([q["qexpand"] for q in queries], dtype=np.uint32), cat("score", np.float64), cat("order", np.uint32),
                 cat("position", np.uint32), cat("vocab", np.uint32), cat("freq", np.uint32), cat("via", np.uint32),
                 np.concatenate([q["phys"] + s for q, s in zip(queries, soff)]).astype(np.int64) if queries else np.zeros(0, dtype=np.int64))


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


# ---- the batches ---------------------------------------------------------------------------------------------------------------------
def main_params():
    return [Params(mm, c, fw, hf, av) for hf, av, fw, mm, c in itertools.product((0, 1), (0, 1), FREQ_WEIGHTS, MAX_MATCHES, CUTOFFS)]


def main_groups():
    """the crossing in 16 groups of 72 parameter sets: (have_freq, any_variants, freq_weight) -> [Params]"""
    g = {}
    for P in main_params():
        g.setdefault((P.have_freq, P.any_variants, P.freq_weight), []).append(P)
    return g


def main_batch(P):
    """every fixed quadruple, every list length, 40 or 160 random lists; nq mod 16 varies (the last wave and block partly empty)"""
    k = MAX_MATCHES.index(P.max_matches) * len(CUTOFFS) + CUTOFFS.index(P.cutoff)
    rng = np.random.default_rng(_seed("main", P))
    counts = [n for quad in FIXED_QUADS for n in quad] + [2, 15, 31, 255]
    if k % 4 == 0:
        counts.append(1000)
    for _ in range(160 if k % 3 == 0 else 40):  # every third batch has a few hundred queries
        u = rng.random()
        counts.append(int(rng.integers(0, 17)) if u < 0.6 else int(rng.integers(17, 33)) if u < 0.8 else int(rng.integers(33, 141)))
    counts = counts[:len(counts) - k % 5]
    return _assemble(P, [_query(rng, n, P) for n in counts])


def small_nq_batches():
    """nq of 1, 3, 4, 5, 15, 16, 17: one partly filled wave / block"""
    out = []
    ps = [Params(10, 2.0, 0.0, 1, 0), Params(2, 1.5, 0.5, 1, 1), Params(0, 0.0, 0.0, 0, 1), Params(16, 1.0, -0.25, 0, 0)]
    for i, nq in enumerate(SMALL_NQ):
        for j, P in enumerate(ps):
            rng = np.random.default_rng(_seed("small", nq, j))
            pool = [17, 3, 40, 16, 0, 32, 9, 130, 1, 20, 64, 5, 33, 12, 2, 70, 25]
            out.append(_assemble(P, [_query(rng, pool[(q + i + j) % len(pool)], P) for q in range(nq)]))
    return out


def equal2000_batches():
    """2 000 equal rows at max_matches 10: quickselect keeps them all, kept > RANK_LCAP, rank_query_all runs (once per kernel instance)"""
    out = []
    for av in (0, 1):
        P = Params(10, 0.0, 0.0, 1, av)
        rng = np.random.default_rng(_seed("equal2000", av))
        qs = [_query(rng, n, P) for n in (5, 2000, 20, 40)]
        qs[1] = _query(rng, 2000, P, ("equal", "equal", "unique"))
        qs[1]["qexpand"] = 0
        out.append(_assemble(P, qs))
    return out


def long_batches():
    """lists of 65 535 .. 70 000 rows with all-distinct keys under quickselect (max_matches 10, freq_weight 0); the rows that come out lie
    at the highest physical indices -- beyond 65 535 where the list has such indices"""
    out = []
    for cutoff, av in itertools.product((0.0, 2.0), (0, 1)):
        P = Params(10, cutoff, 0.0, 1, av)
        rng = np.random.default_rng(_seed("long", cutoff))
        qs = []
        for n in LONG_LISTS:
            q = _query(rng, n, P, ("distinct", "small", "unique"))
            q["qexpand"] = 0
            if n == 65537:  # a steep head: the best row alone above best / 2, so that the cutoff cuts right behind it (still all distinct)
                q["score"] *= 0.4
                q["score"][np.argmax(q["score"])] = 1.0
            top = np.argsort(-q["score"])[:24][::-1]   # reference rows ranked first ...
            rest = np.setdiff1d(np.arange(n), top)
            q["phys"] = np.concatenate([rng.permutation(rest), top])  # ... at the last physical indices, the best one last
            qs.append(q)
        qs.insert(1, _query(rng, 9, P))
        out.append(_assemble(P, qs))
    return out


def segment_params():
    return [Params(mm, c, fw, hf, 0) for hf, fw, mm, c in itertools.product((0, 1), FREQ_WEIGHTS, (0, 10, 16), (0.0, 2.0))]


def all_batches():
    """(name, batch) of every batch the GPU test ranks"""
    for P in main_params():
        yield "main", main_batch(P)
    for b in small_nq_batches():
        yield "small_nq", b
    for b in equal2000_batches():
        yield "equal2000", b
    for b in long_batches():
        yield "long", b


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def reference(b):
    """rank_tail per query -> (count[nq], vocab, via, dist_score, freq_score) with the ranked rows of all queries back to back"""
    P, soff = b.params, b.soff
    cnt, vo, vi, ds, fs = [], [], [], [], []
    for q in range(b.counts.size):
        a, e = int(soff[q]), int(soff[q + 1])
        rows = [T.VariantResult(int(v), float(s), float(f) if P.have_freq else 1.0, None if w == NONE else int(w))
                for v, s, f, w in zip(b.vocab[a:e].tolist(), b.score[a:e].tolist(), b.freq[a:e].tolist(), b.via[a:e].tolist())]
        mf = float(b.maxfreq[q]) if P.have_freq else (1.0 if b.maxfreq[q] else 0.0)
        res = T.rank_tail(rows, mf, bool(P.any_variants and b.qexpand[q] != 0), P.max_matches, P.cutoff, P.freq_weight)
        cnt.append(len(res))
        for r in res:
            vo.append(r.vocab_id)
            vi.append(NONE if (r.via is None or not P.any_variants) else r.via)
            ds.append(r.dist_score)
            fs.append(r.freq_score)
    return (np.array(cnt, dtype=np.uint32), np.array(vo, dtype=np.uint32), np.array(vi, dtype=np.uint32), np.array(ds, dtype=np.float64),
            np.array(fs, dtype=np.float64))


# ---- the census: which of k_rank's branches a query takes (the conditions of kernels_rank.hpp, from the inputs alone) -------------------
CROP_OUTCOMES = ("not_cropped", "cropped_lt_last", "early", "late", "neither")


def census_query(P, n, maxfreq, qex, score, freq, order, position, vocab):
    width = 16 if n <= 16 else 32 if n <= 32 else 64
    if n == 0:
        return dict(width=width, empty=True)
    lcap = RANK_LCAP if width == 64 else width
    fw = float(np.float32(P.freq_weight))
    sort_weighted, score_weighted = fw > 0.0, fw != 0.0
    expanded = bool(P.any_variants and qex != 0)
    key, ws, _ = _keys(P, maxfreq, score, freq)
    best = key.max()
    prune = P.cutoff >= 1.0 and not expanded and not score_weighted and n <= 0xFFFF
    pa = np.ones(n, dtype=bool)
    if prune:
        pa = ~((key <= best / P.cutoff) & (key < best))
    full = score_weighted or P.max_matches == 0 or expanded
    quickselect = width == 64 and n > 32 and not full
    tau = -1.0
    if quickselect and int(pa.sum()) >= P.max_matches + 1:
        tau = np.sort(key[pa])[::-1][P.max_matches]
    keep = pa & (key >= tau)
    kept = int(keep.sum())
    lds = kept <= lcap
    sel = np.nonzero(keep)[0] if lds else np.arange(n)
    nn = sel.size
    M = nn if full else min(nn, P.max_matches + 1)
    parallel = not expanded and M <= width
    if lds:
        compare = "packed" if (not sort_weighted and not P.any_variants) else "weighted" if sort_weighted else "plain"
    else:
        compare = "weighted" if sort_weighted else "plain"
    r = sel[_ranking(P, key[sel], freq[sel], order[sel], position[sel])]
    dups = False
    avail = M
    if expanded:
        v = vocab[r]
        first = np.concatenate([[True], v[1:] != v[:-1]])
        dups = not first.all()
        r = r[first]
        avail = r.size
    dist, sc = score[r], ws[r]
    length, mm = r.size, P.max_matches
    crop = "not_cropped"
    if mm > 0 and length > mm:
        last, cropped = sc[mm - 1], sc[mm]
        if cropped < last:
            crop, length = "cropped_lt_last", mm
        else:
            early = late = 0
            for i in range(avail):
                if dist[i] == cropped and early == 0:
                    early = i
                if dist[i] < cropped:
                    late = i
                    break
            if early > 0:
                crop, length = "early", early + 1
            elif late > 0:
                crop, length = "late", late + 1
            else:
                crop = "neither"
    cut = False
    if P.cutoff >= 1.0:
        hit = np.nonzero(sc[1:length] <= sc[0] / P.cutoff)[0]
        cut = hit.size > 0
    return dict(width=width, empty=False, prune=bool(prune), pruned_rows=bool(prune and not pa.all()), quickselect=bool(quickselect),
                tau=bool(tau >= 0.0), kept=kept, lds=bool(lds), compare=compare, parallel_tail=bool(parallel), expanded=expanded,
                dups=bool(dups), crop=crop, cut=bool(cut))


def census(b):
    soff = b.soff
    out = []
    for q in range(b.counts.size):
        a, e = int(soff[q]), int(soff[q + 1])
        out.append(census_query(b.params, e - a, int(b.maxfreq[q]), int(b.qexpand[q]), b.score[a:e], b.freq[a:e], b.order[a:e],
                                b.position[a:e], b.vocab[a:e]))
    return out
