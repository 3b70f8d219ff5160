#!/usr/bin/env python3
"""Throughput of anx_score_pairs (host to host) on eng.aspell, against the C oracle's per-pair functions on the host.

    score_pairs_bench.py [--pairs 1000000] [--long 10000] [--reps 5] [--oracle-procs 16] [--json OUT]

Two sets of pairs:
  words : --pairs pairs (synth query, nearest lexicon word: the first ranked row of find_variants, max_matches 1; a query without a
          row is paired with itself) -- almost all of them take the short tier (both sides <= 16 bytes, k_pairs_short);
  long  : --long pairs of 100-255 symbols (random words joined with spaces, the other side the same text after 1-12 edits and
          transpositions) -- the long tier (k_pairs_long).
Per set: best and median of --reps calls of anx_score_pairs_packed, buffer of strings to records in host memory (the packing of the
Python lists is outside the timed region), pairs/s from the median; the summed time of each tier's kernel for one call (the library's
kernel timer, anx_debug_kernel_time); and the rate of orc_damerau_levenshtein + orc_lcs + orc_prefix + orc_suffix over the same
pairs (codes normalised beforehand, outside the timed region) on --oracle-procs host processes, each making its ctypes calls one pair
at a time -- the per-call overhead of ctypes is part of that figure.  The worker processes are started before this process opens the
GPU and never open it themselves."""
import argparse
import json
import multiprocessing as mp
import os
import random
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def oracle_worker(job):
    """(list of (codes a, codes b)) -> seconds spent in the four oracle functions"""
    from oracle import cwrap as O
    lib = O.lib()
    t0 = time.perf_counter()
    acc = 0
    for a, b in job:
        acc += lib.orc_damerau_levenshtein(a, len(a), b, len(b), 255) + lib.orc_lcs(a, len(a), b, len(b)) + \
            lib.orc_prefix(a, len(a), b, len(b)) + lib.orc_suffix(a, len(a), b, len(b))
    return time.perf_counter() - t0, acc


def edits(rng, s, n, letters="abcdefghijklmnopqrstuvwxyz ", max_len=255):
    cs = list(s)
    for _ in range(n):
        op = rng.randrange(5)
        if op == 0 and len(cs) > 1:
            del cs[rng.randrange(len(cs))]
        elif op == 1 and len(cs) < max_len:
            cs.insert(rng.randrange(len(cs) + 1), rng.choice(letters))
        elif op == 2:
            cs[rng.randrange(len(cs))] = rng.choice(letters)
        elif len(cs) > 1:
            p = rng.randrange(len(cs) - 1)
            cs[p], cs[p + 1] = cs[p + 1], cs[p]
    return "".join(cs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--long", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-procs", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pool = mp.get_context("spawn").Pool(a.oracle_procs)  # fresh processes, before the GPU is opened here
    pool.map(oracle_worker, [[(b"a", b"b")]] * a.oracle_procs)  # (started and the oracle library loaded)

    import analiticcl_amd as A
    from analiticcl_amd import _lib as L
    from analiticcl_amd import synth
    from analiticcl_amd.model import _pack
    from oracle import cwrap as O
    with tempfile.TemporaryDirectory() as tmp:
        data = synth.materialize_golden(os.path.join(tmp, "data"))
        words = synth.load_lexicon_words(data["eng"])
        g = A.VariantModel(data["alphabet"], A.Weights(), device=0)
        g.read_lexicon(data["eng"])
        g.build()
        o = O.OracleModel(alphabet_path=data["alphabet"])
        rng = random.Random(20241018)
        qs = synth.make_queries(words, a.pairs, max_len=16, seed=8)
        near = g.find_variants_ids(qs, A.SearchParameters(max_anagram_distance=3, max_edit_distance=3, max_matches=1, score_threshold=0.0))
        sets = {"words": (qs, [g.vocab_text(r[0][0]) if r else q for q, r in zip(qs, near)])}
        la, lb = [], []
        while len(la) < a.long:
            t = " ".join(rng.choice(words) for _ in range(rng.randint(14, 40)))[:rng.randint(100, 255)]
            la.append(t)
            lb.append(edits(rng, t, rng.randint(1, 12)))
        sets["long"] = (la, lb)
        lib = L.lib()
        res = {}
        for name, (sa, sb) in sets.items():
            n = len(sa)
            ba, bb = _pack(sa), _pack(sb)
            out = (L.PairScore * n)()
            times = []
            for rep in range(a.reps + 1):  # (the first call warms the pools)
                if rep == a.reps:
                    L.kernel_timer(True)
                t0 = time.perf_counter()
                L.check(lib.anx_score_pairs_packed(g.h, ba, len(ba), bb, len(bb), n, out))
                times.append(time.perf_counter() - t0)
            k_short, k_long = L.kernel_time("k_pairs_short"), L.kernel_time("k_pairs_long")
            L.kernel_timer(False)
            times = times[1:]
            nshort = sum(1 for x, y in zip(sa, sb) if len(x.encode()) <= 16 and len(y.encode()) <= 16)
            codes = [(bytes(o.normalize(x)), bytes(o.normalize(y))) for x, y in zip(sa, sb)]
            jobs = [codes[i::a.oracle_procs] for i in range(a.oracle_procs)]
            t0 = time.perf_counter()
            pool.map(oracle_worker, jobs)
            t_oracle = time.perf_counter() - t0
            res[name] = {"pairs": n, "short_tier_pairs": nshort, "best_ms": min(times) * 1e3, "median_ms": statistics.median(times) * 1e3,
                         "pairs_per_s": n / statistics.median(times), "k_pairs_short_ms": k_short[0], "k_pairs_long_ms": k_long[0],
                         "oracle_procs": a.oracle_procs, "oracle_pairs_per_s": n / t_oracle}
            r = res[name]
            print(f"{name:6s} {n:8d} pairs ({nshort} short tier): best {r['best_ms']:.2f} ms, median {r['median_ms']:.2f} ms = {r['pairs_per_s'] / 1e6:.2f} M pairs/s; "
                  f"k_pairs_short {k_short[0]:.3f} ms ({k_short[1]} launches), k_pairs_long {k_long[0]:.3f} ms ({k_long[1]} launches); "
                  f"oracle on {a.oracle_procs} processes {r['oracle_pairs_per_s'] / 1e6:.3f} M pairs/s", flush=True)
    pool.close()
    pool.join()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
