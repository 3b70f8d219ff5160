#!/usr/bin/env python3
"""anx_mine_confusables against the same table made with what existed before it, on eng.aspell.

    mine_bench.py [--pairs 1000000] [--reps 5] [--procs 2] [--workers 16] [--parent-tree DIR] [--json OUT]

Pairs: (edited query, source word) as tools/evaluate_bench.py makes them (one to three random edits of lexicon words, seeded), context 0,
no anchors.
  (a) anx_mine_confusables_packed, table only: two blobs in host memory to the table in host memory (numpy arrays).  Once more with the site list, for
      the record.
  (b) the baseline: anx_edit_script per pair on --workers host processes, the sites cut out of the script strings and counted with a
      Python Counter per worker, the counters merged.  The workers are forked before the timed region with their share of the pairs and
      never open the device.
Every measurement runs in a fresh process, (a) and (b) alternating, --procs processes each, --reps timed calls after one warm-up call:
median and best of procs x reps calls per side.  Verdict: (a)'s median is below (b)'s median minus (b)'s own best-to-median spread.
Also reported for (a), from the library's kernel timer (one extra call): k_mine_script, the sort and the reduce; bytes up and down;
pairs scripted on the host.  The two tables are compared once, outside the timed region.
--parent-tree DIR: a checkout of the parent commit with its library built.  anx_score_pairs_packed on the same pairs then runs on this
build and on the parent's in turn (fresh processes), and this build's median is reported against the parent's own spread."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_chunks = []  # the baseline's pairs, one list per worker: set before the fork, so no call ships them


def _worker(k):
    from collections import Counter

    from analiticcl_amd.model import edit_script
    c = Counter()
    cut = re.compile(r"=\[[^\]]*\]")
    for a, b in _chunks[k]:
        for site in cut.split(edit_script(a, b)):
            if site:
                c[site] += 1
    return c


def child(side, n, reps, workers, tree):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import analiticcl_amd as A
    from analiticcl_amd import _lib as L
    from analiticcl_amd import synth
    from analiticcl_amd.model import _pack
    from eval_twin import edited_pairs
    res = {"side": side, "pairs": n}
    with tempfile.TemporaryDirectory() as tmp:
        data = synth.materialize_golden(os.path.join(tmp, "data"))
        words = synth.load_lexicon_words(data["eng"])
        pairs = edited_pairs(words, n, seed=7)
        qa, qb = [a for a, _ in pairs], [b for _, b in pairs]
        if side == "b":
            import multiprocessing as mp
            from collections import Counter
            per = (n + workers - 1) // workers
            _chunks[:] = [pairs[k:k + per] for k in range(0, n, per)]
            with mp.get_context("fork").Pool(workers) as pool:
                def call():
                    total = Counter()
                    for c in pool.map(_worker, range(len(_chunks)), chunksize=1):
                        total.update(c)
                    return total
                table = call()
                times = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    table = call()
                    times.append(time.perf_counter() - t0)
            res["table"] = sorted(table.items(), key=lambda kv: (-kv[1], kv[0].encode()))[:50]
            res["patterns"] = len(table)
        else:
            g = A.VariantModel(data["alphabet"], A.Weights(), device=0)
            g.read_lexicon(data["eng"])
            g.build()
            ba, bb = _pack(qa), _pack(qb)
            if side == "a":
                def call(sites=False):  # from the packed host buffers, as the baseline's workers start from lists they hold
                    return g.mine_confusables_arrays(ba, bb, sites=sites, packed="blobs", n=n)
                r = call()
                times = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    r = call()
                    times.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                call(True)
                res["with_sites_ms"] = (time.perf_counter() - t0) * 1e3
                s0 = A.VariantModel.mine_stats()
                L.kernel_timer(True)
                call()
                res["kernels_ms"] = {k: L.kernel_time(k)[0] for k in ("k_mine_script", "k_mine_sort", "k_mine_reduce")}
                L.kernel_timer(False)
                s1 = A.VariantModel.mine_stats()
                res["stats_one_call"] = {k: s1[k] - s0[k] for k in s1}
                off, text = r["text_off"].tolist(), r["text"]
                res["table"] = [(text[off[k]:off[k + 1]].decode(), int(r["count"][k])) for k in range(min(50, len(off) - 1))]
                res["patterns"] = len(off) - 1
            else:  # "s": anx_score_pairs_packed of whatever build `tree` holds
                import ctypes as C

                import numpy as np
                out = np.zeros(n, dtype=np.dtype(A.VariantModel.PAIR_DTYPE))
                optr = out.ctypes.data_as(C.POINTER(L.PairScore))

                def call():
                    L.check(L.lib().anx_score_pairs_packed(g.h, ba, len(ba), bb, len(bb), n, optr))
                call()
                times = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    call()
                    times.append(time.perf_counter() - t0)
        res["times_ms"] = [t * 1e3 for t in times]
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), a.reps, a.workers, a.child[2])
        return 0

    def measure(sides):  # sides: [(name, side, tree)], alternating, every one a fresh process
        runs = {name: [] for name, _s, _t in sides}
        for _ in range(a.procs):
            for name, side, tree in sides:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--workers", str(a.workers), "--child", side,
                                    str(a.pairs), tree], capture_output=True, text=True, timeout=1500)
                line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                    return None  # nothing more is started after a failed measurement
                runs[name].append(json.loads(line[-1][7:]))
        return runs

    def summary(rs):
        t = [x for r in rs for x in r["times_ms"]]
        return {"median_ms": statistics.median(t), "best_ms": min(t), "calls": len(t)}

    report = {"pairs": a.pairs}
    runs = measure([("a", "a", REPO), ("b", "b", REPO)])
    if runs is None:
        return 1
    ra, rb = summary(runs["a"]), summary(runs["b"])
    spread = rb["median_ms"] - rb["best_ms"]
    same = [tuple(x) for x in runs["a"][0]["table"]] == [tuple(x) for x in runs["b"][0]["table"]] and runs["a"][0]["patterns"] == runs["b"][0]["patterns"]
    verdict = "ok" if ra["median_ms"] < rb["median_ms"] - spread else "DEFECT: (a) is not below (b)'s median minus (b)'s own spread"
    if not same:
        verdict = "DEFECT: the two tables differ"
    report.update({"a": ra, "b": rb, "verdict": verdict, "with_sites_ms": runs["a"][0]["with_sites_ms"], "kernels_ms": runs["a"][0]["kernels_ms"],
                   "stats_one_call": runs["a"][0]["stats_one_call"], "patterns": runs["a"][0]["patterns"]})
    print(f"{a.pairs} pairs, {report['patterns']} patterns: (a) median {ra['median_ms']:.2f} ms (best {ra['best_ms']:.2f}); "
          f"(b) median {rb['median_ms']:.2f} ms (best {rb['best_ms']:.2f}) on {a.workers} processes; {verdict}")
    print(f"   (a) with the site list: {report['with_sites_ms']:.2f} ms; kernels of one call, ms: "
          + ", ".join(f"{k} {v:.3f}" for k, v in report["kernels_ms"].items()))
    print("   one call: " + json.dumps(report["stats_one_call"]), flush=True)
    if a.parent_tree:
        runs = measure([("this", "s", REPO), ("parent", "s", os.path.abspath(a.parent_tree))])
        if runs is None:
            return 1
        rt, rp = summary(runs["this"]), summary(runs["parent"])
        pspread = rp["median_ms"] - rp["best_ms"]
        sv = "ok" if rt["median_ms"] <= rp["median_ms"] + pspread else "DEFECT: anx_score_pairs_packed is slower than the parent's by more than the parent's own spread"
        report["score_pairs"] = {"this": rt, "parent": rp, "verdict": sv}
        print(f"   anx_score_pairs_packed: this build median {rt['median_ms']:.2f} ms (best {rt['best_ms']:.2f}); parent median {rp['median_ms']:.2f} ms "
              f"(best {rp['best_ms']:.2f}); {sv}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
