#!/usr/bin/env python3
"""anx_batch_fetch_measures against the same answer composed from the entry points that existed before it, on eng.aspell.

    explain_bench.py [--queries 1000000] [--reps 10] [--procs 2] [--json OUT]

One resident batch of synthetic queries (the benchmark's law: synth.make_queries, max_len 16) under k = 3, d = 2, n = 10, run once.
  (a) Batch.fetch_measures on the resident batch: 16 bytes per ranked row and the offsets come down, nothing goes up.
  (b) the composition, in the same build: fetch_compact(with_via=True) (every row comes down), the text of every row's input and of
      its vocabulary item (the item texts from a host list built outside the timed region), score_pairs_arrays over every row (both
      strings of every row go up, 24 bytes per row come down).  (b) has no anagram distance at all, so it does LESS than (a); it is
      charged nothing for that.
Every measurement runs in a fresh process, (a) and (b) alternating, --procs processes each, --reps timed calls after one warm-up call.
Reported: median and best per side, the bytes each side downloads and uploads, and for (a) k_row_measures / k_row_measures_long from
the library's kernel timer (one extra call).  The verdict: (a)'s median lies below (b)'s median minus (b)'s own best-to-median
spread; nothing is compared against the code under test."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def child(side, n, reps):
    import numpy as np

    import analiticcl_amd as A
    from analiticcl_amd import _lib as L
    from analiticcl_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        data = synth.materialize_golden(os.path.join(tmp, "data"))
        words = synth.load_lexicon_words(data["eng"])
        g = A.VariantModel(data["alphabet"], A.Weights(), device=0)
        g.read_lexicon(data["eng"])
        g.build()
        qs = synth.make_queries(words, n, max_len=16, seed=synth.SEED)
        P = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
        b = g.encode_batch(qs, P)
        b.run()
        res = {"side": side, "queries": n}
        if side == "a":
            def call():
                off, m = b.fetch_measures()
                res["rows"] = int(off[-1])
                return m.nbytes + off.nbytes, 0
        else:
            texts = [g.vocab_text(v) for v in range(g.vocab_size())]   # the host list, built once

            def call():
                off, rec, _via = b.fetch_compact(with_via=True)
                cnt = np.diff(off.astype(np.int64))
                left = [qs[i] for i in np.repeat(np.arange(n), cnt).tolist()]
                right = [texts[v] for v in rec["vocab_id"].tolist()]
                cols = g.score_pairs_arrays(left, right)
                rows = len(rec)
                res["rows"] = rows
                up = sum(len(x.encode("utf-8")) + 1 for x in left) + sum(len(x.encode("utf-8")) + 1 for x in right) + 4 * (2 * rows + 1)
                return rec.nbytes + off.nbytes + 4 * rows + 24 * rows + 0 * int(cols["ld"][0]), up
        call()   # warms the pools (and builds the vocabulary table of the replica)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            down, up = call()
            times.append(time.perf_counter() - t0)
        res["bytes_down"], res["bytes_up"] = int(down), int(up)
        res["times_ms"] = [t * 1e3 for t in times]
        if side == "a":
            L.kernel_timer(True)
            call()
            res["kernels_ms"] = {k: L.kernel_time(k)[0] for k in ("k_row_measures", "k_row_measures_long")}
            L.kernel_timer(False)
        b.free()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--queries", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), a.reps)
        return 0
    runs = {"a": [], "b": []}
    for _ in range(a.procs):
        for side in ("a", "b"):   # alternating, every one a fresh process
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", side, str(a.queries)], capture_output=True,
                               text=True, timeout=900)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                return 1   # nothing more is started after a failed measurement
            runs[side].append(json.loads(line[-1][7:]))
    r = {"queries": a.queries, "rows": runs["a"][0]["rows"]}
    for side in ("a", "b"):
        t = [x for run in runs[side] for x in run["times_ms"]]
        r[side] = {"median_ms": statistics.median(t), "best_ms": min(t), "bytes_down": runs[side][0]["bytes_down"], "bytes_up": runs[side][0]["bytes_up"]}
    r["kernels_ms"] = runs["a"][0]["kernels_ms"]
    spread = r["b"]["median_ms"] - r["b"]["best_ms"]
    r["verdict"] = "ok" if r["a"]["median_ms"] < r["b"]["median_ms"] - spread else "DEFECT: (a) is not below (b)'s median minus (b)'s own spread"
    print(f"{a.queries} queries, {r['rows']} rows: " + "; ".join(
        f"({s}) median {r[s]['median_ms']:.2f} ms (best {r[s]['best_ms']:.2f}), {r[s]['bytes_down'] / 1e6:.2f} MB down, {r[s]['bytes_up'] / 1e6:.2f} MB up" for s in ("a", "b"))
          + "; " + r["verdict"])
    print("   kernels of one call of (a), ms: " + ", ".join(f"{k} {v:.3f}" for k, v in r["kernels_ms"].items()), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
