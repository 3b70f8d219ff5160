#!/usr/bin/env python3
"""anx_evaluate_sweep against the same answer from one anx_evaluate_gold call per parameter set, on eng.aspell.

    sweep_bench.py [--pairs 1000000] [--small 10000] [--reps 5] [--procs 2] [--json OUT]

Pairs: (edited query, source word) -- one to three random edits of lexicon words, seeded.  Eight parameter sets:
k in {2, 3} x d in {1, 2} x n in {3, 10}; the first is the baseline.
  (a) one anx_evaluate_sweep_packed call with out == NULL: two blobs in, 624 bytes per set out.
  (b) the same answer in the same build: eight anx_evaluate_gold_packed calls (32 bytes per pair and set out), each reduced with
      evaluate_summary (numpy).
Every measurement runs in a fresh process, (a) and (b) alternating, --procs processes each, --reps timed calls after one warm-up call;
the packing of the Python lists into blobs is outside the timed region for both.  Reported: median and best per side, the bytes each
side downloads, and from one extra call of (a): the k_sweep_* times of the library's kernel timer, the batch step of every set on its
own (encode_packed + run), and how many k_scan launches the call's batch runs made -- RunHints are keyed by the parameters, so a
batch that follows one of another set finds no hint; more launches than runs would mean batches ran twice.  (a)'s summaries are held
against (b)'s.  The verdict asks that (a)'s median lie below (b)'s median minus (b)'s own best-to-median spread; nothing is compared
against the code under test.  The same again for --small pairs."""
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
sys.path.insert(0, os.path.join(REPO, "tests"))

SETS = [(k, d, n) for k in (2, 3) for d in (1, 2) for n in (3, 10)]
SWEEP_KERNELS = ("k_sweep_lookup", "k_sweep_rows", "k_sweep_classify", "k_enc_strings_pairs", "k_pairs_short", "k_pairs_long")


def child(side, n, reps):
    import ctypes as C

    import numpy as np

    import analiticcl_amd as A
    from analiticcl_amd import _lib as L
    from analiticcl_amd import synth
    from analiticcl_amd.model import _pack
    from eval_twin import edited_pairs
    with tempfile.TemporaryDirectory() as tmp:
        data = synth.materialize_golden(os.path.join(tmp, "data"))
        words = synth.load_lexicon_words(data["eng"])
        g = A.VariantModel(data["alphabet"], A.Weights(), device=0)
        g.read_lexicon(data["eng"])
        g.build()
        pairs = edited_pairs(words, n, seed=7)
        ba, bg = _pack([a for a, _ in pairs]), _pack([b for _, b in pairs])
        Ps = [A.SearchParameters(max_anagram_distance=k, max_edit_distance=d, max_matches=m) for k, d, m in SETS]
        cps = [p._c() for p in Ps]
        sets = (L.Params * len(Ps))(*cps)
        sums = np.zeros(len(Ps), dtype=np.dtype(A.VariantModel.SUMMARY_DTYPE))
        out = np.zeros(n, dtype=np.dtype(A.VariantModel.GOLD_DTYPE))
        optr = out.ctypes.data_as(C.POINTER(L.GoldEval))
        res = {"side": side, "pairs": n}

        def per_set():
            got = []
            for cp in cps:
                L.check(L.lib().anx_evaluate_gold_packed(g.h, ba, len(ba), bg, len(bg), n, C.byref(cp), optr, None))
                got.append(A.VariantModel.evaluate_summary(out))
            return got

        if side == "a":
            def call():
                t0 = A.VariantModel.sweep_stats()["bytes_down"]
                L.check(L.lib().anx_evaluate_sweep_packed(g.h, ba, len(ba), bg, len(bg), n, sets, len(Ps), sums.ctypes.data_as(C.POINTER(L.GoldSummary)), None, None))
                return A.VariantModel.sweep_stats()["bytes_down"] - t0
        else:
            def call():
                per_set()
                return len(Ps) * 32 * n
        call()   # warms the pools (and builds the vocabulary table)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res["bytes_down"] = int(call())
            times.append(time.perf_counter() - t0)
        res["times_ms"] = [t * 1e3 for t in times]
        if side == "a":
            L.kernel_timer(True)
            runs0 = A.VariantModel.sweep_stats()["batch_runs"]
            call()
            res["kernels_ms"] = {k: L.kernel_time(k)[0] for k in SWEEP_KERNELS}
            res["batch_runs"] = A.VariantModel.sweep_stats()["batch_runs"] - runs0
            res["k_scan_launches"] = int(L.kernel_time("k_scan")[1])
            L.kernel_timer(False)
            step = []
            for p in Ps:   # the batch step of every set on its own, each after a batch of another set
                t0 = time.perf_counter()
                b = g.encode_packed(ba, n, p)
                b.run()
                step.append((time.perf_counter() - t0) * 1e3)
                b.free()
            res["batch_step_ms"] = step
            mine = [A.VariantModel.sweep_summary(s) for s in sums]
            ref = per_set()
            res["agrees"] = all(m["reasons"] == r["reasons"] and m["accuracy_at_1"] == r["accuracy_at_1"] and m["gold_known"] == r["gold_known"] and
                                abs(m["mrr"] - r["mrr"]) < 2.0 ** -32 + 1e-9 for m, r in zip(mine, ref))
            res["summary"] = [{"k,d,n": list(SETS[i]), "accuracy_at_1": m["accuracy_at_1"], "mrr": m["mrr"], "ranked": m["reasons"]["RANKED"],
                               "gained_at_1": m["gained_at_1"], "lost_at_1": m["lost_at_1"], "mean_list": m["n_results"] / n} for i, m in enumerate(mine)]
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--small", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), a.reps)
        return 0
    report = {}
    for n in (a.pairs, a.small):
        runs = {"a": [], "b": []}
        for _ in range(a.procs):
            for side in ("a", "b"):   # alternating, every one a fresh process
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", side, str(n)], capture_output=True, text=True, timeout=900)
                line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                    return 1   # nothing more is started after a failed measurement
                runs[side].append(json.loads(line[-1][7:]))
        r = {}
        for side in ("a", "b"):
            t = [x for run in runs[side] for x in run["times_ms"]]
            r[side] = {"median_ms": statistics.median(t), "best_ms": min(t), "bytes_down": runs[side][0]["bytes_down"]}
        for k in ("kernels_ms", "batch_runs", "k_scan_launches", "batch_step_ms", "agrees", "summary"):
            r[k] = runs["a"][0][k]
        spread = r["b"]["median_ms"] - r["b"]["best_ms"]
        r["verdict"] = "ok" if r["a"]["median_ms"] < r["b"]["median_ms"] - spread else "NO GAIN: (a) is not below (b)'s median minus (b)'s own spread"
        if not r["agrees"]:
            r["verdict"] = "DEFECT: (a)'s summaries differ from (b)'s"
        report[str(n)] = r
        print(f"{n} pairs, {len(SETS)} sets: (a) median {r['a']['median_ms']:.2f} ms (best {r['a']['best_ms']:.2f}), {r['a']['bytes_down']} bytes down; "
              f"(b) median {r['b']['median_ms']:.2f} ms (best {r['b']['best_ms']:.2f}), {r['b']['bytes_down'] / 1e6:.2f} MB down; {r['verdict']}")
        print("   kernels of one call of (a), ms: " + ", ".join(f"{k} {v:.3f}" for k, v in r["kernels_ms"].items()))
        print(f"   batch runs of that call: {r['batch_runs']}, k_scan launches: {r['k_scan_launches']}; the batch step per set, ms: " +
              ", ".join(f"{v:.2f}" for v in r["batch_step_ms"]))
        print("   summaries: " + json.dumps(r["summary"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
