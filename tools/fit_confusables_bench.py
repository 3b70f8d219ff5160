#!/usr/bin/env python3
"""anx_fit_confusable_weights against what a user does without it: the same greedy driven from Python over the confusable sweep.

    fit_confusables_bench.py [--pairs 1000000] [--small 10000] [--reps 5] [--procs 1] [--json OUT]

Pairs: (edited query, source word) -- one to three random edits of eng.aspell words, seeded.  Candidates: the 20 commonest
representable patterns mine_confusables finds on those pairs; grid (0.8, 0.9, 1.1, 1.25); k = 3, d = 2, n = 10; objective acc1,
min_gain 1, at most 10 rounds.
  (a) one anx_fit_confusable_weights_packed call: two blobs in, the base run, the masks and the late ranking once, then per round one
      launch of k_fit_trials and one download of the counters.
  (b) the same greedy from Python (tests/fit_twin.py) over anx_evaluate_sweep_confusables_packed: one call of up to 81 sets per
      round, each with its own upload, base run, mask pass and per-set ranking.
Every measurement runs in a fresh process, (a) and (b) alternating, --procs processes each, --reps timed calls after one warm-up
call; the packing of the Python lists into blobs is outside the timed region on both sides.  Reported: median and best per side, the
rounds accepted, the text bytes each side uploads and the bytes it downloads, the state's size, and from one extra call of (a) the
kernel times of k_fit_gold, k_fit_state and k_fit_trials (per round).  Both sides must return the same rounds and weights.  The
verdict asks that (a)'s median lie below (b)'s median minus (b)'s own best-to-median spread; nothing is compared against the code
under test.  The same again for --small pairs."""
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

CANDIDATES, GRID, MAX_ROUNDS, MIN_GAIN = 20, (0.8, 0.9, 1.1, 1.25), 10, 1
KERNELS = ("k_fit_gold", "k_fit_state", "k_fit_trials")


def child(side, n, reps):
    import ctypes as C

    import numpy as np

    import analiticcl_amd as A
    from analiticcl_amd import _lib as L
    from analiticcl_amd import synth
    from analiticcl_amd.model import _pack
    from eval_twin import edited_pairs
    import fit_twin as F
    with tempfile.TemporaryDirectory() as tmp:
        data = synth.materialize_golden(os.path.join(tmp, "data"))
        words = synth.load_lexicon_words(data["eng"])
        pairs = edited_pairs(words, n, seed=7)
        ba, bg = _pack([a for a, _ in pairs]), _pack([b for _, b in pairs])
        P = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
        plain = A.VariantModel(data["alphabet"], A.Weights(), device=0)
        plain.read_lexicon(data["eng"])
        plain.build()
        patterns = [r["pattern"] for r in plain.mine_confusables([a for a, _ in pairs], [b for _, b in pairs]) if r["representable"]][:CANDIDATES]
        J, G = len(patterns), len(GRID)
        pats = (C.c_char_p * J)(*[p.encode() for p in patterns])
        cp = P._c()
        dp = C.POINTER(C.c_double)
        res = {"side": side, "pairs": n, "patterns": patterns, "grid": list(GRID)}
        if side == "a":
            grid = (C.c_double * G)(*GRID)
            fp = L.FitParams(grid, G, 0, None, L.ANX_FIT_ACC1, MAX_ROUNDS, MIN_GAIN)
            weights, rounds, result = np.zeros(J), (L.FitRound * MAX_ROUNDS)(), L.FitResult()

            def call():
                t0 = A.VariantModel.fit_stats()
                L.check(L.lib().anx_fit_confusable_weights_packed(plain.h, ba, len(ba), bg, len(bg), n, pats, J, C.byref(cp), C.byref(fp), weights.ctypes.data_as(dp),
                                                                  rounds, None, C.byref(result)))
                t1 = A.VariantModel.fit_stats()
                d = {k: t1[k] - t0[k] for k in t0}
                return d["bytes_down"], 2 * len(ba) + len(bg), d   # the pair side once, the inputs once more for the one batch run

            def outcome():
                return ([[int(r.pattern), int(r.grid_index), float(r.weight).hex(), [int(r.counts.at1), int(r.counts.ranked), int(r.counts.rr_fixed)]]
                         for r in rounds[:result.n_rounds]], [float(w).hex() for w in weights], int(result.stop))
        else:
            box = {}

            def evaluate(rows):
                S = len(rows)
                sets = (L.Params * S)(*[cp for _ in rows])
                ws = np.ascontiguousarray(np.asarray(rows, dtype=np.float64))
                sums = np.zeros(S, dtype=np.dtype(A.VariantModel.SUMMARY_DTYPE))
                L.check(L.lib().anx_evaluate_sweep_confusables_packed(plain.h, ba, len(ba), bg, len(bg), n, pats, J, sets, ws.ctypes.data_as(dp), None, S,
                                                                      sums.ctypes.data_as(C.POINTER(L.GoldSummary)), None))
                box["calls"] = box.get("calls", 0) + 1
                return [(int(s["rank_hist"][0]), int(s["reasons"][L.ANX_GOLD_RANKED]), int(s["rr_fixed"])) for s in sums]

            def call():
                t0 = A.VariantModel.conf_sweep_stats()
                box["calls"] = 0
                box["fit"] = F.greedy(evaluate, J, list(GRID), None, "acc1", MAX_ROUNDS, MIN_GAIN)
                t1 = A.VariantModel.conf_sweep_stats()
                return t1["bytes_down"] - t0["bytes_down"], box["calls"] * (len(ba) + len(bg)) + (t1["batch_runs"] - t0["batch_runs"]) * len(ba), {}

            def outcome():
                f = box["fit"]
                return [[j, g, float(w).hex(), list(c)] for j, g, w, c in f["rounds"]], [float(w).hex() for w in f["weights"]], f["stop"]
        call()   # warms the pools (and builds the vocabulary table)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            down, up, stats = call()
            times.append(time.perf_counter() - t0)
        res["bytes_down"], res["text_bytes_up"], res["times_ms"] = int(down), int(up), [t * 1e3 for t in times]
        res["rounds"], res["weights"], res["stop"] = outcome()
        if side == "a":
            res["state"] = {"pairs": stats["state_pairs"], "slots": stats["state_slots"], "bytes": 24 * stats["state_slots"] + 12 * n + 4 * stats["chunks"],
                            "trial_rounds": stats["rounds"], "trial_launches": stats["trial_launches"]}
            L.kernel_timer(True)
            call()
            res["kernels_ms"] = {k: L.kernel_time(k)[0] for k in KERNELS}
            res["kernel_launches"] = {k: int(L.kernel_time(k)[1]) for k in KERNELS}
            L.kernel_timer(False)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--small", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=1)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), a.reps)
        return 0
    report = {}
    for n in (a.pairs, a.small):
        if n <= 0:
            continue
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
            r[side] = {"median_ms": statistics.median(t), "best_ms": min(t), "bytes_down": runs[side][0]["bytes_down"], "text_bytes_up": runs[side][0]["text_bytes_up"]}
        for k in ("patterns", "grid", "rounds", "weights", "stop", "state", "kernels_ms", "kernel_launches"):
            r[k] = runs["a"][0][k]
        r["agrees"] = all(run[k] == r[k] for run in runs["a"] + runs["b"] for k in ("rounds", "weights", "stop"))
        spread = r["b"]["median_ms"] - r["b"]["best_ms"]
        r["verdict"] = "ok" if r["a"]["median_ms"] < r["b"]["median_ms"] - spread else "NO GAIN: (a) is not below (b)'s median minus (b)'s own spread"
        if not r["agrees"]:
            r["verdict"] = "DEFECT: (a)'s rounds or weights differ from (b)'s"
        report[str(n)] = r
        k, st = r["kernels_ms"], r["state"]
        print(f"{n} pairs, {len(r['patterns'])} patterns x {len(r['grid'])} weights, {len(r['rounds'])} rounds accepted ({st['trial_rounds']} evaluated): "
              f"(a) median {r['a']['median_ms']:.2f} ms (best {r['a']['best_ms']:.2f}), {r['a']['bytes_down']} bytes down, {r['a']['text_bytes_up'] / 1e6:.1f} MB of text up; "
              f"(b) median {r['b']['median_ms']:.2f} ms (best {r['b']['best_ms']:.2f}), {r['b']['bytes_down']} bytes down, {r['b']['text_bytes_up'] / 1e6:.1f} MB of text up; {r['verdict']}")
        print(f"   state: {st['pairs']} pairs with their gold in the cropped list, {st['slots']} slots, {st['bytes'] / 1e6:.1f} MB resident; "
              f"k_fit_gold {k['k_fit_gold']:.3f} ms, k_fit_state {k['k_fit_state']:.3f} ms, k_fit_trials {k['k_fit_trials']:.3f} ms in all = "
              f"{k['k_fit_trials'] / max(r['kernel_launches']['k_fit_trials'], 1):.3f} ms x {r['kernel_launches']['k_fit_trials']} rounds")
        print("   rounds: " + json.dumps([[r["patterns"][x[0]], r["grid"][x[1]], x[3]] for x in r["rounds"]]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
