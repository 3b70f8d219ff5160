#!/usr/bin/env python3
"""anx_evaluate_sweep_confusables against what a user does without it: one model per candidate list, on eng.aspell.

    sweep_confusables_bench.py [--pairs 1000000] [--small 10000] [--reps 5] [--procs 2] [--json OUT]

Pairs: (edited query, source word) -- one to three random edits of lexicon words, seeded.  Candidates: the 20 commonest representable
patterns mine_confusables finds on those pairs; 3 weights (1.1, 1.25, 0.9), one pattern on per set, the baseline first: 61 sets, late,
all at k = 3, d = 2, n = 10.
  (a) one anx_evaluate_sweep_confusables_packed call with out == NULL on ONE plain model: two blobs in, 624 bytes per set out.
  (b) what gives the same answer today: per set a model holding the set's list (created, its lexicon read, the 20 patterns added,
      built and uploaded) and one anx_evaluate_sweep_packed call with the one parameter set.  The 61 models are built once per process
      (that time is reported on its own) and stay resident; the timed region of (b) is the 61 evaluation calls alone ("without builds");
      "with builds" adds the builds.
Every measurement runs in a fresh process, (a) and (b) alternating, --procs processes each, --reps timed calls after one warm-up call;
the packing of the Python lists into blobs is outside the timed region for both.  Reported: median and best per side, the bytes each
side downloads and uploads as text, and from one extra call of (a): the kernel times from the library's kernel timer (once per call:
k_cs_screen, the sort, k_cs_mask; per set: the fill, k_rank, the late apply, the classify), the screen's share, the rows the host
computed, and one more call with every mask computed on the host (ANX_CONFUSABLES=host) against the device's mask pass.  (a)'s
summaries are held against (b)'s.  The verdict asks that (a)'s median lie below (b)-without-builds' median minus (b)'s own
best-to-median spread; nothing is compared against the code under test.  The same again for --small pairs."""
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

CANDIDATES, WEIGHTS = 20, (1.1, 1.25, 0.9)
ONCE = ("k_rw_base", "k_rw_pre", "k_cs_score", "k_cs_screen", "k_cs_order", "k_cs_mask")
PER_SET = ("k_cs_fill", "k_rank (confusable sweep)", "k_cs_slot_w", "k_conf_apply_late (confusable sweep)", "k_rw_classify")


def child(side, n, reps):
    import ctypes as C

    import numpy as np

    import analiticcl_amd as A
    from analiticcl_amd import _lib as L
    from analiticcl_amd import cli, synth
    from analiticcl_amd.model import _pack
    from eval_twin import edited_pairs
    with tempfile.TemporaryDirectory() as tmp:
        data = synth.materialize_golden(os.path.join(tmp, "data"))
        words = synth.load_lexicon_words(data["eng"])
        pairs = edited_pairs(words, n, seed=7)
        ba, bg = _pack([a for a, _ in pairs]), _pack([b for _, b in pairs])
        P = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)

        def model(weights=None):
            g = A.VariantModel(data["alphabet"], A.Weights(), device=0)
            g.read_lexicon(data["eng"])
            for p, w in zip(patterns, weights or ()):
                g.add_to_confusables(p, w)
            g.build()
            return g

        patterns = []
        plain = model()
        patterns = [r["pattern"] for r in plain.mine_confusables([a for a, _ in pairs], [b for _, b in pairs]) if r["representable"]][:CANDIDATES]
        labels, rows = cli.candidate_grid(patterns, list(WEIGHTS))
        S, J = len(rows), len(patterns)
        sets = (L.Params * S)(*[P._c() for _ in rows])
        pats = (C.c_char_p * J)(*[p.encode() for p in patterns])
        ws = np.ascontiguousarray(np.asarray(rows, dtype=np.float64))
        one = (L.Params * 1)(P._c())
        sums = np.zeros(S, dtype=np.dtype(A.VariantModel.SUMMARY_DTYPE))
        res = {"side": side, "pairs": n, "sets": S, "patterns": patterns}

        def per_model(models):
            got = np.zeros(S, dtype=sums.dtype)
            for s, g in enumerate(models):
                L.check(L.lib().anx_evaluate_sweep_packed(g.h, ba, len(ba), bg, len(bg), n, one, 1, got[s:s + 1].ctypes.data_as(C.POINTER(L.GoldSummary)), None, None))
            return got

        if side == "a":
            def call():
                t0 = A.VariantModel.conf_sweep_stats()
                L.check(L.lib().anx_evaluate_sweep_confusables_packed(plain.h, ba, len(ba), bg, len(bg), n, pats, J, sets, ws.ctypes.data_as(C.POINTER(C.c_double)), None, S,
                                                                      sums.ctypes.data_as(C.POINTER(L.GoldSummary)), None))
                t1 = A.VariantModel.conf_sweep_stats()
                return t1["bytes_down"] - t0["bytes_down"], len(ba) + len(bg) + (t1["batch_runs"] - t0["batch_runs"]) * len(ba)   # the pair side once, the inputs per batch run
        else:
            t0 = time.perf_counter()
            models = [model(r) for r in rows]
            res["builds_ms"] = (time.perf_counter() - t0) * 1e3

            def call():
                t0 = A.VariantModel.sweep_stats()["bytes_down"]
                per_model(models)
                return A.VariantModel.sweep_stats()["bytes_down"] - t0, S * (len(ba) + len(bg) + len(ba))   # per set: the pair side and one batch run
        call()   # warms the pools (and builds the vocabulary table)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            down, up = call()
            times.append(time.perf_counter() - t0)
        res["bytes_down"], res["text_bytes_up"] = int(down), int(up)
        res["times_ms"] = [t * 1e3 for t in times]
        if side == "a":
            L.kernel_timer(True)
            t0 = A.VariantModel.conf_sweep_stats()
            call()
            t1 = A.VariantModel.conf_sweep_stats()
            res["kernels_ms"] = {k: L.kernel_time(k)[0] for k in ONCE + PER_SET}
            res["kernel_launches"] = {k: int(L.kernel_time(k)[1]) for k in ONCE + PER_SET}
            L.kernel_timer(False)
            res.update({k: t1[k] - t0[k] for k in ("batch_runs", "base_rows", "rows_listed", "rows_patched")})
            device_sums = sums.copy()
            L.set_switch("ANX_CONFUSABLES", "host")
            t0 = time.perf_counter()
            call()
            res["host_masks_call_ms"] = (time.perf_counter() - t0) * 1e3
            L.set_switch("ANX_CONFUSABLES", None)
            res["host_masks_agree"] = bool(sums.tobytes() == device_sums.tobytes())
            sums[:] = device_sums
            ref = per_model([model(r) for r in rows])
            res["agrees"] = bool(ref.tobytes() != bytes(ref.nbytes)) and all(
                all(np.array_equal(sums[k][s], ref[k][s]) for k in ("n", "gold_known", "reasons", "rank_hist", "rr_fixed", "n_results")) for s in range(S))
            # (gained / lost compare with set 0, which only (a) knows: they are not held against (b))
            mine = [A.VariantModel.sweep_summary(s) for s in sums]
            res["summary"] = [{"pattern": labels[i][0], "weight": labels[i][1], "accuracy_at_1": m["accuracy_at_1"], "mrr": m["mrr"], "ranked": m["reasons"]["RANKED"],
                               "gained_at_1": m["gained_at_1"], "lost_at_1": m["lost_at_1"]} for i, m in enumerate(mine)]
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
        r["b"]["builds_ms"] = statistics.median(run["builds_ms"] for run in runs["b"])
        for k in ("sets", "patterns", "kernels_ms", "kernel_launches", "batch_runs", "base_rows", "rows_listed", "rows_patched", "host_masks_call_ms", "host_masks_agree", "agrees",
                  "summary"):
            r[k] = runs["a"][0][k]
        spread = r["b"]["median_ms"] - r["b"]["best_ms"]
        r["verdict"] = "ok" if r["a"]["median_ms"] < r["b"]["median_ms"] - spread else "NO GAIN: (a) is not below (b)'s median minus (b)'s own spread"
        if not r["agrees"] or not r["host_masks_agree"]:
            r["verdict"] = "DEFECT: (a)'s summaries differ from (b)'s, or the host's masks from the device's"
        report[str(n)] = r
        S = r["sets"]
        print(f"{n} pairs, {S} sets: (a) median {r['a']['median_ms']:.2f} ms (best {r['a']['best_ms']:.2f}), {r['a']['bytes_down']} bytes down, "
              f"{r['a']['text_bytes_up'] / 1e6:.1f} MB of text up; (b) without builds median {r['b']['median_ms']:.2f} ms (best {r['b']['best_ms']:.2f}), with its "
              f"{S} model builds {r['b']['median_ms'] + r['b']['builds_ms']:.0f} ms, {r['b']['bytes_down']} bytes down, {r['b']['text_bytes_up'] / 1e6:.1f} MB of text up; {r['verdict']}")
        print("   kernels of one call of (a), ms in all (per launch x launches): " +
              ", ".join(f"{k} {v:.3f} ({v / max(r['kernel_launches'][k], 1):.3f} x {r['kernel_launches'][k]})" for k, v in r["kernels_ms"].items()))
        print(f"   base rows: {r['base_rows']}, listed for an edit script: {r['rows_listed']} ({100.0 * r['rows_listed'] / max(r['base_rows'], 1):.1f} %: the screen drops the rest), "
              f"rows on the host: {r['rows_patched']}, batch runs of that call: {r['batch_runs']}")
        print(f"   one call with every mask on the host (ANX_CONFUSABLES=host): {r['host_masks_call_ms']:.1f} ms, summaries equal: {r['host_masks_agree']}")
        print("   summaries: " + json.dumps(r["summary"][:4]) + " ...", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
