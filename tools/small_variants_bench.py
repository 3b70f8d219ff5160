#!/usr/bin/env python3
"""Latency of anx_find_variants_batch (host to host) at n = 1, 64, 1 000 on a model with variant lists and on the plain model.

    small_variants_bench.py [--parent-root build/parent] [--series 3] [--calls 200] [--json OUT]

The variant-list model is eng.aspell plus the list the product itself learns (learn_variants, max_matches 3) from 100 000 synth.py
queries and 5 000 words of the lexicon (the words gain links to their neighbours: without them no INDEXED entry holds a VariantOf
link and the lexicon has no variant lists), written out with variant_list_output and read back with read_variants.
Cases, alternating, each series a fresh process: this build, this build under ANX_SMALL=0 (the batch path), and -- with --parent-root,
a checkout of the parent commit (git worktree) with its library built in place -- the parent, through its own Python package.  Per case and size: best and median of --calls calls after 20
warm-up calls; the spread between the series of one build is the yardstick for a difference between builds."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("ANX_BENCH_ROOT") or REPO)   # (a child measuring the parent commit imports that checkout's package)
SIZES = (1, 64, 1000)


def models(tmp, list_path):
    import analiticcl_amd as A
    from analiticcl_amd import synth
    data = synth.materialize_golden(os.path.join(tmp, "data"))
    words = synth.load_lexicon_words(data["eng"])
    out = {}
    for name in ("plain", "variants"):
        g = A.VariantModel(data["alphabet"], A.Weights(), device=0)
        g.read_lexicon(data["eng"])
        if name == "variants" and list_path:
            g.read_variants(list_path, False)
        g.build()
        out[name] = g
    return A, synth, words, out


def make_list(path):
    with tempfile.TemporaryDirectory() as tmp:
        A, synth, words, m = models(tmp, None)
        rng = random.Random(5)
        inputs = rng.sample([w for w in words if 4 <= len(w) <= 12 and w.isalpha()], 5000) + synth.make_queries(words, 100_000, max_len=16, seed=synth.SEED)
        m["plain"].learn_variants(inputs, A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=3), strict=True, auto_build=False)
        with open(path, "w", encoding="utf-8") as f:
            f.write(m["plain"].variant_list_output())


def child(list_path, calls):
    from analiticcl_amd import _lib as LL
    with tempfile.TemporaryDirectory() as tmp:
        A, synth, words, m = models(tmp, list_path)
        L = A.lib()
        p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
        cp = p._c()
        queries = synth.make_queries(words, 1000, max_len=16, seed=77)
        stats = (C.c_uint64 * 2)()
        res = {}
        for name, g in m.items():
            for n in SIZES:
                arr = (C.c_char_p * n)(*[q.encode("utf-8") for q in queries[:n]])
                ts, rows_total, with_via = [], 0, 0
                L.anx_debug_small_stats(stats)
                taken0 = stats[0]
                for i in range(calls + 20):
                    rows = C.POINTER(LL.Result)()
                    offs = C.POINTER(C.c_size_t)()
                    t = time.perf_counter()
                    rc = L.anx_find_variants_batch(g.h, arr, n, C.byref(cp), C.byref(rows), C.byref(offs))
                    dt = time.perf_counter() - t
                    assert rc == 0, LL.last_error()
                    if i == 0:
                        rows_total = offs[n]
                        with_via = sum(1 for r in range(rows_total) if rows[r].via != 0xFFFFFFFFFFFFFFFF)
                    L.anx_results_free(rows, offs)
                    if i >= 20:
                        ts.append(dt * 1e6)
                L.anx_debug_small_stats(stats)
                res[f"{name}/{n}"] = dict(best_us=min(ts), median_us=statistics.median(ts), rows=rows_total, rows_with_via=with_via,
                                          small_calls=int(stats[0] - taken0))
        print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root")
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--json")
    ap.add_argument("--child")
    ap.add_argument("--make-list")
    a = ap.parse_args()
    if a.make_list:
        return make_list(a.make_list)
    if a.child:
        return child(a.child, a.calls)
    tmp = tempfile.mkdtemp(prefix="anx_small_variants_")
    list_path = os.path.join(tmp, "learned.variants.tsv")
    me = [sys.executable, os.path.abspath(__file__)]
    subprocess.run(me + ["--make-list", list_path], check=True, timeout=600)
    cases = [("this", {}), ("this ANX_SMALL=0", {"ANX_SMALL": "0"})]
    if a.parent_root:
        cases.append(("parent", {"ANX_BENCH_ROOT": os.path.abspath(a.parent_root)}))
    runs = {name: [] for name, _ in cases}
    for s in range(a.series):
        for name, env in cases:   # a failing case ends the measurement (nothing more is started on the device)
            r = subprocess.run(me + ["--child", list_path, "--calls", str(a.calls)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600, check=True)
            line = [x for x in r.stdout.split("\n") if x.startswith("RESULT ")][-1]
            runs[name].append(json.loads(line[7:]))
            print(f"series {s} {name}: " + "  ".join(f"{k} {v['median_us']:.0f}" for k, v in runs[name][-1].items()), flush=True)
    print("\nmedian us of each series (best us of all series) | spread = max - min of the series' medians")
    for model in ("variants", "plain"):
        print(f"\n{model} model" + (f"  (rows per call: " + ", ".join(f"n={n}: {runs['this'][0][f'{model}/{n}']['rows']} rows, {runs['this'][0][f'{model}/{n}']['rows_with_via']} with via" for n in SIZES) + ")"))
        for name, _ in cases:
            cells = []
            for n in SIZES:
                med = [r[f"{model}/{n}"]["median_us"] for r in runs[name]]
                best = min(r[f"{model}/{n}"]["best_us"] for r in runs[name])
                small = runs[name][0][f"{model}/{n}"]["small_calls"]
                cells.append(f"n={n}: " + " / ".join(f"{x:.0f}" for x in med) + f" (best {best:.0f}, spread {max(med) - min(med):.0f}, small path {small}/{a.calls + 20})")
            print(f"  {name:18s} " + "   ".join(cells))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    main()
