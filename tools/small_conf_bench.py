#!/usr/bin/env python3
"""Latency of anx_find_variants_batch (host to host) at n = 1, 64, 1 000 on a model with a confusable list, late and early weighting,
and on the plain model.

    small_conf_bench.py [--parent-root build/parent] [--dbg-lib build/libanx_dbg.so] [--series 3] [--calls 200] [--json OUT]

The confusable model is nld.aspell + tests/golden/data/confusables10.tsv (late: the default; early: set_confusables_before_pruning);
the plain model is nld.aspell alone (the regression guard: the feature adds a branch and lazily created buffers, nothing on its chain).
Cases, alternating, each series a fresh process: this build, this build under ANX_SMALL=0 (the batch path), and -- with --parent-root, a
checkout of the parent commit (git worktree) with its library built in place -- the parent, through its own Python package.  With
--dbg-lib (tools/build_flags.sh dbg "-DANX_DEBUG_SWITCHES") two more: that library as it is (k_small_conf_order) and under
ANX_SMALL_CONF_ORDER=identity (k_conf_script takes the list as k_conf_screen left it).  Per case and size: best and median of --calls
calls after 20 warm-up calls; the spread between the series of one build is the yardstick for a difference between builds."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("ANX_BENCH_ROOT") or REPO)   # (a child measuring the parent commit imports that checkout's package)
SIZES = (1, 64, 1000)
MODELS = ("late", "early", "plain")
CONF10 = os.path.join(REPO, "tests", "golden", "data", "confusables10.tsv")


def child(calls):
    import analiticcl_amd as A
    from analiticcl_amd import _lib as LL
    from analiticcl_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        data = synth.materialize_golden(os.path.join(tmp, "data"))
        words = synth.load_lexicon_words(data["nld"])
        L = A.lib()
        cp = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)._c()
        queries = synth.make_queries(words, 1000, max_len=16, seed=77)
        stats = (C.c_uint64 * 2)()
        cstats = (C.c_uint64 * 3)()
        have_cstats = hasattr(L, "anx_debug_small_conf_stats")   # (the parent commit has none)
        res = {}
        for name in MODELS:
            g = A.VariantModel(data["alphabet"], A.Weights(), device=0)
            g.read_lexicon(data["nld"])
            if name != "plain":
                g.read_confusablelist(CONF10)
            if name == "early":
                g.set_confusables_before_pruning()
            g.build()
            for n in SIZES:
                arr = (C.c_char_p * n)(*[q.encode("utf-8") for q in queries[:n]])
                ts, rows_total = [], 0
                L.anx_debug_small_stats(stats)
                taken0 = stats[0]
                if have_cstats:
                    L.anx_debug_small_conf_stats(cstats)
                scripts0 = cstats[1]
                for i in range(calls + 20):
                    rows = C.POINTER(LL.Result)()
                    offs = C.POINTER(C.c_size_t)()
                    t = time.perf_counter()
                    rc = L.anx_find_variants_batch(g.h, arr, n, C.byref(cp), C.byref(rows), C.byref(offs))
                    dt = time.perf_counter() - t
                    assert rc == 0, LL.last_error()
                    if i == 0:
                        rows_total = offs[n]
                    L.anx_results_free(rows, offs)
                    if i >= 20:
                        ts.append(dt * 1e6)
                L.anx_debug_small_stats(stats)
                if have_cstats:
                    L.anx_debug_small_conf_stats(cstats)
                res[f"{name}/{n}"] = dict(best_us=min(ts), median_us=statistics.median(ts), rows=rows_total, small_calls=int(stats[0] - taken0),
                                          scripts_per_call=int(cstats[1] - scripts0) // (calls + 20))
        print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root")
    ap.add_argument("--dbg-lib")
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.calls)
    if a.series < 2:
        ap.error("--series: at least two (the spread between them is the yardstick)")
    me = [sys.executable, os.path.abspath(__file__)]
    cases = [("this", {}), ("this ANX_SMALL=0", {"ANX_SMALL": "0"})]
    if a.parent_root:
        cases.append(("parent", {"ANX_BENCH_ROOT": os.path.abspath(a.parent_root)}))
    if a.dbg_lib:
        lib = os.path.abspath(a.dbg_lib)
        cases += [("dbg order kernel", {"ANX_LIB": lib}), ("dbg identity order", {"ANX_LIB": lib, "ANX_SMALL_CONF_ORDER": "identity"})]
    runs = {name: [] for name, _ in cases}
    for s in range(a.series):
        for name, env in cases:   # a failing case ends the measurement (nothing more is started on the device)
            r = subprocess.run(me + ["--child", "--calls", str(a.calls)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600, check=True)
            line = [x for x in r.stdout.split("\n") if x.startswith("RESULT ")][-1]
            runs[name].append(json.loads(line[7:]))
            print(f"series {s} {name}: " + "  ".join(f"{k} {v['median_us']:.0f}" for k, v in runs[name][-1].items()), flush=True)
    print("\nmedian us of each series (best us of all series) | spread = max - min of the series' medians")
    for model in MODELS:
        first = runs["this"][0]
        print(f"\n{model} model  (" + ", ".join(f"n={n}: {first[f'{model}/{n}']['rows']} rows, {first[f'{model}/{n}']['scripts_per_call']} edit scripts" for n in SIZES) + ")")
        for name, _ in cases:
            cells = []
            for n in SIZES:
                med = [r[f"{model}/{n}"]["median_us"] for r in runs[name]]
                best = min(r[f"{model}/{n}"]["best_us"] for r in runs[name])
                small = runs[name][0][f"{model}/{n}"]["small_calls"]
                cells.append(f"n={n}: " + " / ".join(f"{x:.0f}" for x in med) + f" (best {best:.0f}, spread {max(med) - min(med):.0f}, small path {small}/{a.calls + 20})")
            print(f"  {name:18s} " + "   ".join(cells))
        if a.parent_root:   # the verdicts: medians of the series' medians against the parent's own spread
            for n in SIZES:
                mine = statistics.median(r[f"{model}/{n}"]["median_us"] for r in runs["this"])
                par = [r[f"{model}/{n}"]["median_us"] for r in runs["parent"]]
                pm, spread = statistics.median(par), max(par) - min(par)
                if model == "plain":
                    verdict = "within the parent's spread" if abs(mine - pm) <= spread else "OUTSIDE the parent's spread"
                else:
                    verdict = "faster by more than the parent's spread" if pm - mine > spread else "NOT faster by more than the parent's spread"
                print(f"  verdict n={n}: this {mine:.0f} us, parent {pm:.0f} us (spread {spread:.0f}): {verdict}")
    if a.dbg_lib:
        print("\norder kernel against identity order (the -DANX_DEBUG_SWITCHES library, both)")
        for model in ("late", "early"):
            for n in SIZES:
                k = [r[f"{model}/{n}"]["median_us"] for r in runs["dbg order kernel"]]
                i = [r[f"{model}/{n}"]["median_us"] for r in runs["dbg identity order"]]
                print(f"  {model} n={n}: order kernel {statistics.median(k):.0f} us (spread {max(k) - min(k):.0f}), identity {statistics.median(i):.0f} us (spread {max(i) - min(i):.0f})")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    main()
