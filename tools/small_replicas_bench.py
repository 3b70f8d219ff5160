#!/usr/bin/env python3
"""Latency of anx_find_variants_batch (host to host) at n = 1, 64, 1 000 on eng.aspell for a model on [0], [0, 0] and [0, 0, 0], and the
aggregate rate of 8 threads issuing 1 000-input calls on the [0, 0, 0] model.

    small_replicas_bench.py [--parent-root build/parent] [--series 3] [--calls 200] [--json OUT]

Cases, alternating, each series a fresh process: this build and -- with --parent-root, a checkout of the parent commit with its library
built in place -- the parent, through its own Python package.  Per case, model and size: best and median of --calls calls after 20
warm-up calls.  Two verdicts are printed:
  (a) multi-device latency: the median of this build on [0, 0] / [0, 0, 0] against the parent on the same model (the gain), and against
      this build's one-replica median, within that configuration's own best-to-median spread;
  (b) one-replica latency: this build's median on [0] against the parent's, within the parent's own best-to-median spread (the replica
      choice adds atomics to the path).
The replicas share one GPU here: the thread figure shows that the calls spread over the replicas (anx_debug_small_replica_stats), it
does not show N-GPU scaling."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("ANX_BENCH_ROOT") or REPO)   # (a child measuring the parent commit imports that checkout's package)
SIZES = (1, 64, 1000)
LAYOUTS = ((0,), (0, 0), (0, 0, 0))
THREADS, THREAD_CALLS = 8, 40


def child(calls):
    import analiticcl_amd as A
    from analiticcl_amd import _lib as LL
    from analiticcl_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        data = synth.materialize_golden(os.path.join(tmp, "data"))
        words = synth.load_lexicon_words(data["eng"])
        L = A.lib()
        p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
        cp = p._c()
        queries = synth.make_queries(words, 1000, max_len=16, seed=77)
        stats = (C.c_uint64 * 2)()
        res = {}

        def one_call(g, arr, n):
            rows = C.POINTER(LL.Result)()
            offs = C.POINTER(C.c_size_t)()
            t = time.perf_counter()
            rc = L.anx_find_variants_batch(g.h, arr, n, C.byref(cp), C.byref(rows), C.byref(offs))
            dt = time.perf_counter() - t
            assert rc == 0, LL.last_error()
            L.anx_results_free(rows, offs)
            return dt

        for devices in LAYOUTS:
            g = A.VariantModel(data["alphabet"], A.Weights(), devices=list(devices))
            g.read_lexicon(data["eng"])
            g.build()
            name = "x".join(str(d) for d in devices)
            for n in SIZES:
                arr = (C.c_char_p * n)(*[q.encode("utf-8") for q in queries[:n]])
                L.anx_debug_small_stats(stats)
                taken0 = stats[0]
                ts = [one_call(g, arr, n) * 1e6 for _ in range(calls + 20)][20:]
                L.anx_debug_small_stats(stats)
                res[f"{name}/{n}"] = dict(best_us=min(ts), median_us=statistics.median(ts), small_calls=int(stats[0] - taken0))
            if len(devices) == 3:   # 8 threads x THREAD_CALLS calls of 1 000 inputs: queries per second over all of them
                arr = (C.c_char_p * 1000)(*[q.encode("utf-8") for q in queries])
                before = g.small_replica_stats() if hasattr(g, "small_replica_stats") else None
                barrier = threading.Barrier(THREADS + 1)

                def work():
                    barrier.wait()
                    for _ in range(THREAD_CALLS):
                        one_call(g, arr, 1000)
                th = [threading.Thread(target=work) for _ in range(THREADS)]
                for t in th:
                    t.start()
                barrier.wait()
                t0 = time.perf_counter()
                for t in th:
                    t.join()
                dt = time.perf_counter() - t0
                res["threads"] = dict(queries_per_s=THREADS * THREAD_CALLS * 1000 / dt,
                                      per_replica=[b - a for a, b in zip(before, g.small_replica_stats())] if before is not None else None)
            del g
        print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root")
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.calls)
    me = [sys.executable, os.path.abspath(__file__)]
    cases = [("this", {})]
    if a.parent_root:
        cases.append(("parent", {"ANX_BENCH_ROOT": os.path.abspath(a.parent_root)}))
    runs = {name: [] for name, _ in cases}
    for s in range(a.series):
        for name, env in cases:   # a failing case ends the measurement (nothing more is started on the device)
            r = subprocess.run(me + ["--child", "--calls", str(a.calls)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600, check=True)
            line = [x for x in r.stdout.split("\n") if x.startswith("RESULT ")][-1]
            runs[name].append(json.loads(line[7:]))
            print(f"series {s} {name}: " + "  ".join(f"{k} {v['median_us']:.0f}" for k, v in runs[name][-1].items() if k != "threads")
                  + f"  threads {runs[name][-1]['threads']['queries_per_s'] / 1e6:.2f} Mq/s", flush=True)

    def med(name, key):   # median over the series of the per-series medians, and the best of all series
        return statistics.median(r[key]["median_us"] for r in runs[name]), min(r[key]["best_us"] for r in runs[name])

    print("\nmedian us (best us) over the series; small path = calls of the first series it answered")
    for devices in LAYOUTS:
        layout = "x".join(str(d) for d in devices)
        for name, _ in cases:
            cells = []
            for n in SIZES:
                m, b = med(name, f"{layout}/{n}")
                cells.append(f"n={n}: {m:.0f} ({b:.0f}), small path {runs[name][0][f'{layout}/{n}']['small_calls']}/{a.calls + 20}")
            print(f"  [{layout.replace('x', ', ')}] {name:7s} " + "   ".join(cells))
    for name, _ in cases:
        qps = [r["threads"]["queries_per_s"] for r in runs[name]]
        print(f"  8 threads x 1000 inputs on [0, 0, 0], {name}: " + " / ".join(f"{x / 1e6:.2f}" for x in qps) + f" Mq/s, calls per replica {runs[name][0]['threads']['per_replica']}")
    if a.parent_root:
        print("\nverdicts (median against median; margin = the reference configuration's own median - best)")
        for layout in ("0x0", "0x0x0"):
            for n in SIZES:
                m, _b = med("this", f"{layout}/{n}")
                pm, _pb = med("parent", f"{layout}/{n}")
                m1, b1 = med("this", f"0/{n}")
                print(f"  (a) [{layout.replace('x', ', ')}] n={n}: parent {pm:.0f} -> this {m:.0f} us; one replica {m1:.0f} us, margin {m1 - b1:.0f}: "
                      + ("reached" if m <= m1 + (m1 - b1) else "NOT reached"))
        for n in SIZES:
            m, _b = med("this", f"0/{n}")
            pm, pb = med("parent", f"0/{n}")
            print(f"  (b) [0] n={n}: parent {pm:.0f} (best {pb:.0f}) -> this {m:.0f} us, margin {pm - pb:.0f}: " + ("within" if m <= pm + (pm - pb) else "OUTSIDE"))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    main()
