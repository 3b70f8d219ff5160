#!/usr/bin/env python3
"""anx_score_pairs_weighted against anx_score_pairs on nld.aspell + confusables10.tsv, host buffer to host memory.

    score_pairs_conf_bench.py [--pairs 1000000] [--reps 5] [--parent-tree DIR] [--rounds 3] [--dbg-lib LIB] [--json OUT]

The pairs are (synth query, nearest lexicon word: the first ranked row of find_variants, max_matches 1; a query without a row is
paired with itself).  The main process builds them once and leaves the two packed blobs in a temporary directory; every measurement
is a fresh child process that loads the blobs, builds the model and makes one warming call and --reps timed ones:
  weighted   : anx_score_pairs_weighted_packed -- best and median, and per timed call the time of k_pairs_conf_screen, the sort of the
               list by shape key (k_pairs_conf_order) and k_pairs_conf_script (the library's kernel timer, anx_debug_kernel_time), the
               share of pairs the screen removed, the
               scripts run on the device and the pairs left to the host (anx_debug_pairs_conf_stats);
  unweighted : anx_score_pairs_packed on the same pairs;
  host       : the weighted call under ANX_CONFUSABLES=host -- anx_model_confusable_weight_text over every scorable pair on up to 16
               host threads; its median minus the unweighted median is the CPU baseline of the weighting.
--dbg-lib: a library built with -DANX_DEBUG_SWITCHES (tools/build_flags.sh dbg "-DANX_DEBUG_SWITCHES").  Two more weighted children run
with it, under ANX_PAIRS_CONF_ORDER=identity (the list in the screen's order, no sort) and as it is (shape-key order): experiment (b).
The order stays only if sort + script, median of the timed calls, lies below the script's median in the screen's order by more than
that configuration's own best-to-median spread.  Experiment (a), the lane memories in LDS for short pairs, lost by the same rule and
its kernel is not in the tree: HISTORY.md has its figures.
--parent-tree: a checkout of the parent commit with its library built in place (git archive <parent> | tar -x -C DIR, then
python -m analiticcl_amd.build there).  The unweighted child then runs --rounds times from this tree and from the parent's in turn,
and the tool says whether this build's median lies within the parent's own best-to-median spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("ANX_BENCH_TREE") or REPO)  # a child of --parent-tree imports the parent's package and library
KERNELS = ["k_pairs_conf_screen", "k_pairs_conf_order", "k_pairs_conf_script", "k_pairs_short", "k_pairs_long"]


def model_of(data, confusables):
    import analiticcl_amd as A
    g = A.VariantModel(data["alphabet"], A.Weights(), device=0)
    g.read_lexicon(data["nld"])
    if confusables:
        g.read_confusablelist(confusables)
    g.build()
    return g


def child(a):
    """one measurement in this (fresh) process -> one JSON line"""
    import ctypes as C
    import analiticcl_amd as A
    from analiticcl_amd import _lib as L
    from analiticcl_amd import synth
    data = synth.materialize_golden(os.path.join(a.dir, "data"))
    g = model_of(data, os.path.join(synth.GOLDEN_DATA, "confusables10.tsv"))
    ba, bb = open(os.path.join(a.dir, "a.bin"), "rb").read(), open(os.path.join(a.dir, "b.bin"), "rb").read()
    n = a.pairs
    out = (L.PairScore * n)()
    w = (C.c_double * n)()
    lib = L.lib()
    weighted = a.child != "unweighted"
    has_weighted = hasattr(A.VariantModel, "pairs_conf_stats")  # (not in the parent's tree)
    if a.child == "host":
        A.set_switch("ANX_CONFUSABLES", "host")
    times, ktimes, st = [], [], []
    for rep in range(a.reps + 1):  # (the first call warms the pools and uploads the pattern tables)
        L.kernel_timer(True)
        s0 = A.VariantModel.pairs_conf_stats() if has_weighted else None
        t0 = time.perf_counter()
        if weighted:
            L.check(lib.anx_score_pairs_weighted_packed(g.h, ba, len(ba), bb, len(bb), n, out, w))
        else:
            L.check(lib.anx_score_pairs_packed(g.h, ba, len(ba), bb, len(bb), n, out))
        times.append(time.perf_counter() - t0)
        kt = {}
        for k in KERNELS:
            try:
                kt[k] = L.kernel_time(k)[0]
            except Exception:  # noqa: BLE001 (no launch of that kernel was timed)
                pass
        L.kernel_timer(False)
        ktimes.append(kt)
        if has_weighted:
            s1 = A.VariantModel.pairs_conf_stats()
            st.append({k: s1[k] - s0[k] for k in s1})
    times, ktimes = times[1:], ktimes[1:]
    res = {"mode": a.child, "lib": L.LIB_PATH, "pairs": n, "best_ms": min(times) * 1e3, "median_ms": statistics.median(times) * 1e3,
           "times_ms": [t * 1e3 for t in times], "kernels_ms": {k: [kt[k] for kt in ktimes if k in kt] for k in KERNELS},
           "stats": st[-1] if st else None, "checksum": sum(w[i] for i in range(0, n, 97)) if weighted else None}
    print("RESULT " + json.dumps(res), flush=True)


def run_child(a, mode, env_extra=None, tree=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    if tree:
        env["ANX_BENCH_TREE"] = tree
        env.pop("ANX_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--dir", a.dir, "--pairs", str(a.pairs), "--reps", str(a.reps)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if r.returncode != 0:
        raise SystemExit(f"child {mode} failed with status {r.returncode}: no further child is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    line = [x for x in r.stdout.split("\n") if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def kstat(v):
    return (min(v), statistics.median(v)) if v else (float("nan"), float("nan"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--dbg-lib", default=None, help="a -DANX_DEBUG_SWITCHES build: shape-key order against the screen's order")
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        return child(a)
    with tempfile.TemporaryDirectory() as tmp:
        a.dir = tmp
        # the pairs, from a child of their own (this process never opens the GPU): the plain model's nearest word
        prep = ("import os,sys; sys.path.insert(0, %r)\n"
                "import analiticcl_amd as A\nfrom analiticcl_amd import synth\nfrom analiticcl_amd.model import _pack\n"
                "d = synth.materialize_golden(os.path.join(%r, 'data'))\n"
                "g = A.VariantModel(d['alphabet'], A.Weights(), device=0); g.read_lexicon(d['nld']); g.build()\n"
                "qs = synth.make_queries(synth.load_lexicon_words(d['nld']), %d, max_len=16, seed=8)\n"
                "near = g.find_variants_ids(qs, A.SearchParameters(max_anagram_distance=3, max_edit_distance=3, max_matches=1, score_threshold=0.0))\n"
                "open(os.path.join(%r, 'a.bin'), 'wb').write(_pack(qs))\n"
                "open(os.path.join(%r, 'b.bin'), 'wb').write(_pack([g.vocab_text(r[0][0]) if r else q for q, r in zip(qs, near)]))\n"
                % (REPO, tmp, a.pairs, tmp, tmp))
        r = subprocess.run([sys.executable, "-c", prep], capture_output=True, text=True, timeout=a.child_timeout)
        if r.returncode != 0:
            raise SystemExit(f"building the pairs failed with status {r.returncode}\n{r.stderr[-4000:]}")
        res = {"weighted": run_child(a, "weighted"), "unweighted": [run_child(a, "unweighted")], "host": run_child(a, "host"), "env": {}, "parent": []}
        wt, un, ho = res["weighted"], res["unweighted"][0], res["host"]
        st = wt["stats"]
        print(f"weighted   {a.pairs} pairs: best {wt['best_ms']:.2f} ms, median {wt['median_ms']:.2f} ms = {a.pairs / wt['median_ms'] / 1e3:.2f} M pairs/s")
        print(f"unweighted {a.pairs} pairs: best {un['best_ms']:.2f} ms, median {un['median_ms']:.2f} ms = {a.pairs / un['median_ms'] / 1e3:.2f} M pairs/s")
        for k in KERNELS:
            if wt["kernels_ms"][k]:
                b, m = kstat(wt["kernels_ms"][k])
                print(f"  {k}: best {b:.3f} ms, median {m:.3f} ms per call")
        print(f"  screen removed {st['screened']} of {st['pairs']} pairs ({100.0 * st['screened'] / max(1, st['pairs']):.1f} %), "
              f"{st['device_scripts']} scripts on the device, {st['host_pairs']} pairs on the host")
        print(f"host (ANX_CONFUSABLES=host, up to 16 threads): median {ho['median_ms']:.2f} ms; weighting alone {ho['median_ms'] - un['median_ms']:.2f} ms "
              f"against {wt['median_ms'] - un['median_ms']:.2f} ms on the device; checksum equal: {ho['checksum'] == wt['checksum']}")
        if a.dbg_lib:
            lib = os.path.abspath(a.dbg_lib)
            ident = run_child(a, "weighted", env_extra={"ANX_LIB": lib, "ANX_PAIRS_CONF_ORDER": "identity"})
            shape = run_child(a, "weighted", env_extra={"ANX_LIB": lib})
            res["env"] = {"identity": ident, "shape": shape}
            gb, gm = kstat(ident["kernels_ms"]["k_pairs_conf_script"])
            tot = [x + y for x, y in zip(shape["kernels_ms"]["k_pairs_conf_script"], shape["kernels_ms"]["k_pairs_conf_order"])]
            b, m = kstat(tot)
            print(f"experiment (b), shape-key order: sort + script best {b:.3f} ms, median {m:.3f} ms (script {kstat(shape['kernels_ms']['k_pairs_conf_script'])[1]:.3f}, "
                  f"sort {kstat(shape['kernels_ms']['k_pairs_conf_order'])[1]:.3f}) against the screen's order: script best {gb:.3f} / median {gm:.3f} ms "
                  f"(spread {gm - gb:.3f} ms): {'KEEP' if gm - m > gm - gb else 'REMOVE'}; call medians {shape['median_ms']:.2f} / {ident['median_ms']:.2f} ms; "
                  f"checksums equal: {shape['checksum'] == ident['checksum'] == wt['checksum']}")
            print("experiment (a), lane memories in LDS for short pairs: lost (HISTORY.md), not in the tree")
        if a.parent_tree:
            for _ in range(a.rounds):
                res["parent"].append(run_child(a, "unweighted", tree=os.path.abspath(a.parent_tree)))
                res["unweighted"].append(run_child(a, "unweighted"))
            pt = [t for x in res["parent"] for t in x["times_ms"]]
            ut = [t for x in res["unweighted"][1:] for t in x["times_ms"]]
            pb, pm, um = min(pt), statistics.median(pt), statistics.median(ut)
            print(f"anx_score_pairs, {a.rounds} fresh processes each in turn: parent best {pb:.2f} ms, median {pm:.2f} ms (spread {pm - pb:.2f} ms); "
                  f"this build best {min(ut):.2f} ms, median {um:.2f} ms: {'within' if um <= pm + (pm - pb) else 'OUTSIDE'} the parent's spread")
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
