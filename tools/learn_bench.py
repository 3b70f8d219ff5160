"""One learn_variants iteration on eng.aspell, timed by phase (anx_debug_learn_times): strict mode, `--queries` synth.py queries,
max_matches 1.  The device fold (learn.hip, default) and the host fold (ANX_LEARN_FOLD=host) each run on a fresh model; every
phase is printed for both, plus the call's wall time.  Usage: python tools/learn_bench.py [--queries 1000000] [--reps 3]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import analiticcl_amd as A  # noqa: E402
from analiticcl_amd import _lib as L  # noqa: E402
from analiticcl_amd import synth  # noqa: E402


def run(paths, qs, fold: str, reps: int):
    L.set_switch("ANX_LEARN_FOLD", fold)
    p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=1)
    out = []
    for _ in range(reps):
        g = A.VariantModel(paths["alphabet"], A.Weights(), device=0)
        g.read_lexicon(paths["eng"])
        g.build()
        g.learn_variants(qs[:4096], p, auto_build=False)  # warm-up: kernels loaded, pools filled (not timed)
        g = A.VariantModel(paths["alphabet"], A.Weights(), device=0)
        g.read_lexicon(paths["eng"])
        g.build()
        t0 = time.perf_counter()
        count = g.learn_variants(qs, p, auto_build=True)
        wall = (time.perf_counter() - t0) * 1e3
        t = A.VariantModel.learn_times()
        t["wall"] = wall
        t["count"] = count
        out.append(t)
    L.set_switch("ANX_LEARN_FOLD", "device")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    paths = synth.materialize_golden(tempfile.mkdtemp(prefix="anx_learn_bench_"))
    words = synth.load_lexicon_words(paths["eng"])
    qs = synth.make_queries(words, a.queries, max_len=16, seed=1)
    res = {"queries": a.queries, "device": run(paths, qs, "device", a.reps), "host": run(paths, qs, "host", a.reps)}
    keys = ("batch", "device_fold", "host_fold", "host_apply", "build", "upload", "wall")
    print(f"{'fold':8s}" + "".join(f"{k:>13s}" for k in keys) + "   (ms, median of %d)" % a.reps)
    for fold in ("device", "host"):
        med = {k: sorted(r[k] for r in res[fold])[len(res[fold]) // 2] for k in keys}
        print(f"{fold:8s}" + "".join(f"{med[k]:13.2f}" for k in keys))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
