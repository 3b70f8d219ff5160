#!/usr/bin/env python3
"""anx_evaluate_gold against the same answer composed from the entry points that existed before it, on eng.aspell.

    evaluate_bench.py [--pairs 1000000] [--small 10000] [--reps 5] [--procs 2] [--json OUT]

Pairs: (edited query, source word) -- one to three random edits of lexicon words, seeded -- under k = 3, d = 2, n = 10.
  (a) anx_evaluate_gold_packed: two blobs in, 32 bytes per pair out; the ranked rows never leave the device.
  (b) the composition, in the same build: encode_packed + run + fetch_compact(with_via=True) (every ranked row crosses PCIe),
      score_pairs_arrays for the direct pairs, the gold ids through a host dict (built outside the timed region), ranks with numpy
      (first row of an input's segment whose vocabulary id is the gold id) and the reasons RANKED / STATUS / NOT_A_RESULT / EDIT /
      THRESHOLD / CROPPED with numpy.  (b) cannot tell ANAGRAM from EDIT or find EXACT_STOP -- the count vectors and the class
      index are on the device -- so it does LESS than (a) there; it is charged nothing for that.
Every measurement runs in a fresh process, (a) and (b) alternating, --procs processes each, --reps timed calls after one warm-up call;
the packing of the Python lists into blobs is outside the timed region for both (both take packed blobs).  Reported: median and best
per side, the bytes each side downloads, and for (a) the summed time of k_eval_rows, k_eval_classify, k_eval_lookup and the encoder
launch of the pair side (the library's kernel timer, one extra call).  The verdict compares (a)'s median with (b)'s median plus (b)'s own
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


def child(side, n, reps):
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
        qa, qg = [a for a, _ in pairs], [b for _, b in pairs]
        P = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10)
        ba, bg = _pack(qa), _pack(qg)
        cp = P._c()
        res = {"side": side, "pairs": n}
        if side == "a":
            import ctypes as C
            out = np.zeros(n, dtype=np.dtype(A.VariantModel.GOLD_DTYPE))
            optr = out.ctypes.data_as(C.POINTER(L.GoldEval))

            def call():
                L.check(L.lib().anx_evaluate_gold_packed(g.h, ba, len(ba), bg, len(bg), n, C.byref(cp), optr, None))
                return 32 * n
        else:
            ids = {g.vocab_text(v): v for v in range(g.vocab_size())}   # the host map, built once
            indexed = np.array([bool(g.vocabtype(v) & 1) and not g.vocabtype(v) & 4 for v in range(g.vocab_size())])

            def call():
                b = g.encode_packed(ba, n, P)
                b.run()
                off, rec, _via = b.fetch_compact(with_via=True)
                cols = g.score_pairs_arrays(qa, qg)
                gid = np.fromiter((ids.get(t, 0xFFFFFFFF) for t in qg), dtype=np.uint32, count=n)
                cnt = np.diff(off.astype(np.int64))
                hit = rec["vocab_id"] == np.repeat(gid, cnt)
                pos = np.where(hit, np.arange(len(hit)) - np.repeat(off[:-1].astype(np.int64), cnt), 1 << 30)
                rank = np.full(n, 1 << 30, dtype=np.int64)
                nz = cnt > 0
                if len(pos):
                    rank[nz] = np.minimum.reduceat(pos, off[:-1][nz].astype(np.int64))
                ranked = rank < (1 << 30)
                known = gid != 0xFFFFFFFF
                ok = np.zeros(n, dtype=bool)
                ok[known] = indexed[gid[known]]
                d = np.minimum(2, cols["len_a"] // 2)
                reason = np.select([ranked, cols["status"] != 0, ~ok, cols["ld"] > d, cols["score"] < P.score_threshold], [0, 1, 2, 5, 6], 7)
                bytes_down = rec.nbytes + off.nbytes + 4 * len(rec) + 24 * n
                b.free()
                return bytes_down + 0 * int(reason[0])
        call()   # warms the pools (and builds the vocabulary table)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res["bytes_down"] = int(call())
            times.append(time.perf_counter() - t0)
        res["times_ms"] = [t * 1e3 for t in times]
        if side == "a":
            L.kernel_timer(True)
            call()
            res["kernels_ms"] = {k: L.kernel_time(k)[0] for k in ("k_eval_rows", "k_eval_classify", "k_eval_lookup", "k_enc_strings_pairs", "k_pairs_short", "k_pairs_long")}
            L.kernel_timer(False)
            s = A.VariantModel.evaluate_summary(out)
            res["summary"] = {"accuracy_at_1": s["accuracy_at_1"], "mrr": s["mrr"], "reasons": s["reasons"]}
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
        r["kernels_ms"] = runs["a"][0]["kernels_ms"]
        r["summary"] = runs["a"][0]["summary"]
        spread = r["b"]["median_ms"] - r["b"]["best_ms"]
        r["verdict"] = "ok" if r["a"]["median_ms"] <= r["b"]["median_ms"] + spread else "DEFECT: (a) is slower than (b) by more than (b)'s own spread"
        report[str(n)] = r
        print(f"{n} pairs: (a) median {r['a']['median_ms']:.2f} ms (best {r['a']['best_ms']:.2f}), {r['a']['bytes_down'] / 1e6:.2f} MB down; "
              f"(b) median {r['b']['median_ms']:.2f} ms (best {r['b']['best_ms']:.2f}), {r['b']['bytes_down'] / 1e6:.2f} MB down; {r['verdict']}")
        print("   kernels of one call of (a), ms: " + ", ".join(f"{k} {v:.3f}" for k, v in r["kernels_ms"].items()))
        print("   summary: " + json.dumps(r["summary"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
