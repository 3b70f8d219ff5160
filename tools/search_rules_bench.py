#!/usr/bin/env python3
"""Search-mode throughput of a model WITH context rules (the device lattice decoder scores them) against the host decoder and the
parent commit, and of the same model without rules as the control.

    search_rules_bench.py [--mb 12.5] [--parent-root build/parent] [--series 2] [--calls 10] [--json OUT]

Workload: the BASELINE configs[4] shape as tools/search_bench.py builds it (eng.aspell, a bigram LM over 5 000 frequent words, running
text of perturbed words, max_ngram 3, max_seq 250) and the fixed rule set below (20 rules over frequent words of that text: every
pattern form, bonus and penalty scores, tags).  Cases, alternating, each series a fresh process: this build, this build under
ANX_LATTICE=host, and -- with --parent-root, a checkout of the parent commit with its library built in place -- the parent through
its own Python package.  Per case and model: best and median MB/s over series x calls calls of anx_find_all_matches_batch (one
warm-up call before); the spread between a build's own best and median is the yardstick for a difference between builds."""
import argparse
import ctypes as C
import hashlib
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

# {k}: the k-th of ten frequent words of the text (common[37 * k]); pattern, score, tags, tag offsets
RULES = [
    ("{0}", 1.1, [], []),
    ("{1}; {2}", 1.3, ["pair"], []),
    ("{3}|{4}|{5}", 0.9, [], []),
    ("?; {6}", 1.05, ["after"], ["1:1"]),
    ("^; {7}", 0.8, [], []),
    ("!{8}; {9}", 1.2, ["neg"], []),
    ("!({0}|{1}); {2}; ?", 1.1, ["tri", "any"], ["0:1", ":"]),
    ("@eng.aspell.lexicon; ^", 0.75, ["oov"], ["1:1"]),
    ("^; ^", 0.6, [], []),
    ("{4}; ?; {5}", 1.4, [], []),
    ("!{6}|{7}; {8}", 1.15, [], []),
    ("{9}; !^", 1.1, ["known"], []),
    ("{2}; {3}; {4}; {5}", 2.0, ["run"], []),
    ("?; ?; ?; {0}", 0.95, [], []),
    ("!@eng.aspell.lexicon", 0.9, [], []),
    ("{1}|{3}|{5}|{7}|{9}; {0}|{2}|{4}|{6}|{8}", 1.25, ["odd", "even"], ["0:1", "1:1"]),
    ("{6}; {6}", 0.5, [], []),
    ("!({7}|{8}|{9}); !({0}|{1}|{2}); {3}", 1.1, [], []),
    ("{5}", 0.97, ["five"], []),
    ("{8}; ?", 1.02, [], []),
]


def workload(mb, tmp):
    import analiticcl_amd as A
    from analiticcl_amd import synth
    d = synth.materialize_golden(os.path.join(tmp, "data"))
    words = synth.load_lexicon_words(d["eng"])
    common = [w for w in words if w.isalpha()][::23][:5000]
    LM = A.VocabParams(vocabtype="LM")
    models = {}
    for name in ("rules", "plain"):
        rng = random.Random(7)
        m = A.VariantModel(d["alphabet"], A.Weights(), device=0)
        m.read_lexicon(d["eng"])
        for _ in range(20000):
            a, b = rng.choice(common), rng.choice(common)
            m.add_to_vocabulary(f"{a} {b}", rng.randrange(1, 20), LM)
        for w in common[:500]:
            m.add_to_vocabulary(f"<bos> {w}", 5, LM)
        m.build()
        if name == "rules":
            hot = [common[37 * k] for k in range(10)]
            for pat, score, tags, offs in RULES:
                m.add_contextrule(pat.format(*hot), score, tags, offs)
        models[name] = m
    rng = random.Random(8)
    pert = synth.make_queries(common, int(mb * 1e6 / 7) + 100, max_len=16, seed=3)
    texts, cur, size, k = [], [], 0, 0
    while size < mb * 1e6:
        n = rng.randrange(5, 26)
        cur.append(" ".join(pert[k:k + n]) + rng.choice([". ", "\n", ", ", "\n\n"]))
        k += n
        if len(cur) == 8:
            texts.append("".join(cur))
            size += len(texts[-1])
            cur = []
    return A, models, texts, size


def child(mb, calls):
    from analiticcl_amd import _lib as L
    with tempfile.TemporaryDirectory() as tmp:
        A, models, texts, size = workload(mb, tmp)
        p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=2, max_matches=10, max_ngram=3)
        spc = p._c_search()
        arr = (C.c_char_p * len(texts))(*[t.encode() for t in texts])
        has_stats = hasattr(A.VariantModel, "search_lattice_stats")
        res = {}
        for name, m in models.items():
            before = A.VariantModel.search_lattice_stats() if has_stats else None
            rates, matches, tagged, digest = [], 0, 0, ""
            for i in range(calls + 1):
                ms, offs, rows, nrows = C.POINTER(L.Match)(), C.POINTER(C.c_size_t)(), C.POINTER(L.Result)(), C.c_size_t(0)
                tags = C.POINTER(L.MatchTag)()
                t = time.perf_counter()
                L.check(L.lib().anx_find_all_matches_batch(m.h, arr, len(texts), C.byref(spc), C.byref(ms), C.byref(offs), C.byref(rows), C.byref(nrows), C.byref(tags)))
                dt = time.perf_counter() - t
                if i == 0:
                    matches = offs[len(texts)]
                    tagged = sum(1 for j in range(matches) if ms[j].tag_end > ms[j].tag_begin) if name == "rules" else 0
                    ntags = max((ms[j].tag_end for j in range(matches)), default=0) if name == "rules" else 0
                    h = hashlib.sha256()  # every byte the call returns: matches, offsets, variant rows, tags
                    for ptr, count, typ in ((ms, matches, L.Match), (offs, len(texts) + 1, C.c_size_t), (rows, nrows.value, L.Result), (tags, ntags, L.MatchTag)):
                        if count:
                            h.update(C.string_at(ptr, count * C.sizeof(typ)))
                    digest = h.hexdigest()
                else:
                    rates.append(size / 1e6 / dt)
                L.lib().anx_matches_free(ms, offs, rows, tags)
            after = A.VariantModel.search_lattice_stats() if has_stats else None
            kernels = None
            if name == "rules":  # one more call with the kernel timer on: the device time of the lattice kernels, the rules' kernel among them
                L.kernel_timer(True)
                ms, offs, rows, nrows = C.POINTER(L.Match)(), C.POINTER(C.c_size_t)(), C.POINTER(L.Result)(), C.c_size_t(0)
                t = time.perf_counter()
                L.check(L.lib().anx_find_all_matches_batch(m.h, arr, len(texts), C.byref(spc), C.byref(ms), C.byref(offs), C.byref(rows), C.byref(nrows), None))
                kernels = {"call_ms": (time.perf_counter() - t) * 1e3}
                L.lib().anx_matches_free(ms, offs, rows, None)
                for k in ("k_lattice", "k_ctx_rules", "k_lattice_lm"):
                    kernels[k] = L.kernel_time(k)[0]
                L.kernel_timer(False)
            res[name] = dict(rates=rates, matches=int(matches), tagged=int(tagged), digest=digest, mb=size / 1e6, kernels=kernels,
                             decoded={k: after[k] - before[k] for k in after} if has_stats else None)
        print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=12.5)
    ap.add_argument("--parent-root")
    ap.add_argument("--series", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--json")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.mb, a.calls)
    me = [sys.executable, os.path.abspath(__file__), "--child", "--mb", str(a.mb), "--calls", str(a.calls)]
    cases = [("this", {}), ("this ANX_LATTICE=host", {"ANX_LATTICE": "host"})]
    if a.parent_root:
        cases.append(("parent", {"ANX_BENCH_ROOT": os.path.abspath(a.parent_root)}))
    runs = {name: [] for name, _ in cases}
    for s in range(a.series):
        for name, env in cases:   # a failing case ends the measurement (nothing more is started on the device)
            r = subprocess.run(me, env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-3000:])
                sys.exit(f"case {name!r} failed with status {r.returncode}")
            runs[name].append(json.loads([x for x in r.stdout.split("\n") if x.startswith("RESULT ")][-1][7:]))
            last = runs[name][-1]
            print(f"series {s} {name}: " + "  ".join(f"{k} median {statistics.median(v['rates']):.1f} MB/s" for k, v in last.items()), flush=True)
    first = runs["this"][0]
    print(f"\n{first['rules']['mb']:.1f} MB of text, {a.series} series x {a.calls} calls per case; rules model: {first['rules']['matches']} matches, "
          f"{first['rules']['tagged']} tagged; lattices of one series: {first['rules']['decoded']}")
    print(f"{'case':24s} {'rules: best':>12s} {'median':>8s} {'spread':>8s} {'plain: best':>12s} {'median':>8s} {'spread':>8s}")
    for name, _ in cases:
        cells = []
        for model in ("rules", "plain"):
            rates = [x for r in runs[name] for x in r[model]["rates"]]
            cells += [f"{max(rates):12.1f}", f"{statistics.median(rates):8.1f}", f"{max(rates) - statistics.median(rates):8.1f}"]
        print(f"{name:24s} " + " ".join(cells))
    if a.parent_root:  # the two criteria: the rules model beats the parent by more than the parent's own best - median spread; the
        # model without rules stays within that spread of the parent's median
        stat = {(n, mdl): [x for r in runs[n] for x in r[mdl]["rates"]] for n, _ in cases for mdl in ("rules", "plain")}
        med = {k: statistics.median(v) for k, v in stat.items()}
        spread = {k: max(v) - statistics.median(v) for k, v in stat.items()}
        gain = med["this", "rules"] - med["parent", "rules"]
        print(f"rules model: this - parent = {gain:+.1f} MB/s median ({med['this', 'rules'] / med['parent', 'rules']:.2f} x), parent's spread {spread['parent', 'rules']:.1f}: "
              + ("margin MET" if gain > spread["parent", "rules"] else "margin NOT met"))
        diff = med["this", "plain"] - med["parent", "plain"]
        print(f"plain model: this - parent = {diff:+.1f} MB/s median, parent's spread {spread['parent', 'plain']:.1f}: "
              + ("within the spread" if abs(diff) <= spread["parent", "plain"] else ("FASTER than the spread" if diff > 0 else "SLOWER than the spread")))
    ks = [r["rules"]["kernels"] for r in runs["this"] if r["rules"].get("kernels")]
    if ks:
        print("rules model, one call with the kernel timer (ms, per series): " + "; ".join(
            f"call {k['call_ms']:.1f}: k_lattice {k['k_lattice']:.2f}, k_ctx_rules {k['k_ctx_rules']:.2f}, k_lattice_lm {k['k_lattice_lm']:.2f}" for k in ks))
    for model in ("rules", "plain"):
        same = all(r[model]["digest"] == first[model]["digest"] for rs in runs.values() for r in rs)
        print(f"{model} model: output bytes (matches, offsets, rows, tags) equal in every case and series: " + ("yes" if same else "NO"))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    main()
