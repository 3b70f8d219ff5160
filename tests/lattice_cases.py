"""Hand-made lattices for the device lattice decoder by itself (lattice.hip: k_lattice<32|64>, k_ctx_rules, k_lattice_lm and their
driver lattice_launch): the cases tests/test_gpu_lattice_door.py sends through anx_debug_lattice_decode, their reference (oracle/twin.py
decode_lattice) and a census that proves from the lattices and the reference alone which of the kernels' branch classes a set of cases
populates.  TEST INFRASTRUCTURE (no GPU needed here).

A lattice is a dict in the layout of build_lattice_view: nstates (without the virtual end state), in_off [nstates + 2], arcs
[(cost, src, sym | EPS)] per destination in (source state, arc number) order, syms [(vocab_id, boundary)], btok_off [nstates], btok,
best_cost_init.  Parallel arcs between one pair of states are legal (the variants of a segment) and are how three states reach any
in-degree.  A batch = (name, model kind, K, weights, lattices, budgets): one call of the door."""
import ctypes
import ctypes.util
import random
import time

import numpy as np

from oracle import twin as T

EPS = T.LAT_EPS
LAT_MAX_STATES = 1024  # per stretch, virtual end state included
WORDS = ("able acid aged also area army away baby back ball band bank base bath bear beat been beer bell belt best bill bird blow blue "
         "boat body bomb bond bone book boom born boss both bowl bulk burn bush busy call").split()  # 40 lexicon words: ids 3 .. 42
LM_ONLY = ("calm came camp card care case").split()  # LM unigrams that are no lexicon words: ids 43 .. 48


def model_spec(kind):
    """What both sides build, in this order (ids are aligned by insertion order after <bos> <eos> <unk>): lexicon words, then for the
    LM kinds unigrams, bigrams (joint counts below and above the prior), <bos> / <eos> terms and entries of 2, 3, 5 and 6 parts (the
    last has no token list), then for 'rules' four flat rules (one with a score <= 0, two overlapping on a position)."""
    rng = random.Random(20240611)
    lex = [(w, rng.randrange(1, 50)) for w in WORDS]
    lm, rules = [], []
    if kind in ("lm", "rules"):
        lm += [(w, rng.randrange(2, 30)) for w in LM_ONLY]
        pool = list(WORDS[:12]) + list(LM_ONLY)
        seen = set()
        while len(seen) < 60:
            a, b = rng.choice(pool), rng.choice(pool)
            if (a, b) not in seen:
                seen.add((a, b))
                lm.append((f"{a} {b}", rng.randrange(1, 40)))
        lm += [(f"<bos> {w}", 3) for w in pool[:6]] + [(f"{w} <eos>", 2) for w in pool[3:9]]
        lm += [("able acid aged", 4), ("calm came camp", 2), ("also area army away baby", 3), ("able zzz acid", 1),
               ("back ball band bank base bath", 5)]
    if kind == "rules":
        rules = [("able; acid", 1.1, ["t0"], []), ("aged", 0.9, [], []), ("?; also", -3.0, ["t1"], ["1:1"]), ("acid; area", 1.25, [], [])]
    return lex, lm, rules


def twin_model(kind):
    m = T.SearchModel(T.TEST_ALPHABET)
    lex, lm, rules = model_spec(kind)
    for w, f in lex:
        m.add_to_vocabulary(w, f)
    for t, f in lm:
        m.add_lm(t, f)
    m.build()
    for pat, score, tag, offs in rules:
        m.add_contextrule(pat, score, tag, offs)
    return m


def libm_logf():
    """The C library's logf, which the product's bigram terms are computed with (numpy's float32 log need not round alike)."""
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lib.logf.restype = ctypes.c_float
    lib.logf.argtypes = [ctypes.c_float]
    return lambda x: np.float32(lib.logf(float(x)))


class Params:  # what decode_lattice reads of the twin's SearchParams
    def __init__(self, K, lm_weight=1.0, variantmodel_weight=3.0, contextrules_weight=1.0):
        self.max_seq, self.lm_weight, self.variantmodel_weight, self.contextrules_weight = K, lm_weight, variantmodel_weight, contextrules_weight


# ---- lattice builders -------------------------------------------------------------------------------------------------------------------
def make(nstates, incoming, syms, btoks=None, best_cost_init=None):
    """incoming[d] = [(cost, src, sym)] for d = 1 .. nstates (nstates = the virtual end state); sorted here by source (stable)."""
    in_off, arcs = [0, 0], []
    for d in range(1, nstates + 1):
        arcs.extend(sorted(incoming.get(d, []), key=lambda a: a[1]))
        in_off.append(len(arcs))
    btoks = btoks or [[] for _ in range(nstates - 1)]
    btok_off, btok = [], []
    for b in btoks:
        btok_off.append(len(btok))
        btok.extend(b)
    btok_off.append(len(btok))
    return dict(nstates=nstates, in_off=in_off, arcs=[(np.float32(c), s, y) for c, s, y in arcs], syms=list(syms), btok_off=btok_off, btok=btok,
                best_cost_init=np.float32(max(nstates - 2, 0) * 2.0 if best_cost_init is None else best_cost_init))


class Gen:
    def __init__(self, seed, nvocab, ntok, costs=(0.0, 1.0, 1.5, 2.0)):
        self.rng, self.nvocab, self.ntok, self.costs = random.Random(seed), nvocab, ntok, costs

    def cost(self):
        c = self.rng.choice(self.costs)
        return self.rng.random() * 3 if c is None else c

    def sym(self, syms, d, nstates, vid=None):
        """a new symbol behind boundary d - 1 (arcs into the end state carry none)"""
        if d >= nstates:
            return EPS
        syms.append((self.rng.randrange(0, self.nvocab) if vid is None else vid, d - 1))
        return len(syms) - 1

    def btoks(self, nstates, p=0.4, maxlen=3):
        r = self.rng
        return [[r.choice([-1] + list(range(3, self.ntok))) for _ in range(r.randrange(1, maxlen + 1))] if r.random() < p else [] for _ in range(nstates - 1)]

    def fan(self, degs, end_deg=1, eps_p=0.1, best_cost_init=None, btoks=None):
        """len(degs) + 1 states in a chain, degs[i] parallel arcs from state i to i + 1, end_deg arcs from the last state to the end"""
        nstates = len(degs) + 1
        syms, inc = [], {}
        for i, D in enumerate(degs):
            inc[i + 1] = [(self.cost(), i, EPS if self.rng.random() < eps_p else self.sym(syms, i + 1, nstates)) for _ in range(D)]
        inc[nstates] = [(0.0 if k == 0 else self.cost(), nstates - 1, EPS) for k in range(end_deg)]
        return make(nstates, inc, syms, self.btoks(nstates) if btoks is None else btoks, best_cost_init)

    def dag(self, nstates, max_span, deg, finals=1, unreachable=(), chain=True, best_cost_init=None):
        """random arcs of span <= max_span, about `deg` per state; `chain`: an epsilon arc of cost 100 from every state to the next;
        states in `unreachable` get no incoming arc at all"""
        r = self.rng
        syms, inc = [], {}
        for d in range(1, nstates):
            if d in unreachable:
                continue
            arcs = [(100.0, d - 1, EPS)] if chain else []
            for _ in range(r.randrange(1, deg + 1)):
                src = max(0, d - r.randrange(1, max_span + 1))
                arcs.append((self.cost(), src, self.sym(syms, d, nstates)))
            inc[d] = arcs
        inc[nstates] = [(0.0, nstates - 1 - k, EPS) for k in range(min(finals, nstates))]
        return make(nstates, inc, syms, self.btoks(nstates), best_cost_init)

    def spanning(self, nstates, span):
        """a chain whose widest arc spans exactly `span` states (ring = span + 1): d % ring wraps nstates / ring times"""
        r = self.rng
        syms, inc = [], {}
        for d in range(1, nstates):
            arcs = [(self.cost(), d - 1, self.sym(syms, d, nstates))]
            if d >= span:
                arcs.append((self.cost(), d - span, self.sym(syms, d, nstates)))
            if d >= 2 and r.random() < 0.5:
                arcs.append((self.cost(), d - r.randrange(1, min(d, span) + 1), self.sym(syms, d, nstates)))
            inc[d] = arcs
        inc[nstates] = [(0.0, nstates - 1, EPS)]
        return make(nstates, inc, syms, self.btoks(nstates))


# ---- the documented limits (lattice.hip lattice_launch) ---------------------------------------------------------------
def ring_caps(K, lds_limit):
    """ring_cap = max(3, budget / 4K) - 1 with a budget of 48 KB (one stretch per wave) / 24 KB (two), then shrunk until the block's
    dynamic LDS -- (64 / lanes) * ((ring + 1) * K * 4 + 1024 * 2) bytes -- is within the device's limit; 0 = the kernel takes nothing."""
    caps = []
    for lanes, budget in ((64, 48 << 10), (32, 24 << 10)):
        cap = max(3, budget // (4 * K)) - 1
        while cap > 0 and (64 // lanes) * ((cap + 1) * K * 4 + LAT_MAX_STATES * 2) > lds_limit:
            cap -= 1
        caps.append(cap)
    return caps[0], caps[1]  # (wide, narrow)


def ring_of(lat):
    ns, io = lat["nstates"], lat["in_off"]
    return 1 + max([d - lat["arcs"][k][1] for d in range(1, ns + 1) for k in range(io[d], io[d + 1])] + [0])


def maxdeg_of(lat):
    io = lat["in_off"]
    return max(io[d + 1] - io[d] for d in range(1, lat["nstates"] + 1))


def plan(lattices, K, lds_limit, budget_nodes=0, rules=False):
    """Which kernel takes every stretch, or why it is handed back, which launch, and the narrow kernel's pairs: narrow = in-degree <= 64
    and ring <= the narrow cap, by decreasing nstates (stable), two per wave; then the wide ones, one per wave; a launch holds
    stretches of one kind and at most budget_nodes nodes ((nstates + 1) * K per stretch), but always at least one stretch."""
    n = len(lattices)
    if K > 4096:
        return dict(kernel=[None] * n, why=["K"] * n, launch=[None] * n, pairs=[], n_launches=0)
    cap64, cap32 = ring_caps(K, lds_limit)
    budget = budget_nodes or (6 << 30) // (12 + (8 if rules else 0))
    narrow = [j for j in range(n) if maxdeg_of(lattices[j]) <= 64 and ring_of(lattices[j]) <= cap32]
    wide = [j for j in range(n) if j not in set(narrow)]
    narrow.sort(key=lambda j: -lattices[j]["nstates"])
    kernel, why, launch, pairs = [None] * n, [None] * n, [None] * n, []
    nl = 0
    for kind, lst in ((32, narrow), (64, wide)):
        i = 0
        while i < len(lst):
            used, j = 0, i
            while j < len(lst):
                need = (lattices[lst[j]]["nstates"] + 1) * K
                if j > i and used + need > budget:
                    break
                used += need
                j += 1
            for k in range(i, j):
                kernel[lst[k]], launch[lst[k]] = kind, nl
            if kind == 32:
                pairs += [tuple(lst[k:min(k + 2, j)]) for k in range(i, j, 2)]
            nl += 1
            i = j
    for j, lat in enumerate(lattices):
        if lat["nstates"] + 1 > LAT_MAX_STATES:
            why[j] = "states"
        elif maxdeg_of(lat) > 128:
            why[j] = "indegree"
        elif kernel[j] == 64 and ring_of(lat) > cap64:
            why[j] = "ring"
    return dict(kernel=kernel, why=why, launch=launch, pairs=pairs, n_launches=nl)


# ---- the reference, once per (model, lattice, parameters) --------------------------------------------------------------------------------
REF_SECONDS = [0.0]


def reference(model, lat, P, ln=None, logf=None):
    t0 = time.time()
    res = model.decode_lattice(lat, P.max_seq, P, ln=ln, logf=logf)
    REF_SECONDS[0] += time.time() - t0
    return res


# ---- census ---------------------------------------------------------------------------------------------------------------------------
def deg_class(D):
    for lo, hi, name in ((0, 0, "0"), (1, 1, "1"), (2, 31, "2-31"), (32, 32, "32"), (33, 63, "33-63"), (64, 64, "64"), (65, 127, "65-127"), (128, 128, "128")):
        if lo <= D <= hi:
            return name
    return ">128"


def census_state(lat, ref, K, d, G):
    """classes of the merge into state d as the kernel of G lanes per stretch runs it"""
    io, arcs, nodes = lat["in_off"], lat["arcs"], ref["nodes"]
    out = set()
    a0, D = io[d], io[d + 1] - io[d]
    lists = [len(nodes[arcs[a0 + k][1]]) for k in range(D)]
    total = sum(lists)
    out.add("count<K" if total < K else "count==K" if total == K else "count>K")
    if D and total == 0:
        out.add("sources-empty")
    if D == 0:
        out.add("no-arc")
    if any(n == 1 for n in lists):
        out.add("list-of-one")
    taken = {}
    last_pop = {}
    # the pops in order: (cost, arc, rank) of every node of the state
    cc = [[float(np.float32(nd[0] + arcs[a0 + k][0])) for nd in nodes[arcs[a0 + k][1]]] for k in range(D)]
    cands = sorted((cc[k][r], k, r) for k in range(D) for r in range(lists[k]))
    pops = cands[:K]
    for it, (c, k, r) in enumerate(pops):
        taken[k] = taken.get(k, 0) + 1
        last_pop[k] = it
        if it and pops[it - 1][1] == k and pops[it - 1][0] == c:
            out.add("same-arc-consecutive-equal")
        if float(arcs[a0 + k][0]) == 0.0:
            out.add("zero-cost-arc")
    if any(taken.get(k, 0) == lists[k] and lists[k] and last_pop[k] < len(pops) - 1 for k in range(D)):
        out.add("list-exhausted-mid-merge")
    # ties among the heads at a pop: the heads are, per arc, its next candidate
    heads = {k: 0 for k in range(D) if lists[k]}
    for c, k, r in pops:
        eq = [k2 for k2, r2 in heads.items() if r2 < lists[k2] and cc[k2][r2] == c]
        if len(eq) > 1:
            first, second = [x for x in eq if x < G], [x for x in eq if x >= G]
            if len(first) > 1:
                out.add("tie-first-heads")
            if first and second:
                out.add("tie-first-vs-second" + ("-lower-lane-second" if min(x - G for x in second) < min(first) else "-lower-lane-first"))
            if len(second) > 1 and not first:
                out.add("tie-second-heads")
        heads[k] = r + 1
    if len(set(c for c, _k, _r in cands)) == 1 and len(cands) > 1:
        out.add("all-equal")
    return out


def token_class(model, lat, s):
    vid, b = lat["syms"][s]
    bt = lat["btok"][lat["btok_off"][b]:lat["btok_off"][b + 1]]
    toks = model.symbol_tokens(vid, [None if t < 0 else t for t in bt])
    n = len(toks)
    c = {"tok-%s" % ("0" if n == 0 else str(n) if n in (1, 2, 5, 6, 7) else "3-4" if n < 5 else ">7")}
    if vid == 0:
        c.add("oov-with-boundary" if bt else "oov-bare")
    if any(t == -1 for t in bt):
        c.add("btok-minus-one")
    return c


def census(model, batch, refs, lds_limit):
    """every class a batch populates; refs[j] = reference of lattice j (None where the plan hands the stretch back before decoding)"""
    name, kind, P, lattices, budgets = batch
    K = max(1, P.max_seq)
    out = set()
    use_lm = model.have_lm and P.lm_weight > 0
    for budget in budgets:
        pl = plan(lattices, K, lds_limit, budget, bool(model.context_rules))
        if budget and pl["n_launches"] > 1:
            kinds = [sum(1 for l in set(pl["launch"]) if l is not None and any(pl["launch"][j] == l and pl["kernel"][j] == w for j in range(len(lattices)))) for w in (32, 64)]
            for w, c in zip((32, 64), kinds):
                if c >= 2:
                    out.add("launches-%d-%s" % (w, "2" if c == 2 else "3+"))
            if any((lat["nstates"] + 1) * K > budget for lat in lattices):
                out.add("stretch-above-budget")
        if budget:
            continue
        for j, lat in enumerate(lattices):
            out.add("kernel-%s" % pl["kernel"][j] if pl["why"][j] is None else "handed-back-" + pl["why"][j])
        for pr in pl["pairs"]:
            if len(pr) == 1:
                out.add("pair-odd-half-empty")
                continue
            x, y = pr
            dead = [pl["why"][x] is not None, pl["why"][y] is not None]
            if dead[0] != dead[1]:
                out.add("pair-one-handed-back")
            two = [any(lattices[q]["in_off"][d + 1] - lattices[q]["in_off"][d] > 32 for d in range(1, lattices[q]["nstates"] + 1)) for q in pr]
            if two[0] != two[1] and not any(dead):
                out.add("pair-TWO-one-side")
            if not any(dead):
                if abs(lattices[x]["nstates"] - lattices[y]["nstates"]) > 500:
                    out.add("pair-2-vs-1023-states")
                pops = [sum(len(s) for s in refs[q]["nodes"][1:]) for q in pr]
                if max(pops) > 4 * max(1, min(pops)):
                    out.add("pair-surplus-pops")
        if len(set(k for k in pl["kernel"] if k)) == 2:
            out.add("mixed-wide-narrow")
    pl = plan(lattices, K, lds_limit, 0, bool(model.context_rules))
    for j, lat in enumerate(lattices):
        ref = refs[j]
        if ref is None or pl["why"][j] is not None:
            continue
        G = pl["kernel"][j]
        ns = lat["nstates"]
        for d in range(1, ns + 1):
            D = lat["in_off"][d + 1] - lat["in_off"][d]
            out.add("indeg-" + deg_class(D) + ("-end" if d == ns else ""))
            out |= census_state(lat, ref, K, d, G)
        out.add("ring==cap" if ring_of(lat) == (ring_caps(K, lds_limit)[0] if G == 64 else ring_caps(K, lds_limit)[1]) else "ring<cap")
        if ns > 3 * ring_of(lat):
            out.add("ring-wraps")
        npaths = len(ref["nodes"][ns])
        out.add("npaths-0" if npaths == 0 else "npaths-1" if npaths == 1 else "npaths<=32" if npaths <= 32 else "npaths<=64" if npaths <= 64 else "npaths<=250" if npaths <= 250 else "npaths>250")
        if npaths == 0:
            continue
        bci = float(lat["best_cost_init"])
        costs = [float(nd[0]) for nd in ref["nodes"][ns]]
        out.add("best_cost_init-0" if bci == 0.0 else "best_cost_init-below" if bci < min(costs) else "best_cost_init-above" if bci > max(costs) else "best_cost_init-between")
        sc = ref["scores"]
        if sc[0] != sc[0]:
            out.add("nan-path-0")
        elif any(s != s for s in sc):
            out.add("nan-later-path")
        out.add("chosen-0" if ref["chosen"] == 0 else "chosen-later")
        if use_lm:
            for s in set(sym for st in ref["nodes"] for _c, _p, sym in st if sym != EPS):
                out |= token_class(model, lat, s)
        if model.context_rules:
            out.add("rule-covers-chosen" if any(c is not None for c in ref["out_cover"]) else "rule-none-on-chosen")
            for cov in ref["covers"]:
                fired = set(c >> 8 for c in cov if c is not None)
                out |= set("rule-%d-fired" % r for r in fired)
                out.add("rule-none-found" if not fired else "rules-%d-on-a-path" % min(len(fired), 2))
    return out


# ---- the batches ------------------------------------------------------------------------------------------------------------------------
NLEX = 3 + len(WORDS)            # vocabulary ids every model kind has
NLM = NLEX + len(LM_ONLY)        # LM kinds: + the LM-only unigrams
MULTI0 = NLM + 60 + 12           # behind the bigrams and the <bos> / <eos> entries: the entries of 3, 3, 5, 3 (one unknown) and 6 parts
WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129)


def batches(lds_limit):
    """(name, model kind, Params, lattices, budgets): budgets = node budgets per launch the batch is also run under (0 = the driver's)."""
    out = []
    lm_vocab = MULTI0 + 5  # the LM kinds' vocabulary size
    # widths: fans of in-degree D, D' at states 1 and 2, K = 8 and 250
    for K in (8, 250):
        g = Gen(100 + K, NLEX, NLM)
        lats = [g.fan([D, D2]) for D, D2 in zip(WIDTHS, WIDTHS[3:] + WIDTHS[:3])]
        lats += [g.fan([3, 2], end_deg=E) for E in ((33, 65, 128) if K == 8 else (2,))]
        out.append(("widths-K%d" % K, "lm", Params(K), lats, (0, 100) if K == 8 else (0,)))  # (100 nodes: three wide stretches a launch)
    # ties: all-equal costs, 0-cost arcs, first against second heads in both lane orders
    for K in (1, 2, 3, 4, 5, 251):
        g = Gen(200 + K, NLEX, NLEX, costs=(1.0,) if K % 2 else (0.0, 1.0, 1.5, 2.0))
        lats = [g.fan([5, 40]), g.fan([33, 70]), g.fan([1, 1]), g.fan([64, 3]), g.dag(9, 3, 4)]
        # a first head and a second head with the same cost: the second head's lane below / above the first head's
        sy = [(5, 1), (6, 1), (7, 0)]
        for lane_first, lane_second in ((20, 3), (3, 20)):
            inc = {1: [(1.0, 0, 2)], 2: [(2.0 if k not in (lane_first, 32 + lane_second) else 1.0, 1, k % 2) for k in range(60)], 3: [(0.0, 2, EPS)]}
            lats.append(make(3, inc, sy))
        out.append(("ties-K%d" % K, "nolm", Params(K), lats, (0,)))
    # big K on 64 x 64 fans; 4097 hands everything back
    for K in (1000, 2048, 2049, 4096, 4097):
        g = Gen(300 + K, NLEX, NLEX, costs=(None,))
        out.append(("bigK-%d" % K, "nolm", Params(K), [g.fan([64, 64]), g.fan([3, 2])], (0,)))
    # ring: K = 250, spans at the caps
    cap64, cap32 = ring_caps(250, lds_limit)
    g = Gen(400, NLEX, NLM)
    lats = [g.spanning(s + 6, s) for s in (cap32 - 2, cap32 - 1, cap32, cap64 - 2, cap64 - 1, cap64)] + [g.spanning(40, 3), g.spanning(40, 7)]
    out.append(("ring-K250", "lm", Params(250), lats, (0,)))
    # states at the cap, K = 4, partners of 2 and 1023 states, odd counts, hand-backs beside decoded ones, TWO on one side
    g = Gen(500, NLEX, NLM)
    big = [g.dag(n, 2, 2) for n in (1022, 1023, 1024)]
    small = [g.fan([2]), g.fan([40, 3]), g.dag(6, 3, 3), g.fan([3, 3, 3]), g.dag(12, 4, 50)]
    for cnt, lats in ((1, small[:1]), (2, small[:2]), (3, small[:3]), (7, small + [g.fan([70, 2]), g.fan([129, 1])]), (5, big + small[:2])):
        P = Params(4)
        total = sum((l["nstates"] + 1) * 4 for l in lats)
        out.append(("pairing-%d" % cnt, "lm", P, lats, (0, total // 2 + 1, total // 3 + 1, 8)))
    # unreachable states, sources all empty, the end state unreachable
    g = Gen(600, NLEX, NLM)
    u1 = g.dag(8, 2, 3, unreachable=(3,), chain=False)
    u2 = make(5, {1: [(1.0, 0, 0)], 3: [(1.0, 2, 1)], 4: [(1.0, 3, 2), (2.0, 1, 3)], 5: [(0.0, 4, EPS)]}, [(4, 0), (5, 2), (6, 3), (7, 3)])
    u3 = make(4, {1: [(1.0, 0, 0)], 2: [(1.0, 1, 1)], 4: [(0.0, 3, EPS)]}, [(4, 0), (5, 1)])
    u4 = make(1, {}, [], [])
    out.append(("unreachable", "lm", Params(8), [u1, u2, u3, u4, g.fan([2, 2])], (0, 40)))
    # LM: symbols of 1, 2, 5, 6, 7 tokens; OOV with and without boundary tokens; lm_weight 0
    for lw in (1.0, 0.0):
        g = Gen(700, lm_vocab, NLM)
        lats = []
        for vid, bt in ((4, []), (4, [5]), (MULTI0 + 2, []), (MULTI0 + 2, [6]), (MULTI0 + 2, [6, -1]), (MULTI0, [7, 8, 9, 10]), (0, []), (0, [5, -1]),
                        (MULTI0 + 4, []), (MULTI0 + 1, [43, 44]), (MULTI0 + 3, [])):
            sy = [(vid, 0), (5, 0), (43, 1), (44, 1)]
            inc = {1: [(1.0, 0, 0), (1.5, 0, 1)], 2: [(1.0, 1, 2), (1.0, 1, 3), (3.0, 0, 1)], 3: [(0.0, 2, EPS)]}
            lats.append(make(3, inc, sy, [bt, [3]]))
        lats += [g.dag(10, 3, 6) for _ in range(4)]
        out.append(("lm-tokens-lw%g" % lw, "lm", Params(16, lm_weight=lw), lats, (0,)))
    # rules: > 64 and > 250 final paths, overlapping rules, NaN scores, contextrules_weight 0, best_cost_init classes
    able, acid, aged, also, area = 3, 4, 5, 6, 7
    for cw, K in ((1.0, 300), (0.0, 80), (1.0, 8)):
        g = Gen(800 + K, 12, 12)  # few distinct words: the rules fire
        lats = [g.dag(7, 3, 5, best_cost_init=b) for b in (0.0, 0.25, 1000.0)] + [g.fan([20, 20]), g.fan([4, 4, 5])]
        # path 0 = (any, also): the rule with the score -0.5 -> ctx < 0 -> a NaN; and a lattice where only a later path has it
        sy = [(able, 0), (also, 1), (acid, 1), (area, 1)]
        lats.append(make(3, {1: [(1.0, 0, 0)], 2: [(1.0, 1, 1), (1.5, 1, 2)], 3: [(0.0, 2, EPS)]}, sy))
        lats.append(make(3, {1: [(1.0, 0, 0)], 2: [(1.5, 1, 1), (1.0, 1, 2), (1.2, 1, 3)], 3: [(0.0, 2, EPS)]}, sy))
        out.append(("rules-cw%g-K%d" % (cw, K), "rules", Params(K, contextrules_weight=cw), lats, (0, 4 * K)))
    # random part
    for seed in range(3):
        r = random.Random(900 + seed)
        kind = ("lm", "rules", "nolm")[seed]
        g = Gen(900 + seed, NLEX if kind != "rules" else 14, NLM if kind != "nolm" else NLEX, costs=(0.0, 1.0, 1.5, 2.0, None, None))
        lats = []
        for _ in range(12):
            t = r.randrange(3)
            lats.append(g.dag(r.randrange(2, 30), r.randrange(1, 6), r.randrange(1, 8), finals=r.randrange(1, 3), chain=r.random() < 0.7) if t == 0 else
                        g.fan([r.choice(WIDTHS[:-1]) for _ in range(r.randrange(1, 4))], end_deg=r.randrange(1, 4)) if t == 1 else g.spanning(r.randrange(8, 40), r.randrange(2, 7)))
        K = r.choice((7, 33, 64))
        total = sum((l["nstates"] + 1) * K for l in lats)
        out.append(("random-%d" % seed, kind, Params(K), lats, (0, total // 3 + 1)))
    return out


def subranges(n):
    """(first, count) in the middle and at the end of a view of n lattices"""
    return [(n // 3, max(1, n // 3)), (n - max(1, n // 2), max(1, n // 2))] if n >= 3 else []


# every class the batches populate, under a 64 KB and under a 160 KB LDS limit alike (tests/test_lattice_cases_cpu.py)
EXPECTED_CLASSES = (
    "all-equal best_cost_init-0 best_cost_init-above best_cost_init-below best_cost_init-between btok-minus-one chosen-0 chosen-later "
    "count<K count==K count>K handed-back-K handed-back-indegree handed-back-ring handed-back-states indeg-0 indeg-0-end indeg-1 "
    "indeg-1-end indeg-128 indeg-128-end indeg-2-31 indeg-2-31-end indeg-32 indeg-33-63 indeg-33-63-end indeg-64 indeg-65-127 "
    "indeg-65-127-end kernel-32 kernel-64 launches-32-2 launches-32-3+ launches-64-2 launches-64-3+ list-exhausted-mid-merge list-of-one "
    "mixed-wide-narrow nan-later-path nan-path-0 no-arc npaths-0 npaths-1 npaths<=250 npaths<=32 npaths<=64 npaths>250 oov-bare "
    "oov-with-boundary pair-2-vs-1023-states pair-TWO-one-side pair-odd-half-empty pair-one-handed-back pair-surplus-pops ring-wraps "
    "ring<cap ring==cap rule-0-fired rule-1-fired rule-2-fired rule-3-fired rule-covers-chosen rule-none-found rule-none-on-chosen "
    "rules-1-on-a-path rules-2-on-a-path same-arc-consecutive-equal sources-empty stretch-above-budget tie-first-heads "
    "tie-first-vs-second-lower-lane-first tie-first-vs-second-lower-lane-second tie-second-heads tok-0 tok-1 tok-2 tok-3-4 tok-5 tok-6 "
    "tok-7 zero-cost-arc").split()
# classes the code has that no accepted input reaches, and why:
UNREACHABLE = {
    "k_ctx_rules-path-longer-than-states": "a path enters a state at most once (src < dst is validated), so n + 1 >= ns never holds",
    "K>65535": "lattice_decode hands everything back above K = 4096 before a kernel could see it",
    "ring==0": "the door computes the ring itself: at least 1",
}
