"""Search mode's lattice decoder (lattice.hip: k_lattice<32|64>, k_ctx_rules, k_lattice_lm, lattice_launch) by itself, through the test
hook anx_debug_lattice_decode, on the hand-made lattices of tests/lattice_cases.py against oracle/twin.py decode_lattice.  Everything the
kernels leave in HBM is compared with ==: the per-state counts, every node's (cost bits, parent, symbol), the mark set and every marked
node's (lp bits, n, prev), the bits of ctxval, out_n / out_syms / out_cover, and the fill wherever the reference has nothing -- no
tolerance anywhere (the reference takes the product's logarithm from anx_debug_portable_log and the C library's logf for the bigram
terms; the one latitude: a NaN equals a NaN whatever its sign and payload).  Which stretches come back undecoded, which kernel width and
which launch took each, is predicted from the documented limits (lattice_cases.plan), not read from the driver."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import synth
from oracle import cwrap as O
from oracle import twin as T

import lattice_cases as LC
from search_common import TwinOverOracle

TSV = "\n".join(f"{c}\t{c.upper()}" for c in "abcdefghijklmnopqrstuvwxyz") + "\n.\t,\n"
LMV = A.VocabParams(vocabtype="LM")
FILL = 0xFFFFFFFF
NAMES = [b[0] for b in LC.batches(1 << 16)]  # (the names do not depend on the LDS limit; the ring batch's lattices do)


def gpu_model(kind):
    g = A.VariantModel("", alphabet_text=TSV, device=0)
    lex, lm, rules = LC.model_spec(kind)
    for w, f in lex:
        g.add_to_vocabulary(w, f)
    for t, f in lm:
        g.add_to_vocabulary(t, f, LMV)
    g.build()
    for pat, score, tag, offs in rules:
        g.add_contextrule(pat, score, tag, offs)
    return g


def gparams(P):
    return A.SearchParameters(max_seq=P.max_seq, lm_weight=P.lm_weight, variantmodel_weight=P.variantmodel_weight, contextrules_weight=P.contextrules_weight)


class World:
    def __init__(self):
        self.gpu = {k: gpu_model(k) for k in ("lm", "rules", "nolm")}
        self.twin = {k: LC.twin_model(k) for k in ("lm", "rules", "nolm")}
        self.logf = LC.libm_logf()
        self.ln = lambda x: float(A.VariantModel.portable_log([x])[0])
        tiny = LC.make(1, {1: [(0.0, 0, LC.EPS)]}, [], [])
        self.lds_limit = self.gpu["nolm"].debug_lattice_decode(gparams(LC.Params(1)), [tiny])["lds_limit"]
        self.batches = {b[0]: b for b in LC.batches(self.lds_limit)}
        self.refs = {}

    def ref(self, name):
        """the reference of every lattice of a batch the limits do not hand back, once"""
        if name not in self.refs:
            _n, kind, P, lats, _b = self.batches[name]
            pl = LC.plan(lats, max(1, P.max_seq), self.lds_limit, 0, kind == "rules")
            self.refs[name] = [LC.reference(self.twin[kind], l, P, ln=self.ln, logf=self.logf) if pl["why"][j] is None else None for j, l in enumerate(lats)]
        return self.refs[name]


@pytest.fixture(scope="module")
def world():
    return World()


def canon(a):
    """float64 bits with one pattern for every NaN"""
    a = np.array(a, dtype=np.float64)
    bits = a.view(np.uint64).copy()
    bits[np.isnan(a)] = 0x7FF8000000000000
    return bits


def check(world, kind, P, lats, refs, res, budget, what):
    """everything one door call left, against the references of its lattices"""
    model = world.twin[kind]
    K = max(1, P.max_seq)
    MK = (K + 3) & ~3
    rules, use_lm = bool(model.context_rules), model.have_lm and P.lm_weight > 0
    pl = LC.plan(lats, K, world.lds_limit, budget, rules)
    assert res["n_launches"] == pl["n_launches"], what
    assert len(res["stretches"]) == len(lats), what
    for j, lat in enumerate(lats):
        w = (what, j)
        ref, got, ns = refs[j], res["stretches"][j], lat["nstates"]
        handed = pl["why"][j] is not None or len(ref["nodes"][ns]) == 0  # beyond a documented limit, or no path reaches the end state
        assert (res["out_n"][j] == FILL) == handed, w
        if K > 4096:  # nothing was launched
            assert got["launch"] == FILL and np.all(got["cnts"] == 0xFFFF), w
            continue
        assert (got["launch"], got["width"]) == (pl["launch"][j], pl["kernel"][j]), w
        assert got["lds"] <= world.lds_limit, w
        if pl["why"][j] is not None:  # k_lattice wrote nothing of it
            assert np.all(got["cnts"] == 0xFFFF) and np.all(got["nodes"] == FILL) and np.all(res["out_syms"][j] == FILL), w
            continue
        npaths = len(ref["nodes"][ns])
        assert list(got["cnts"]) == [len(s) for s in ref["nodes"]], w
        exp = np.full((ns + 1, K, 3), FILL, dtype=np.uint32)
        for d, st in enumerate(ref["nodes"]):
            if st:
                exp[d, :len(st), 0] = np.array([c for c, _p, _s in st], dtype=np.float32).view(np.uint32)
                exp[d, :len(st), 1] = [p for _c, p, _s in st]
                exp[d, :len(st), 2] = [s for _c, _p, s in st]
        assert np.array_equal(got["nodes"], exp), (w, "nodes", np.argwhere(got["nodes"] != exp)[:4])
        elm, emk = np.full((ns + 1, K, 3), FILL, dtype=np.uint32), np.full((ns + 1, MK), 0xFF, dtype=np.uint8)
        if use_lm:
            elm[0, 0] = (0, 0, 0)  # the start node: <bos>, nothing summed
            if npaths:
                emk[:] = 0
                for (d, r) in ref["marked"]:
                    emk[d, r] = 1
                    lp, n, prev = ref["lm"][(d, r)]
                    elm[d, r] = (int(np.array([lp], dtype=np.float32).view(np.uint32)[0]), n, FILL if prev is None else prev)
        assert np.array_equal(got["marks"], emk), (w, "marks", np.argwhere(got["marks"] != emk)[:4])
        assert np.array_equal(got["lm"], elm), (w, "lm", np.argwhere(got["lm"] != elm)[:4])
        ectx = np.full(K, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        gctx = got["ctxval"].copy()
        if rules and npaths:
            ectx[:npaths] = canon(ref["ctxval"])
            gctx[:npaths] = canon(gctx[:npaths].view(np.float64))
        assert np.array_equal(gctx, ectx), (w, "ctxval")
        eo, ec = np.full(ns, FILL, dtype=np.uint32), np.full(ns, FILL, dtype=np.uint32)
        if npaths:
            n = len(ref["out_syms"])
            assert res["out_n"][j] == n, (w, "chosen path", ref["chosen"])
            eo[:n] = ref["out_syms"]
            if rules:
                ec[:n] = [FILL if c is None else c for c in ref["out_cover"]]
        assert np.array_equal(res["out_syms"][j], eo), (w, "out_syms", ref["chosen"])
        assert np.array_equal(res["out_cover"][j], ec), (w, "out_cover")


@pytest.mark.parametrize("name", NAMES)
def test_batch_equals_reference(world, name):
    """one launch set, the split budgets and the sub-ranges of a batch: identical results, each equal to the reference"""
    _n, kind, P, lats, budgets = world.batches[name]
    refs = world.ref(name)
    g = world.gpu[kind]
    for budget in budgets:
        res = g.debug_lattice_decode(gparams(P), lats, budget_nodes=budget)
        check(world, kind, P, lats, refs, res, budget, (name, "budget", budget))
    for first, count in LC.subranges(len(lats)):
        res = g.debug_lattice_decode(gparams(P), lats, first=first, count=count)
        assert np.all(res["out_n"][:first] == FILL) and np.all(res["out_n"][first + count:] == FILL), (name, first, count)
        for j in list(range(first)) + list(range(first + count, len(lats))):
            assert np.all(res["out_syms"][j] == FILL) and np.all(res["out_cover"][j] == FILL)
        sub = dict(res, out_n=res["out_n"][first:first + count], out_syms=res["out_syms"][first:first + count], out_cover=res["out_cover"][first:first + count])
        check(world, kind, P, lats[first:first + count], refs[first:first + count], sub, 0, (name, "sub-range", first, count))


def test_census_on_this_device(world):
    """the classes the batches populate under THIS device's LDS limit (tests/test_lattice_cases_cpu.py pins them for 64 KB and 160 KB)"""
    got = set()
    for name in NAMES:
        b = world.batches[name]
        got |= LC.census(world.twin[b[1]], b, world.ref(name), world.lds_limit)
    assert not (set(LC.EXPECTED_CLASSES) - got), sorted(set(LC.EXPECTED_CLASSES) - got)


def test_lds_request_of_the_narrow_kernel_above_k_2048(world):
    """2 x (3 x K x 4 + 2 x states) bytes is what the narrow kernel's floor of three lists asks for above K = 2048.
    Where that exceeds the device's limit the stretch must have gone to the wide kernel; either way what was launched fits."""
    for K in (2049, 4096):
        _n, kind, P, lats, _b = world.batches["bigK-%d" % K]
        res = world.gpu[kind].debug_lattice_decode(gparams(P), lats)
        for lat, st in zip(lats, res["stretches"]):
            narrow_request = 2 * (3 * K * 4 + 2 * ((lat["nstates"] + 2) & ~1))
            print("K", K, "narrow request", narrow_request, "limit", res["lds_limit"], "took", st["width"], "with", st["lds"], "bytes")
            assert st["lds"] <= res["lds_limit"]
            assert st["width"] == (32 if 2 * (3 * K * 4 + 2 * LC.LAT_MAX_STATES) <= res["lds_limit"] else 64)


# ---- the validator: one refusal per rule, nothing launched ------------------------------------------------------------------------------
def _valid():
    return LC.make(3, {1: [(1.0, 0, 0), (1.5, 0, 1)], 2: [(1.0, 0, 2), (1.0, 1, 3)], 3: [(0.0, 2, LC.EPS)]}, [(4, 0), (5, 0), (6, 1), (7, 1)], [[5], [-1]])


def _arc(lat, k, **kw):
    c, s, y = lat["arcs"][k]
    lat["arcs"][k] = (kw.get("cost", c), kw.get("src", s), kw.get("sym", y))


REFUSALS = {
    "in_off not monotone": lambda l: l["in_off"].__setitem__(2, 5) or l["in_off"].__setitem__(3, 4),
    "state 0 has an incoming arc": lambda l: l["in_off"].__setitem__(1, 1),
    "source not below destination": lambda l: _arc(l, 1, src=1),
    "sources decrease": lambda l: _arc(l, 2, src=1) or _arc(l, 3, src=0),
    "symbol beyond the symbols": lambda l: _arc(l, 0, sym=4),
    "boundary beyond nstates - 1": lambda l: l["syms"].__setitem__(0, (4, 2)),
    "vocab_id beyond the vocabulary": lambda l: l["syms"].__setitem__(0, (1 << 20, 0)),
    "token below -1": lambda l: l["btok"].__setitem__(0, -2),
    "token beyond the vocabulary": lambda l: l["btok"].__setitem__(0, 1 << 20),
    "negative cost": lambda l: _arc(l, 0, cost=np.float32(-1.0)),
    "negative zero cost": lambda l: _arc(l, 0, cost=np.float32(-0.0)),
    "infinite cost": lambda l: _arc(l, 0, cost=np.float32(np.inf)),
    "NaN cost": lambda l: _arc(l, 0, cost=np.float32(np.nan)),
    "cost above 1e6": lambda l: _arc(l, 0, cost=np.float32(1.5e6)),
    "best_cost_init NaN": lambda l: l.__setitem__("best_cost_init", np.float32(np.nan)),
    "btok_off not monotone": lambda l: l["btok_off"].__setitem__(1, 3) or l["btok_off"].__setitem__(2, 2),
}


@pytest.mark.parametrize("rule", sorted(REFUSALS))
def test_validator_refuses_and_launches_nothing(world, rule):
    lat = _valid()
    REFUSALS[rule](lat)
    L.kernel_timer(True)
    try:
        with pytest.raises(A.AnxError):
            world.gpu["lm"].debug_lattice_decode(gparams(LC.Params(8)), [_valid(), lat])
        assert L.kernel_time("k_lattice")[1] == 0 and L.kernel_time("k_lattice_lm")[1] == 0
        world.gpu["lm"].debug_lattice_decode(gparams(LC.Params(8)), [_valid()])  # (the counter does count: the valid lattice launches)
        assert L.kernel_time("k_lattice")[1] == 1
    finally:
        L.kernel_timer(False)


def test_validator_refuses_sizes(world):
    g = world.gpu["lm"]
    L.kernel_timer(True)
    try:
        with pytest.raises(A.AnxError):  # nstates = 0
            g.debug_lattice_decode(gparams(LC.Params(8)), [dict(nstates=0, in_off=[0, 0], arcs=[], syms=[], btok_off=[0], btok=[], best_cost_init=0.0)])
        with pytest.raises(A.AnxError):  # the sub-range lies outside the view
            g.debug_lattice_decode(gparams(LC.Params(8)), [_valid()], first=1, count=1, pools=False)
        big = LC.Gen(1, LC.NLEX, LC.NLEX).dag(1000, 1, 1)
        with pytest.raises(A.AnxError):  # 5 x 1001 x 4096 nodes: above 2^24
            g.debug_lattice_decode(gparams(LC.Params(4096)), [big] * 5, pools=False)
        assert L.kernel_time("k_lattice")[1] == 0
    finally:
        L.kernel_timer(False)


# ---- one real call routed through the door ----------------------------------------------------------------------------------------------
class Recorder(TwinOverOracle):
    def most_likely_sequence(self, matches, boundaries, begin_offset, end_offset, params):
        self.seen.append((self.build_lattice_view(matches, boundaries, end_offset, params), list(matches)))
        return super().most_likely_sequence(matches, boundaries, begin_offset, end_offset, params)


def test_real_call_through_the_door(world):
    """a few hundred words through find_all_matches on the small LM model; the same text's lattices, rebuilt by the twin's builder from
    the C oracle's variants, through the door: the chosen symbols are the matches (and selected variants) the product returned"""
    lex, lm, _r = LC.model_spec("lm")
    tw, orc = Recorder(T.TEST_ALPHABET), O.OracleModel(alphabet_text=TSV)
    for w, f in lex:
        tw.add_to_vocabulary(w, f)
        orc.add(w, f)
    for t, f in lm:
        tw.add_lm(t, f)
        orc.add_lm(t, f)
    tw.build()
    orc.build()
    tw.attach(orc)
    tw.seen = []
    qs = synth.make_queries(list(LC.WORDS), 300, max_len=12, seed=7)
    text = "".join(q + (". " if i % 11 == 10 else ", " if i % 7 == 6 else " ") for i, q in enumerate(qs)).strip()
    kw = dict(max_anagram_distance=2, max_edit_distance=2, max_matches=6, score_threshold=0.3, cutoff_threshold=0.0, max_ngram=3, max_seq=250)
    g = world.gpu["lm"]
    got = g.find_all_matches_ids([text], A.SearchParameters(**kw))[0]
    tp = T.SearchParams(("abs", 2), ("abs", 2), 6, 0.3, 0.0, False, 0.0, max_ngram=3, max_seq=250)
    tw.find_all_matches(text, tp)
    views = [v for v, _m in tw.seen if v is not None]
    assert len(views) >= 1
    res = g.debug_lattice_decode(A.SearchParameters(**kw), views, pools=False)
    exp, k = [], 0
    for v, ms in tw.seen:
        if v is None:
            exp += [(m.begin, m.end, None) for m in ms]
            continue
        assert res["out_n"][k] != FILL
        for s in res["out_syms"][k][:res["out_n"][k]]:
            mi, vi = v["refs"][s]
            exp.append((ms[mi].begin, ms[mi].end, vi))
        k += 1
    assert [(m["begin"], m["end"]) for m in got] == [(b, e) for b, e, _v in exp]
    assert [m["selected"] for m in got if m["variants"]] == [v for _b, _e, v in exp if v is not None]
