"""The hand-made lattices of tests/lattice_cases.py and their reference (oracle/twin.py decode_lattice), without a GPU: the census
proves from the lattices and the reference alone that every branch class of the device decoder the cases aim at is populated (under a
64 KB and under a 160 KB LDS limit per block: the routing above K = 2048 depends on it); decode_lattice is pinned against a brute-force
enumeration of every path, against most_likely_sequence on the twin's own running text, and -- on text, the only form the C oracle
takes -- against the C restatement of search mode."""
import random
import time

import numpy as np
import pytest

from analiticcl_amd import synth
from oracle import cwrap as O
from oracle import twin as T

import lattice_cases as LC
from search_common import TwinOverOracle

TSV = "\n".join(f"{c}\t{c.upper()}" for c in "abcdefghijklmnopqrstuvwxyz") + "\n.\t,\n"


@pytest.fixture(scope="module")
def models():
    return {k: LC.twin_model(k) for k in ("lm", "rules", "nolm")}


def test_model_ids_are_where_the_cases_expect_them(models):
    m = models["lm"]
    assert m.encoder[LC.WORDS[0]] == 3 and m.encoder[LC.LM_ONLY[0]] == LC.NLEX and m.encoder["able acid aged"] == LC.MULTI0
    assert len(m.decoder) == LC.MULTI0 + 5 and len(models["nolm"].decoder) == LC.NLEX
    assert m.have_lm and not models["nolm"].have_lm and len(models["rules"].context_rules) == 4
    assert m._into_ngram(LC.MULTI0 + 4) is None and len(m._into_ngram(LC.MULTI0 + 2)) == 5  # 6 parts: no tokens; 5 parts: 5
    assert any(j > m.ngrams.get((a[0],), 1) for a, j in m.ngrams.items() if len(a) == 2)     # both branches of the bigram term
    assert any(j <= m.ngrams.get((a[0],), 1) for a, j in m.ngrams.items() if len(a) == 2)


@pytest.mark.parametrize("lds_limit", [64 << 10, 160 << 10])
def test_every_census_class_is_populated(models, lds_limit):
    t0, ref0 = time.time(), LC.REF_SECONDS[0]
    got, handed = set(), {}
    for b in LC.batches(lds_limit):
        name, kind, P, lats, _budgets = b
        nv = len(models[kind].decoder)  # what the door's validator asks of the cases
        assert all(v < nv and bd < l["nstates"] - 1 for l in lats for v, bd in l["syms"]) and all(-1 <= t < nv for l in lats for t in l["btok"]), name
        pl = LC.plan(lats, max(1, P.max_seq), lds_limit, 0, kind == "rules")
        refs = [LC.reference(models[kind], l, P) if pl["why"][j] is None else None for j, l in enumerate(lats)]
        got |= LC.census(models[kind], b, refs, lds_limit)
        handed[name] = [w for w in pl["why"] if w]
    missing = set(LC.EXPECTED_CLASSES) - got
    print("census: %d classes, reference %.1f s of %.1f s; unreachable by construction: %s" % (len(got), LC.REF_SECONDS[0] - ref0, time.time() - t0, LC.UNREACHABLE))
    assert not missing, sorted(missing)
    # what the issue fixes: D = 129 is handed back and nothing else of the width batches; 1024 states; the ring beyond the wide cap; K = 4097
    assert handed["widths-K8"] == ["indegree"] * 2 and handed["widths-K250"] == ["indegree"] * 2
    assert handed["pairing-5"] == ["states"] and handed["ring-K250"] == ["ring"] and handed["bigK-4097"] == ["K", "K"]
    assert all(not h for n, h in handed.items() if n.startswith(("ties", "lm-", "rules", "unreachable")) or n in ("bigK-1000", "bigK-2048", "bigK-2049", "bigK-4096"))


def test_routing_above_k_2048_follows_the_lds_limit():
    """2 x (3 x K x 4 + 2 x 1024) bytes is the narrow kernel's request with its floor of three lists: ~100 KB at K = 4096"""
    assert LC.ring_caps(2048, 64 << 10) == (5, 2) and LC.ring_caps(250, 64 << 10) == (48, 23)
    assert LC.ring_caps(4096, 64 << 10) == (2, 0) and LC.ring_caps(4096, 160 << 10) == (2, 2)
    assert LC.ring_caps(2560, 64 << 10)[1] == 2 and LC.ring_caps(2561, 64 << 10)[1] == 1
    fan = LC.Gen(1, LC.NLEX, LC.NLEX).fan([64, 64])
    assert LC.plan([fan], 4096, 64 << 10)["kernel"] == [64] and LC.plan([fan], 4096, 160 << 10)["kernel"] == [32]


def brute_force(lat, K):
    """every path from state 0 to the end state, its cost summed in f32 along the path: the K smallest costs (an independent restatement
    of the k-best contract; ties between equal costs leave the cost list itself unchanged)"""
    ns, io, arcs = lat["nstates"], lat["in_off"], lat["arcs"]
    out = [[] for _ in range(ns + 1)]
    for d in range(1, ns + 1):
        for k in range(io[d], io[d + 1]):
            out[arcs[k][1]].append((arcs[k][0], d))
    costs, stack = [], [(0, np.float32(0.0))]
    while stack:
        s, c = stack.pop()
        if s == ns:
            costs.append(float(c))
            continue
        for ac, d in out[s]:
            stack.append((d, np.float32(c + ac)))
    return sorted(costs)[:K]


def test_decode_lattice_against_brute_force(models):
    """K larger than the number of paths: nothing is pruned on the way, so the final list must be exactly the sorted path costs; and
    K small: the K best survive the pruning per state"""
    g = LC.Gen(31, LC.NLEX, LC.NLEX, costs=(0.0, 1.0, 1.5, 2.0, None))
    for i in range(40):
        lat = g.dag(g.rng.randrange(2, 8), g.rng.randrange(1, 4), g.rng.randrange(1, 4), finals=g.rng.randrange(1, 3), chain=i % 2 == 0)
        for K in (1, 3, 100000):
            res = models["nolm"].decode_lattice(lat, K, LC.Params(K))
            assert [float(c) for c, _p, _s in res["nodes"][lat["nstates"]]] == brute_force(lat, K), (i, K)
            for d, st in enumerate(res["nodes"]):  # every node's cost is its parent's plus an arc of its state with that source and symbol
                for c, par, sym in st[0 if d else 1:]:
                    pc = res["nodes"][par >> 16][par & 0xFFFF][0]
                    assert any(np.float32(pc + a[0]) == c and a[1] == par >> 16 and a[2] == sym for a in lat["arcs"][lat["in_off"][d]:lat["in_off"][d + 1]])


def test_tie_order_is_cost_source_arc_rank(models):
    """all-equal costs: the nodes of a state come in (source state, arc number, rank at the source) order"""
    lat = LC.make(3, {1: [(1.0, 0, 0), (1.0, 0, 1)], 2: [(1.0, 1, 2), (2.0, 0, 3), (1.0, 1, 3)], 3: [(0.0, 2, LC.EPS)]}, [(4, 0), (5, 0), (6, 1), (7, 1)])
    res = models["nolm"].decode_lattice(lat, 10, LC.Params(10))
    assert [(p, s) for _c, p, s in res["nodes"][2]] == [(0 << 16, 3), (1 << 16, 2), (1 << 16 | 1, 2), (1 << 16, 3), (1 << 16 | 1, 3)]
    assert res["chosen"] == 0 and res["out_syms"] == [3]


class Recorder(TwinOverOracle):
    def most_likely_sequence(self, matches, boundaries, begin_offset, end_offset, params):
        out = super().most_likely_sequence(matches, boundaries, begin_offset, end_offset, params)
        self.seen.append((list(matches), list(boundaries), end_offset, out))
        return out


def test_builder_and_decoder_reproduce_most_likely_sequence_and_the_c_oracle(models):
    """random running text over the small LM model: decode_lattice over the builder's arrays is what most_likely_sequence returns
    (symbols -> matches through the builder's refs), and the C oracle's search returns the same matches for the same text"""
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
    rng = random.Random(5)
    qs = synth.make_queries(list(LC.WORDS), 120, max_len=12, seed=11)
    tp = T.SearchParams(("abs", 2), ("abs", 2), 6, 0.3, 0.0, False, 0.0, max_ngram=3, max_seq=250)
    sp = O.make_search_params(O.make_params(("abs", 2), ("abs", 2), 6, 0.3, 0.0), max_ngram=3, max_seq=250)
    decoded = 0
    for k in range(0, len(qs), 8):
        text = "".join(q + rng.choice((" ", " ", " ", ", ", ". ")) for q in qs[k:k + 8]).strip()
        exp = tw.find_all_matches(text, tp)
        res, _ = orc.find_all_matches(text, sp)
        assert [(t, b, e, sel) for t, b, e, _n, sel, var in res if var] == [(m.text, m.begin, m.end, m.selected) for m in exp if m.variants], text
    for matches, boundaries, end_offset, out in tw.seen:
        view = tw.build_lattice_view(matches, boundaries, end_offset, tp)
        if view is None:
            assert out is matches or out == matches
            continue
        ref = tw.decode_lattice(view, 250, tp)
        got = [view["refs"][s] for s in ref["out_syms"]]
        assert [(matches[mi].begin, matches[mi].end, vi) for mi, vi in got] == [(m.begin, m.end, m.selected) for m in out]
        assert LC.ring_of(view) == view["ring"] and len(view["in_off"]) == view["nstates"] + 2 and len(view["btok_off"]) == view["nstates"]
        decoded += 1
    assert decoded >= 10
