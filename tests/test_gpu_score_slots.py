"""The scoring stage (kernels_score.hpp: k_filter_score, k_filter_wide, k_score_fast8, k_score_pairs / k_small_lists) by itself, through the
test hook anx_debug_score_slots, on the hand-laid pair lists of tests/score_cases.py against the twin's measures and pair_score
(oracle/twin.py).  Every slot of every region is compared, integers as integers and scores with ==; no tolerance anywhere (DESIGN.md
section 3: bit-identical f64).  Which paths of the kernels the pair lists take is asserted by tests/test_score_cases_cpu.py."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import analiticcl_amd as A
import score_cases as S
from analiticcl_amd import _lib as L

pytestmark = pytest.mark.gpu

SURVREC = np.dtype([("q", "<u4"), ("e", "<u4"), ("score", "<f8")])      # kernels_common.hpp SurvRec
SURVSEG = np.dtype([("score", "<f8"), ("e", "<u4"), ("pad", "<u4")])    # SurvSeg
FF = 0xFFFFFFFF
NAMES = list(S.BATCHES)


class Door:
    """a model of tests/score_cases.py on the device, with the entry id of every vocabulary item"""

    def __init__(self, m, tmp, device=0):
        self.m = m
        alpha, lex = tmp / ("%s.alphabet.tsv" % m.name), tmp / ("%s.lexicon.tsv" % m.name)
        alpha.write_text(m.alphabet_text(), encoding="utf-8")
        lex.write_text(m.lexicon_text(), encoding="utf-8")
        w = m.weights
        g = A.VariantModel(str(alpha), A.Weights(ld=w.ld, lcs=w.lcs, prefix=w.prefix, suffix=w.suffix, case=w.case), device=device)
        g.read_vocabulary(str(lex), A.VocabParams(freq_column=1 if m.have_freq else None))
        tp = A.VocabParams(freq_column=None, vocabtype="INDEXED|TRANSPARENT")
        for ref, text, score in m.variants:
            g.add_variant(3 + ref, text, score, None, tp)
        for text in m.transparent_only:
            g.add_to_vocabulary(text, None, tp)
        g.build()
        assert g.vocab_size() == 3 + len(m.texts) and all(g.vocab_text(3 + i) == t for i, t in enumerate(m.texts))
        pv, n = C.POINTER(C.c_uint32)(), C.c_size_t()
        L.check(L.lib().anx_debug_entries(g.h, C.byref(pv), C.byref(n)))
        self.ent_vocab = np.ctypeslib.as_array(pv, shape=(n.value,)).astype(np.int64)   # entry id -> vocabulary id
        C.CDLL(None).free(pv)
        assert sorted(self.ent_vocab.tolist()) == list(range(3, 3 + len(m.texts)))
        self.entry_of = np.zeros(3 + len(m.texts), dtype=np.int64)                      # vocabulary id -> entry id
        self.entry_of[self.ent_vocab] = np.arange(n.value)
        self.g = g
        self.batches = {}

    def batch(self, c):
        if c.name not in self.batches:
            th = c.threshold
            d = th[1] if th[0] == "abs" else (th[1], th[2])
            p = A.SearchParameters(max_anagram_distance=3, max_edit_distance=d, max_matches=0, score_threshold=c.score_threshold,
                                   cutoff_threshold=0.0, stop_criterion=c.stop)
            self.batches[c.name] = (A.Batch(self.g, c.queries, p), p)
        return self.batches[c.name][0]

    def device_slots(self, c, slots=None):
        """the case's slots with entry ids in place of vocabulary positions (the flag bits stay)"""
        s = (c.slots if slots is None else slots).astype(np.int64)
        valid = s[:, 0] != S.INVALID
        out = s.copy()
        out[valid, 1] = self.entry_of[3 + (s[valid, 1] & 0x3FFFFFF)] | (s[valid, 1] & (S.PRE | S.EXACT))
        return np.ascontiguousarray(out.astype(np.uint32))

    def run(self, c, seg_cap=0, surv_cap=8192, list_cap=8192, blk=S.FS_BLK, one_launch=0, slots=None, fills=None, shift=S.REGION_SHIFT, raw=False):
        b = self.batch(c)
        fills = np.ascontiguousarray(c.fills if fills is None else fills, dtype=np.uint32)
        dev = slots if raw else self.device_slots(c, slots)
        n, nq = len(dev), len(c.queries)
        assert n == int(fills.sum()), "the outputs are sized by the slots"
        o = dict(meta=np.zeros(max(n, 1), np.uint32), score=np.zeros(max(n, 1)), qcount=np.zeros((3, nq), np.uint32),
                 surv=np.zeros((S.REGIONS, surv_cap), SURVREC), ctr=np.zeros((5, S.REGIONS), np.uint32), seg=np.zeros((nq, max(seg_cap, 1)), SURVSEG),
                 skipped=np.zeros(1, np.uint32))
        o["rc"] = L.lib().anx_debug_score_slots(self.g.h, b.h, shift, fills.ctypes.data, dev.ctypes.data, seg_cap, surv_cap, list_cap, blk, one_launch,
                                                o["meta"].ctypes.data, o["score"].ctypes.data, o["qcount"].ctypes.data, o["surv"].ctypes.data,
                                                o["ctr"].ctypes.data, o["seg"].ctypes.data if seg_cap else None, o["skipped"].ctypes.data)
        o["meta"], o["score"] = o["meta"][:n], o["score"][:n]
        if seg_cap == 0:
            o["seg"] = None
        return o


@pytest.fixture(scope="module")
def doors(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("score_slots")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Door(S.model(name), tmp)
        return cache[name]
    return get


_EXPECT = {}


def expectation(c):
    if c.name not in _EXPECT:
        _EXPECT[c.name] = (S.expect(c), S.census(c))
    return _EXPECT[c.name]


def all_ff(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def check_slots(c, door, o, ex, listed_may_be_dropped=False):
    """p_meta and p_score of EVERY slot, the per-query counters, CTR_SKIPPED"""
    assert o["rc"] == 0, L.last_error()
    if listed_may_be_dropped:   # (slot lists below the need: a pair that found no room is never scored and keeps its 0xFF bytes)
        dropped = (o["meta"] == FF) & (ex.meta != FF)
        assert dropped.any()
        for i in np.nonzero(dropped)[0]:
            p = S.slot_pair(c, int(i))
            assert max(p.lq, p.lc) > 16 or c.D == 0, ("an inline pair lost", int(i))
        ok = ~dropped
    else:
        ok = np.ones(len(ex.meta), dtype=bool)
    bad = np.nonzero((o["meta"] != ex.meta) & ok)[0]
    assert bad.size == 0, (c.name, "p_meta of slot", int(bad[0]), "region", int(ex.region[bad[0]]), hex(int(o["meta"][bad[0]])), hex(int(ex.meta[bad[0]])),
                           _describe(c, int(bad[0])), bad.size)
    has = ~np.isnan(ex.score) & ok
    bad = np.nonzero(has & ~(o["score"] == ex.score))[0]
    assert bad.size == 0, (c.name, "p_score of slot", int(bad[0]), o["score"][bad[0]], ex.score[bad[0]], _describe(c, int(bad[0])), bad.size)
    assert np.isnan(o["score"][~has & ok]).all(), "a score where the reference has no distance"
    if not listed_may_be_dropped:
        for k, name in enumerate(("qsurv", "qmaxfreq")):
            bad = np.nonzero(o["qcount"][k] != getattr(ex, name))[0]
            assert bad.size == 0, (c.name, name, "query", int(bad[0]), c.queries[bad[0]], int(o["qcount"][k][bad[0]]), int(getattr(ex, name)[bad[0]]), bad.size)
        if c.model.any_variants:
            assert (o["qcount"][2] == ex.qexpand).all(), np.nonzero(o["qcount"][2] != ex.qexpand)[0][:5]
        else:
            assert all_ff(o["qcount"][2])   # (only models with variant lists clear and use qexpand)
        assert int(o["skipped"][0]) == ex.n_skipped


def _describe(c, i):
    q, w = int(c.slots[i, 0]), int(c.slots[i, 1])
    return (c.queries[q], c.model.texts[w & 0x3FFFFFF], "d", c.dq[q], "flags", w >> 30) if q != S.INVALID else "invalid"


def region_records(door, o, cap):
    """Counter of (region, query, vocabulary position, score) over the written records of the region lists; the rest must be 0xFF"""
    got = Counter()
    for r in range(S.REGIONS):
        fill = int(o["ctr"][0][r])
        n = min(fill, cap)
        rec = o["surv"][r]
        assert all_ff(rec[n:]), ("survivor list of region", r, "written beyond", n)
        for q, e, s in rec[:n].tolist():
            assert e < len(door.ent_vocab), ("survivor record", r, q, e)
            got[(r, q, int(door.ent_vocab[e]) - 3, s)] += 1
    return got


def check_survivors(c, door, o, ex, seg_cap):
    kept_by_q = Counter()
    for (r, q, e, s), n in ex.kept.items():
        kept_by_q[q] += n
    lists = region_records(door, o, o["surv"].shape[1])
    if seg_cap == 0:
        assert lists == ex.kept, (c.name, "survivor records", list((lists - ex.kept).items())[:3], list((ex.kept - lists).items())[:3])
        for r in range(S.REGIONS):
            assert int(o["ctr"][0][r]) == sum(n for (rr, _, _, _), n in ex.kept.items() if rr == r)
        return
    # segments: positions 0 .. min(n, C) - 1 written, the rest 0xFF; the surplus in the region lists; the union is the kept set
    total = Counter()
    for (r, q, e, s), n in lists.items():
        total[(q, e, s)] += n
        assert ex.kept[(r, q, e, s)] >= n, (c.name, "surplus record outside its slot's region", r, q, e, s)
    for q in range(len(c.queries)):
        n = min(kept_by_q[q], seg_cap)
        seg = o["seg"][q]
        assert all_ff(seg[n:]), (c.name, "segment of query", q, "beyond", n)
        for s, e, pad in seg[:n].tolist():
            assert pad == 0 and e < len(door.ent_vocab), (c.name, "segment of query", q, e, pad)
            total[(q, int(door.ent_vocab[e]) - 3, s)] += 1
    want = Counter()
    for (r, q, e, s), n in ex.kept.items():
        want[(q, e, s)] += n
    assert total == want, (c.name, "segments + surplus", list((total - want).items())[:3], list((want - total).items())[:3])
    assert int(o["ctr"][0].sum()) == sum(max(0, n - seg_cap) for n in kept_by_q.values())


def check_lists(o, t, split=True):
    assert int(o["ctr"][3].sum()) == (t["need_listw"] if split else 0)
    assert int(o["ctr"][1].sum()) == t["need_list8"] and int(o["ctr"][2].sum()) == t["need_listg"]
    assert int(o["ctr"][4].sum()) == t["need_selected"]


@pytest.mark.parametrize("name", NAMES)
def test_every_slot_against_the_twin(doors, name):
    """the batch path's launches at its block size, without segments and with segments of 2 and 32 records"""
    c = S.case(name)
    door = doors(c.model.name)
    ex, t = expectation(c)
    for seg_cap in (0,) + S.SEG_CAPS:
        o = door.run(c, seg_cap=seg_cap)
        if seg_cap and (c.stop or c.model.any_variants):
            assert o["rc"] == L.ANX_EINVAL and all_ff(o["meta"]) and all_ff(o["surv"]) and all_ff(o["seg"])   # a run of this batch has no segments
            continue
        check_slots(c, door, o, ex)
        check_survivors(c, door, o, ex, seg_cap)
        check_lists(o, t)


@pytest.mark.parametrize("name", [n for n in NAMES if S.BATCHES[n][0] != "f"])
@pytest.mark.parametrize("blk", [256, 512])
def test_small_blocks_and_one_launch(doors, name, blk):
    """the small call's geometry: blocks of 256 / 512 slots and the slot-list kernels as the one launch k_small_lists (launched by the
    function small_find launches them with).  Every batch whose plan leaves k_score_pairs 256 threads: all but model f's
    (test_one_launch_needs_256_threads)."""
    c = S.case(name)
    door = doors(c.model.name)
    ex, t = expectation(c)
    seg_cap = 0 if (c.stop or c.model.any_variants) else 32 if blk == 512 else 2
    o = door.run(c, seg_cap=seg_cap, blk=blk, one_launch=1)
    check_slots(c, door, o, ex)
    check_survivors(c, door, o, ex, seg_cap)
    check_lists(o, t)


def test_one_launch_needs_256_threads(doors):
    """beside a 255-symbol entry k_score_pairs has 128 or 64 threads: the small call launches the list kernels one by one, and so must the door"""
    c = S.case("f-abs4")
    o = doors("f").run(c, one_launch=1)
    assert o["rc"] == L.ANX_EINVAL and all_ff(o["meta"]) and all_ff(o["surv"]) and all_ff(o["ctr"])
    for blk in (256, 512):
        o = doors("f").run(c, blk=blk)
        check_slots(c, doors("f"), o, *expectation(c)[:1])


@pytest.mark.parametrize("name", ["a-abs3-cut", "a-abs4", "d-abs2"])
def test_capacity_below_need(doors, name):
    """a survivor list / slot lists smaller than the need: nothing is written beyond the capacity, the counter reports the whole need
    (what batch_finish regrows from), the records below the capacity are valid"""
    c = S.case(name)
    door = doors(c.model.name)
    ex, t = expectation(c)
    cap = 48
    o = door.run(c, surv_cap=cap)
    check_slots(c, door, o, ex)
    need = [sum(n for (rr, _, _, _), n in ex.kept.items() if rr == r) for r in range(S.REGIONS)]
    assert max(need) > 4 * cap and [int(x) for x in o["ctr"][0]] == need
    got = region_records(door, o, cap)   # (asserts the 0xFF bytes beyond min(fill, cap))
    assert not got - ex.kept and sum(got.values()) == sum(min(n, cap) for n in need)
    # the slot lists: k_filter_score's own appends report the whole need, pairs without room are not scored, everything else is as before
    o = door.run(c, list_cap=16)
    assert o["rc"] == 0, L.last_error()
    first = "need_listw" if c.D > 0 else "need_listg"
    assert t[first] > 16 * S.REGIONS or t[first] > 200
    assert int(o["ctr"][3 if c.D > 0 else 2].sum()) == t[first]
    check_slots(c, door, o, ex, listed_may_be_dropped=True)
    got = region_records(door, o, o["surv"].shape[1])
    assert not got - ex.kept


@pytest.mark.parametrize("switch", ["ANX_FS_SPLIT", "ANX_FS_PLANES"])
def test_byte_row_instances(doors, switch):
    """ANX_FS_SPLIT=0: the WIDE = true instances (8-word prefilter inline, byte rows); ANX_FS_PLANES=0: byte rows with the split prefilter.
    Both run the short round on the batch's D and leave the query's own d to the drain: a ratio batch, whose queries have d = 1, 2 and 3."""
    c = S.case("a-ratio")
    door = doors("a")
    ex, t = expectation(c)
    assert S.census(c, planes=False)["drain_fails_own_d"] > 0
    A.set_switch(switch, "0")
    try:
        for seg_cap in (0, 2):
            o = door.run(c, seg_cap=seg_cap)
            check_slots(c, door, o, ex)
            check_survivors(c, door, o, ex, seg_cap)
            check_lists(o, t, split=switch != "ANX_FS_SPLIT")
    finally:
        A.set_switch(switch, None)


def test_refusals_launch_nothing(doors):
    """a flag outside the scan's contract, an index out of range, a fill beyond the region, a bad geometry: ANX_EINVAL, every output still 0xFF"""
    c = S.case("a-abs2")
    door = doors("a")
    dev = door.device_slots(c)

    def refused(o):
        assert o["rc"] == L.ANX_EINVAL, o["rc"]
        assert all(all_ff(o[k]) for k in ("meta", "score", "qcount", "surv", "ctr", "skipped")) and (o["seg"] is None or all_ff(o["seg"]))

    P = [S.slot_pair(c, i) for i in range(len(c.slots))]
    flags = (c.slots[:, 1] & S.PRE) != 0
    cases = []
    i = next(i for i, p in enumerate(P) if p and not flags[i] and p.bandrej and p.lq <= 16 and p.lc <= 16)
    cases.append(("the band-match bound rejects the pair", i, int(dev[i, 1]) | S.PRE))
    i = next(i for i, p in enumerate(P) if p and abs(p.lq - p.lc) > p.dq)
    cases.append(("lengths further apart than d", i, int(dev[i, 1]) | S.PRE))
    i = next(i for i, p in enumerate(P) if p and p.lc > 16 and abs(p.lq - p.lc) <= p.dq)
    cases.append(("an entry beyond 16 symbols", i, int(dev[i, 1]) | S.PRE))
    i = next(i for i, p in enumerate(P) if p)
    cases.append(("the exact-class bit outside StopAtExactMatch", i, int(dev[i, 1]) | S.EXACT))
    cases.append(("entry id out of range", i, len(door.ent_vocab)))
    # a valid flagged word with a bit above the short round's 26-bit entry mask: a mixed wave's general round would gather at the 30-bit id
    i = int(np.nonzero(flags)[0][0])
    for bit in (26, 27, 29):
        cases.append(("flagged word with bit %d" % bit, i, int(dev[i, 1]) | (1 << bit)))
    for what, i, word in cases:
        bad = dev.copy()
        bad[i, 1] = word
        refused(door.run(c, slots=bad, raw=True, seg_cap=2))
    bad = dev.copy()
    bad[7, 0] = len(c.queries)
    refused(door.run(c, slots=bad, raw=True))
    fills = np.zeros(S.REGIONS, np.uint32)
    fills[5] = (1 << 10) + 1   # (region_shift 10 below: 1024 slots per region)
    refused(door.run(c, slots=np.ascontiguousarray(dev[:fills[5]]), raw=True, fills=fills, shift=10))
    fills[5] = 1 << 10
    assert door.run(c, slots=np.ascontiguousarray(dev[:fills[5]]), raw=True, fills=fills, shift=10)["rc"] == 0, L.last_error()
    for kw in (dict(blk=0), dict(blk=300), dict(blk=8192), dict(list_cap=0), dict(list_cap=(1 << 16) + 1), dict(surv_cap=0), dict(shift=9), dict(shift=17)):
        refused(door.run(c, **kw))
    # flags in a StopAtExactMatch batch, and under an alphabet the bit-plane scan does not take
    cs = S.case("a-stop")
    i = next(i for i in range(len(cs.slots)) if S.slot_pair(cs, i) and S.slot_pair(cs, i).ld is not None and S.slot_pair(cs, i).lc <= 16)
    bad = door.device_slots(cs)
    bad[i, 1] |= S.PRE
    refused(door.run(cs, slots=bad, raw=True))
    cb = S.case("b-abs2")
    i = next(i for i in range(len(cb.slots)) if S.slot_pair(cb, i) and S.slot_pair(cb, i).ld is not None and S.slot_pair(cb, i).lc <= 16)
    bad = doors("b").device_slots(cb)
    bad[i, 1] |= S.PRE
    refused(doors("b").run(cb, slots=bad, raw=True))
    # and the unchanged slots pass
    check_slots(c, door, door.run(c, slots=dev, raw=True), expectation(c)[0])


def test_door_against_pipeline(doors):
    """The pairs a real run scored (anx_batch_fetch_pairs), laid out as slots, through the door: its kept set is the run's survivors as the
    ranked rows show them at max_matches = 0 and cutoff 0, and its per-slot outputs are the run's own."""
    c = S.case("a-abs3-cut")
    door = doors("a")
    b = door.batch(c)
    b.run()
    pairs = b.fetch_pairs()
    rows = b.fetch()
    assert len(pairs) > 2000
    per = 1 << S.REGION_SHIFT
    fills = np.zeros(S.REGIONS, np.uint32)
    slots = np.zeros((len(pairs), 2), np.uint32)
    for i, (q, vid, *_rest) in enumerate(pairs):
        slots[i] = (q, door.entry_of[vid])
        fills[i % S.REGIONS] += 1
    order = np.argsort(np.arange(len(pairs)) % S.REGIONS, kind="stable")   # region r takes pairs r, r + 64, ...
    assert fills.max() <= per
    o = door.run(c, slots=np.ascontiguousarray(slots[order]), fills=fills, raw=True)
    assert o["rc"] == 0, L.last_error()
    got = Counter()
    for (r, q, e, s), n in region_records(door, o, o["surv"].shape[1]).items():
        got[(q, e + 3, s)] += n
    want = Counter((q, vid, dist) for q, rr in enumerate(rows) for vid, dist, _ in rr)
    assert got == want and sum(want.values()) > 300
    for k, i in enumerate(order.tolist()):
        q, vid, ld, lcs, pre, suf, same, score = pairs[i]
        meta = int(o["meta"][k])
        assert (meta & 0x7F) == (0x7F if ld < 0 else ld) and (ld < 0 or (meta >> 8, o["score"][k]) == (lcs | pre << 8 | suf << 16, score)), (k, pairs[i], hex(meta))
