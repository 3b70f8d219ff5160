"""The scan stage (kernels_scan.hpp: k_scan_adj, k_scan_bits, k_scan_sad; k_scan_small) by itself, through the test hook
anx_debug_scan_pairs, on tiles the product's own encoders made, against the reference set of tests/scan_cases.py (count vectors,
computed from the strings alone; tied to the twin and the C oracle by tests/test_scan_cases_cpu.py).  Every slot of the pair list and
every region counter is compared with ==, and no query is left out: a mismatch names the query, the entry and the tile.

The tile-side classes of inputs (tile sizes, kinds inside a tile, walks, launches) are asserted here from the tiles the door returns:
if the encoder stops producing one of them, the test says so instead of passing."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import analiticcl_amd as A
import scan_cases as S
from analiticcl_amd import _lib as L

pytestmark = pytest.mark.gpu

PROD = dict(chunk=256, chunk_fused=128, chunk_first=32, fuse=True, twins=True, drop_len=True, want_exact=False, count_pairs=False)   # what a run sets
SMALL = dict(PROD, chunk=64, chunk_fused=32, chunk_first=64)                                                                      # ... and the small call


class Door:
    """a model of tests/scan_cases.py on the device, with the vocabulary position of every entry id"""

    def __init__(self, m, tmp):
        self.m = m
        alpha, lex = tmp / ("%s.alphabet.tsv" % m.name), tmp / ("%s.lexicon.tsv" % m.name)
        alpha.write_text(m.alphabet_text(), encoding="utf-8")
        lex.write_text(m.lexicon_text(), encoding="utf-8")
        try:
            for k, v in m.switches:
                A.set_switch(k, v)
            g = A.VariantModel(str(alpha), A.Weights(), device=0)
            g.read_vocabulary(str(lex), A.VocabParams(freq_column=None))
            g.build()
        finally:
            for k, _ in m.switches:
                A.set_switch(k, None)
        assert g.vocab_size() == 3 + len(m.texts) and all(g.vocab_text(3 + i) == t for i, t in enumerate(m.texts[:50]))
        pv, n = C.POINTER(C.c_uint32)(), C.c_size_t()
        L.check(L.lib().anx_debug_entries(g.h, C.byref(pv), C.byref(n)))
        self.pos_of_entry = np.ctypeslib.as_array(pv, shape=(n.value,)).astype(np.int64) - 3
        C.CDLL(None).free(pv)
        assert sorted(self.pos_of_entry.tolist()) == list(range(len(m.texts)))
        self.g = g
        self.batches = {}

    def params(self, c):
        th = lambda t: t[1] if t[0] == "abs" else (t[1], t[2])
        return A.SearchParameters(max_anagram_distance=th(c.kth), max_edit_distance=th(c.dth), max_matches=10, stop_criterion=c.stop)

    def batch(self, c):
        """the case's batch, encoded under the case's switches (they are read at encode time)"""
        if c.name not in self.batches:
            try:
                for k, v in c.switches:
                    A.set_switch(k, v)
                self.batches[c.name] = A.Batch(self.g, c.queries, self.params(c))
            finally:
                for k, _ in c.switches:
                    A.set_switch(k, None)
        return self.batches[c.name]

    def scan(self, c, shift=None, **opts):
        o = dict(SMALL if c.small_slots else PROD)
        o.update(opts)
        if shift is None:   # room for every pair of the case in ONE region, whatever the tiles are
            need = sum(len(r.ents) for r in c.ref) + 2048
            shift = max(12, int(np.ceil(np.log2(need))))
        if c.small_slots:
            res = self.g.debug_scan_pairs(inputs=c.queries, params=self.params(c), region_shift=shift, slots=c.small_slots, **o)
        else:
            res = self.g.debug_scan_pairs(batch=self.batch(c), region_shift=shift, **o)
        res["opts"], res["shift"] = o, shift
        return res

    def list_headers(self, tiles):
        """anx_debug_adjacency_device for the tiles' signatures: [tiles, 8] {first row or UINT32_MAX, cumulative rows of the 7 sections}"""
        sig = np.ascontiguousarray(tiles[:, S.T_SIGLO].astype(np.uint64) | (tiles[:, S.T_SIGHI].astype(np.uint64) << np.uint64(32)))
        cum = np.zeros((len(sig), 8), dtype=np.uint32)
        ids = C.POINTER(C.c_uint32)()
        L.check(L.lib().anx_debug_adjacency_device(self.g.h, sig.ctypes.data_as(C.c_void_p), len(sig), cum.ctypes.data_as(C.c_void_p), C.byref(ids)))
        C.CDLL(None).free(ids)
        return cum


@pytest.fixture(scope="module")
def doors(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scan_door")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Door(S.model(name), tmp)
        return cache[name]
    yield get
    for d in cache.values():
        for b in d.batches.values():
            b.free()


_EXPECT = {}


def expectation(c, o):
    key = (c.name, bool(o["drop_len"]), bool(o["fuse"]), bool(o["want_exact"]))
    if key not in _EXPECT:
        _EXPECT[key] = [S.expected(c.model, r, *key[1:]) for r in c.ref]
    return _EXPECT[key]


def pair_key(inp, pos, flags):
    return (np.asarray(inp, dtype=np.int64) << 34) | (np.asarray(pos, dtype=np.int64) << 2) | np.asarray(flags, dtype=np.int64)


def describe(c, key):
    inp, pos, fl = int(key) >> 34, (int(key) >> 2) & ((1 << 32) - 1), int(key) & 3
    return dict(input=inp, query=c.queries[inp], entry=c.model.texts[pos][:40], prefiltered=bool(fl & 1), exact=bool(fl & 2))


def check(c, door, res, below_capacity=False):
    """everything the door returns against the reference; -> per-region RC_VALID"""
    m, o, small = c.model, res["opts"], bool(c.small_slots)
    tiles, nq, cap = res["tiles"], res["nq"], 1 << res["shift"]
    ex = expectation(c, o)
    assert res["guard"] == 0, "slots behind the pair list were written"
    # ---- the queries: every input once, with the reference's length, clamps and kind ---------------------------------------------------
    assert nq == len(c.queries) and sorted(res["q_orig"].tolist()) == list(range(nq))
    qo = res["q_orig"].astype(np.int64)
    refs = [c.ref[i] for i in qo]
    meta = res["meta"]
    assert (meta & 0xFF).tolist() == [r.lq for r in refs]
    assert ((meta >> 8) & 0xFF).tolist() == [r.k for r in refs] and ((meta >> 16) & 0xFF).tolist() == [r.d for r in refs]
    assert res["kind"].tolist() == [r.kind for r in refs], "the kind a tile tests a query with"
    # ---- the tiles: every query in a tile (the small form: in every part of its own), uniform in length, k, d ---------------------------
    live = np.nonzero(tiles[:, S.T_NQ] != 0)[0]
    region_of_tile = S.launch_regions(len(tiles), res["nadj"], res["nbits"], res["nsad"], small)
    # (a tile that walks a window or probes a large ball is cut into parts, in both forms: such a query is in several tiles)
    tile_of_q = np.full(nq, -1, dtype=np.int64)        # its first tile
    ntiles_of_q = np.zeros(nq, dtype=np.int64)
    allowed = np.zeros((nq, S.REGIONS), dtype=bool)    # the regions of a query's tiles
    for t in live:
        q0, n = int(tiles[t, S.T_Q0]), int(tiles[t, S.T_NQ])
        assert n <= 64 and q0 + n <= nq
        first = tile_of_q[q0:q0 + n] == -1
        tile_of_q[q0:q0 + n][first] = t
        ntiles_of_q[q0:q0 + n] += 1
        allowed[q0:q0 + n, region_of_tile[t]] = True
        for s in range(q0, q0 + n):
            r = refs[s]
            assert (int(tiles[t, S.T_LQ]), int(tiles[t, S.T_K]), int(tiles[t, S.T_D])) == (r.lq, r.k, r.d)
            assert (int(tiles[t, S.T_KIND]) == 0) == (r.kind == 0)
    assert (tile_of_q >= 0).all(), "a query in no tile"
    # ---- the slots --------------------------------------------------------------------------------------------------------------------------
    raw, rctr = res["raw"], res["rctr"]
    rc_raw = rctr[:, S.RC_RAW].astype(np.int64)
    if below_capacity:
        assert (rc_raw > cap).any(), "the capacity was meant to be below the need"
    else:
        assert (rc_raw <= cap).all(), ("a region overflowed: the case needs a larger region_shift", int(rc_raw.max()), cap)
    idx = np.arange(cap)[None, :]
    reserved = idx < np.minimum(rc_raw, cap)[:, None]
    qw, ew = raw[:, :, 0], raw[:, :, 1]
    untouched = (qw == S.FILL) & (ew == S.FILL)
    assert untouched[~reserved].all(), "a slot beyond the region's reservations was written"
    valid = reserved & (qw != S.INVALID)
    if not below_capacity:
        assert not (untouched & reserved).any(), "a reserved slot that is neither a pair nor RAW_INVALID"
    else:   # (reservations that reach beyond the region: the part inside is written or closed, nothing of it keeps the fill)
        assert not (untouched & reserved & (idx < cap)).any()
    assert (qw[valid] < nq).all() and ((ew[valid] & S.ENTRY_MASK) < len(m.texts)).all()
    reg, _ = np.nonzero(valid)
    got_q = qw[valid].astype(np.int64)
    got = pair_key(qo[got_q], door.pos_of_entry[(ew[valid] & S.ENTRY_MASK).astype(np.int64)], ew[valid] >> 30)
    exp_inp = np.concatenate([np.full(len(e.written), i, dtype=np.int64) for i, e in enumerate(ex)] + [np.zeros(0, np.int64)])
    exp_pf = np.array([pf for e in ex for pf in e.written], dtype=np.int64).reshape(-1, 2)
    assert all(v == 1 for e in ex for v in e.written.values())
    want = pair_key(exp_inp, exp_pf[:, 0], exp_pf[:, 1])
    gs, ws = np.sort(got), np.sort(want)
    dup = gs[1:][gs[1:] == gs[:-1]]
    assert dup.size == 0, ("a pair written twice", describe(c, dup[0]), "tile", int(tile_of_q[np.nonzero(qo == (int(dup[0]) >> 34))[0][0]]), dup.size)
    extra, missing = np.setdiff1d(gs, ws), np.setdiff1d(ws, gs)
    assert extra.size == 0, ("a pair the reference does not have (or with other flag bits)", describe(c, extra[0]),
                             "tile", int(tile_of_q[np.nonzero(qo == (int(extra[0]) >> 34))[0][0]]), extra.size)
    if below_capacity:
        assert missing.size > 0
    else:
        assert missing.size == 0, ("a reference pair is not in the list", describe(c, missing[0]),
                                   "tile", int(tile_of_q[np.nonzero(qo == (int(missing[0]) >> 34))[0][0]]), missing.size)
    # ---- per region: the slots and the counters ------------------------------------------------------------------------------------------------
    sorted_pos = np.empty(nq, dtype=np.int64)
    sorted_pos[qo] = np.arange(nq)
    n_ref = np.array([e.n_ref for e in ex], dtype=np.int64)[qo]        # per sorted query
    n_fused = np.array([e.n_fused for e in ex], dtype=np.int64)[qo]
    assert allowed[got_q, reg].all(), "a pair outside the regions of its query's tiles"
    assert int(rctr[:, S.RC_VALID].sum()) == int(n_ref.sum()), "RC_VALID, all regions"
    assert int(rctr[:, S.RC_FUSED].sum()) == int(n_fused.sum()), "RC_FUSED, all regions"
    # the regions that hold no part of a cut query: their counters are the sums over their tiles' queries
    whole = ntiles_of_q == 1
    clean = ~allowed[~whole].any(axis=0)
    region_of_q = region_of_tile[tile_of_q]
    for word, per_q in ((S.RC_VALID, n_ref), (S.RC_FUSED, n_fused)):
        want_r = np.bincount(region_of_q[whole], weights=per_q[whole], minlength=S.REGIONS).astype(np.int64)
        most_r = want_r + (allowed[~whole] * per_q[~whole][:, None]).sum(axis=0).astype(np.int64)   # (a cut query's pairs: in any of its parts)
        have_r = rctr[:, word].astype(np.int64)
        bad = np.nonzero((clean & (have_r != want_r)) | (have_r < want_r) | (have_r > most_r))[0]
        assert bad.size == 0, ("region counter", word, "region", int(bad[0]), int(have_r[bad[0]]), int(want_r[bad[0]]), int(most_r[bad[0]]))
    if c.name.startswith("lex"):
        assert clean.all(), "a cut tile in a batch of small tiles"
    # ---- adjacency rows streamed, class tests of the list tiles -------------------------------------------------------------------------------
    adj = [t for t in live if tiles[t, S.T_ADJ]]
    rows_adj, rows_first = np.zeros(S.REGIONS, np.int64), np.zeros(S.REGIONS, np.int64)
    tests = np.zeros((S.REGIONS, 5), dtype=np.int64)
    only_lists = np.ones(S.REGIONS, dtype=bool)
    for t in live:
        if not tiles[t, S.T_ADJ]:
            only_lists[region_of_tile[t]] = False
    if adj:
        hdr = door.list_headers(tiles[adj])
        for t, h in zip(adj, hdr):
            assert h[0] != 0xFFFFFFFF, "a tile streams a list its signature does not have"
            rbeg, rend = S.adj_rows(int(tiles[t, S.T_K]), h[1:8])
            if tiles[t, S.T_FLAGS] & 2:
                assert rbeg <= tiles[t, S.T_S0] <= tiles[t, S.T_S1] <= rend, "a part outside its list's sections"
                rbeg, rend = int(tiles[t, S.T_S0]), int(tiles[t, S.T_S1])
            rows = max(0, rend - rbeg)
            r = region_of_tile[t]
            rows_adj[r] += rows
            if tiles[t, S.T_FLAGS] & 1:
                rows_first[r] += rows
            ke = [0, int(tiles[t, S.T_KEND]) & 0xFF, (int(tiles[t, S.T_KEND]) >> 8) & 0xFF, (int(tiles[t, S.T_KEND]) >> 16) & 0xFF, int(tiles[t, S.T_NQ])]
            for kind in range(1, 5):
                tests[r, kind] += (rows + 3) // 4 * 256 * max(0, ke[kind] - ke[kind - 1])
    assert np.array_equal(rctr[:, S.RC_ADJ].astype(np.int64), rows_adj), "RC_ADJ"
    assert np.array_equal(rctr[:, S.RC_ADJ_FIRST].astype(np.int64), rows_first), "RC_ADJ_FIRST"
    got_tests = rctr[:, S.RC_TESTS:S.RC_TESTS + 10].astype(np.uint64)
    got_tests = (got_tests[:, 0::2] | (got_tests[:, 1::2] << np.uint64(32))).astype(np.int64)
    for r in np.nonzero(only_lists)[0]:
        assert got_tests[r].tolist() == tests[r].tolist(), ("RC_TESTS of region", int(r))
    # ---- per-query counts (the general instances) ---------------------------------------------------------------------------------------------
    if o["count_pairs"]:
        assert res["qpairs"].tolist() == [ex[i].n_counted for i in qo], "qpairs"
    else:
        assert not res["qpairs"].any()
    info = tile_census(c, res, refs, ex, ntiles_of_q, region_of_tile)
    info["clean regions with pairs"] = int((clean & (rctr[:, S.RC_VALID] > 0)).sum())
    info["list-only regions with tests"] = int((only_lists & (got_tests.sum(axis=1) > 0)).sum())
    return rctr[:, S.RC_VALID].astype(np.int64), rc_raw, Counter(got.tolist()), info


def tile_census(c, res, refs, ex, ntiles_of_q, region_of_tile):
    """Classes of the kernel's control flow that follow from the returned tiles, the reference and the model -- conditions on the inputs,
    by arithmetic on the constants of kernels_common.hpp; nothing here is measured.  ex is per input, refs per sorted query.

    Held unreachable: a FOUND run that is empty.  A probe finds a signature only in a slot with a count (`if (!e.w) break` ends the probe at
    an empty slot), and the flat walk's records without entries are the table's paddings, which never match; stage_runs' `n != 0` guards
    against a table that no builder produces."""
    m, o, tiles = c.model, res["opts"], res["tiles"]
    qo = res["q_orig"].astype(np.int64)
    have = Counter()
    cnt = np.bincount(m.lens, minlength=300)
    one_group = ("ANX_SIG_GROUPS", "1") in m.switches
    live = np.nonzero(tiles[:, S.T_NQ] != 0)[0]
    for t in live:
        q0, n, lq, k = (int(tiles[t, x]) for x in (S.T_Q0, S.T_NQ, S.T_LQ, S.T_K))
        if tiles[t, S.T_KIND] == 0 or (ntiles_of_q[q0:q0 + n] != 1).any():
            continue
        es = [ex[i] for i in qo[q0:q0 + n]]
        through = sum(e.n_ref - e.n_lendrop for e in es)       # pairs through the ring pbuf: 64 a round
        if through > S.SCAN_PBUF:
            have["ring wraps"] += 1
        if through % 64:
            have["last ring round below 64"] += 1
        if through >= 128:
            have["two full ring rounds"] += 1
        # the hit list holds one entry per record with a hit in a pass; a tile of <= 32 queries expands it mid-tile when more than
        # SCAN_HITS - 256 wait after a chunk, which adds at most 256: E records hit in all make at least E // SCAN_HITS such expansions,
        # and at most 256 make none.  Records that pass the length test always enter the list.
        hit_ok = set().union(*[{e for e in r.ents.tolist() if abs(int(m.lens[e]) - r.lq) <= r.d} for r in refs[q0:q0 + n]])
        hit_all = set().union(*[set(r.ents.tolist()) for r in refs[q0:q0 + n]])
        if n <= 32 and len(hit_ok) >= 2 * S.SCAN_HITS:
            have["deferred flush at least twice"] += 1
        if n <= 32 and 0 < len(hit_all) <= S.SCAN_HITS - 256:
            have["never a deferred flush"] += 1
        if one_group and not tiles[t, S.T_ADJ]:
            # one group: the signature is the length, a run = every entry of a length, and the tile stages the runs of lq - k .. lq + k
            runs = cnt[max(lq - k, 0):lq + k + 1]
            if (runs > 64).any():
                have["more than 64 ids in a step"] += 1
            if (runs > S.SCAN_MASKW).any():
                have["a run of two windows"] += 1
            if int(runs.sum()) % 64:
                have["the stage ends on a partial row"] += 1
    return have


def tile_stats(res):
    t = res["tiles"]
    t = t[t[:, S.T_NQ] != 0]
    ke = np.stack([t[:, S.T_KEND] & 0xFF, (t[:, S.T_KEND] >> 8) & 0xFF, (t[:, S.T_KEND] >> 16) & 0xFF], axis=1).astype(np.int64)
    bits = t[:, S.T_KIND] != 0
    return dict(t=t, ke=ke, bits=bits, nq=t[:, S.T_NQ].astype(np.int64), adj=t[:, S.T_ADJ] != 0, ball=(t[:, S.T_BALLN] != 0) & (t[:, S.T_ADJ] == 0),
                flat=(t[:, S.T_BALLN] == 0) & (t[:, S.T_ADJ] == 0))


# ---- every batch case under the production arguments --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.BATCH_CASES)
def test_production_instances(doors, name):
    c = S.case(name)
    door = doors(c.model.name)
    res = door.scan(c)
    info = check(c, door, res)[3]
    ts = tile_stats(res)
    sizes = sorted(ts["nq"].tolist())
    need = []
    if name.startswith("lex") or name == "five-bits":
        need += ["clean regions with pairs"]
    if name == "five-bits":   # no cut tile: every region's counters are exact, and regions of list tiles alone have their class tests compared
        assert info["clean regions with pairs"] == int((res["rctr"][:, S.RC_VALID] > 0).sum()) >= 32 and info["list-only regions with tests"] >= 8, info
        need += ["last ring round below 64", "never a deferred flush"]
    if name == "five1-run":
        need += ["ring wraps", "deferred flush at least twice", "last ring round below 64"]
    if name in ("five1-run-noadj", "five1-run-flat"):
        need += ["more than 64 ids in a step", "a run of two windows", "the stage ends on a partial row", "ring wraps"]
    assert all(info[k] for k in need), (need, dict(info))
    if name in ("lex-1", "lex-31", "lex-32"):
        assert sizes == [len(c.queries)]
    if name == "lex-33":
        assert sizes == [1, 32]
    if name == "lex-40-tq64":
        assert sizes == [40]
    if name in S.KEND_CASES:   # ONE tile, kinds 1 and 2, the boundary where the case puts it
        n1, n2 = S.KEND_CASES[name]
        assert sizes == [n1 + n2] and ts["ke"][0].tolist() == [n1, n1 + n2, n1 + n2]
    if name == "lex1-50-tq64":   # two passes, kinds 1 and 2 in the tile, the kind boundary inside a pass
        i = int(np.argmax(ts["nq"]))
        assert 33 <= ts["nq"][i] <= 64 and 0 < ts["ke"][i, 0] < ts["nq"][i]
    if name == "lex-many":
        n = (res["nadj"], res["nbits"], res["nsad"])
        assert len(res["tiles"]) > 256 and max(n) > 64 and any(x % 4 for x in n) and res["nadj"] > 0 and res["nbits"] > 0
        assert ts["ball"].any(), "no tile probes its ball"
        b = ts["t"][ts["ball"]]
        assert (b[:, S.T_LQ] <= 3).any(), "no short query among the probing tiles"
    if name == "five-k3d2":
        assert res["nadj"] > 0 and res["nsad"] > 0, "bit-plane and count-vector tiles in one batch"
        need34 = ts["bits"] & (ts["ke"][:, 1] < ts["nq"])
        assert need34.any() and (ts["bits"] & ~need34).any()
        assert (ts["bits"] & (ts["t"][:, S.T_LQ] > 16)).any() and (ts["bits"] & (ts["t"][:, S.T_LQ] == 16)).any()
    if name == "five1-run":   # kinds 1 .. 4 inside one tile, every boundary present
        k = ts["ke"]
        assert (ts["bits"] & (0 < k[:, 0]) & (k[:, 0] < k[:, 1]) & (k[:, 1] < k[:, 2]) & (k[:, 2] < ts["nq"])).any()
    if name == "five-flat":
        assert res["nadj"] == 0 and (ts["flat"] & ts["bits"]).any() and not (ts["ball"] & ts["bits"]).any()
    if name == "five-noadj":
        assert res["nadj"] == 0 and (ts["ball"] & ts["bits"]).any()
    if name == "five1-run":
        assert res["nadj"] > 0
    if name in ("five1-run-noadj", "five1-run-flat"):
        assert res["nadj"] == 0 and res["nbits"] > 0
    if name == "wide":
        assert res["nadj"] == 0 and res["nbits"] == 0 and res["nsad"] > 64
        assert max(Counter(ts["t"][:, S.T_Q0].tolist()).values()) > 1, "no window split over several waves"


@pytest.mark.parametrize("name", ["lex-40-tq64", "lex-anagrams", "lex1-twins-first-last", "lex1-no-twins", "lex1-all-twins", "lex1-kind-boundary", "lex1-50-tq64", "five-k3d2",
                                  "five-tq64", "five1-run"] + list(S.KEND_CASES))
def test_twins_and_fuse_switches(doors, name):
    """twins 0 against 1 and fuse 0 against 1: the same reference, equal RC_VALID; without the filter every length-compatible pair is written"""
    c = S.case(name)
    door = doors(c.model.name)
    base = check(c, door, door.scan(c))
    for o in (dict(twins=False), dict(fuse=False), dict(fuse=False, twins=False)):
        other = check(c, door, door.scan(c, **o))
        assert np.array_equal(base[0], other[0])
        if o.get("fuse", True):
            assert base[2] == other[2]


@pytest.mark.parametrize("name", ["lex-many", "five-k3d2", "five1-run"])
def test_reservations(doors, name):
    """Growing reservations (chunk_first 32) against flat ones (chunk_first at the cap): the same pairs.  No more slots reserved -- where
    the tiles hold a handful of pairs, which is what the growing sizes are for (lex-many).  It is no invariant of a correct kernel for a
    tile of many pairs: a wave that writes 225 pairs reserves 32 + 64 + 128 + 128 = 352 slots growing and 128 + 128 = 256 flat, so the
    comparison is not made for the dense cases.
    A run that spills across two reservations, by arithmetic: without the filter a bit-plane tile writes every pair of a ring round, 64 a
    round; with every size at 96 the first round leaves 32 slots and the second round's 64 pairs take them and 32 of the next
    reservation.  Chunks of 32 and of 1024 give the same pairs as well."""
    c = S.case(name)
    door = doors(c.model.name)
    grow = check(c, door, door.scan(c, chunk_first=32))
    flat = check(c, door, door.scan(c, chunk_first=1024))
    assert grow[2] == flat[2] and np.array_equal(grow[0], flat[0])
    if name == "lex-many":
        assert (grow[1] <= flat[1]).all() and grow[1].sum() < flat[1].sum()
    spill = check(c, door, door.scan(c, chunk=32, chunk_fused=32, chunk_first=32))
    assert spill[2] == grow[2]
    check(c, door, door.scan(c, chunk=1024, chunk_fused=1024, chunk_first=32))
    if name != "lex-many":
        plain = check(c, door, door.scan(c, fuse=False))
        s96 = check(c, door, door.scan(c, fuse=False, chunk=96, chunk_fused=96, chunk_first=96))
        assert s96[2] == plain[2] and s96[3]["two full ring rounds"], dict(s96[3])


@pytest.mark.parametrize("name", ["five1-run", "wide"])
def test_capacity_below_the_need(doors, name):
    c = S.case(name)
    door = doors(c.model.name)
    full = check(c, door, door.scan(c))
    low = check(c, door, door.scan(c, shift=10), below_capacity=True)
    assert np.array_equal(full[0], low[0]), "RC_VALID does not depend on the capacity"
    assert not low[2] - full[2]


@pytest.mark.parametrize("name", ["five-k3d2", "five-k3d1", "lex1-50-tq64", "five1-run-noadj", "wide"])
def test_general_instances(doors, name):
    """per-query counts on: qpairs is the reference's count; drop_len off: every reference pair is written"""
    c = S.case(name)
    door = doors(c.model.name)
    a = check(c, door, door.scan(c, count_pairs=True))
    b = check(c, door, door.scan(c, count_pairs=True, fuse=False, drop_len=False))
    assert np.array_equal(a[0], b[0])
    assert sum(b[2].values()) == sum(len(r.ents) for r in c.ref)
    check(c, door, door.scan(c, fuse=False, drop_len=False))


def test_want_exact(doors):
    """a batch encoded for StopAtExactMatch: bit 31 on the pairs of the query's exact class, qpairs narrowed to it"""
    c = S.case("five-stop")
    door = doors(c.model.name)
    for o in (dict(count_pairs=True), dict(count_pairs=False), dict(count_pairs=True, drop_len=True)):
        got = check(c, door, door.scan(c, want_exact=True, fuse=False, drop_len=o.pop("drop_len", False), **o))
        assert sum(1 for k in got[2] if k & 2) > 50
    check(c, door, door.scan(c))   # (and as a run without the criterion would scan it)


def test_host_and_device_encoder_give_the_same_pairs(doors):
    d, h = S.case("five-k3d2"), S.case("five-host")
    door = doors("five")
    assert check(d, door, door.scan(d))[2] == check(h, door, door.scan(h))[2]


@pytest.mark.parametrize("name", S.SMALL_CASES)
def test_small_form(doors, name):
    c = S.case(name)
    door = doors(c.model.name)
    res = door.scan(c)
    check(c, door, res)
    t = res["tiles"]
    assert len(t) == c.small_slots * len(c.queries)
    live = t[t[:, S.T_NQ] != 0]
    n = Counter(min(v, 3) for v in Counter(live[live[:, S.T_ADJ] != 0][:, S.T_Q0].tolist()).values())
    if name == "small-600":
        assert n[1], ("a list streamed by one tile", n)
        assert (t[:, S.T_NQ] == 0).any(), "no unused slot"
        assert (live[:, S.T_KIND] == 0).any() and (live[:, S.T_ADJ] != 0).any() and ((live[:, S.T_KIND] != 0) & (live[:, S.T_ADJ] == 0)).any(), "the three bodies in one launch"
    if name == "small-five1":
        assert n[2] and n[3], ("lists cut into 2 and into more parts", n)
    check(c, door, door.scan(c, fuse=False))


def test_the_batch_is_left_as_it_was_and_a_run_counts_the_same_pairs(doors):
    c = S.case("five-k3d2")
    door = doors("five")
    b = door.batch(c)
    b.run()
    rows, st = b.fetch(), b.stats()
    valid = check(c, door, door.scan(c))[0]
    assert int(valid.sum()) == st["n_pairs"]
    check(c, door, door.scan(c, count_pairs=True, fuse=False, drop_len=False))
    b.run()
    st2 = b.stats()
    assert b.fetch() == rows
    for k in ("n_pairs", "n_survivors", "n_selected", "n_class_tests", "n_prefiltered_in_scan", "n_results"):
        assert st[k] == st2[k], k


def test_refusals_launch_nothing(doors):
    c, s, w = S.case("five-k3d2"), S.case("small-64"), S.case("five-stop")
    door = doors("five")
    door.batch(c), door.batch(w)
    L.kernel_timer(True)
    try:
        bad = [(c, dict(shift=9)), (c, dict(shift=26)), (c, dict(chunk=16)), (c, dict(chunk=2048)), (c, dict(chunk_fused=31)), (c, dict(chunk_first=1025)),
               (c, dict(want_exact=True, fuse=False, drop_len=False)),          # the batch was not encoded for StopAtExactMatch
               (c, dict(fuse=True, drop_len=False)), (w, dict(want_exact=True, fuse=True)),
               (s, dict(count_pairs=True)), (s, dict(drop_len=False, fuse=False)), (s, dict(want_exact=True, fuse=False))]
        for case, o in bad:
            with pytest.raises(L.AnxError):
                door.scan(case, **o)
        g, p = door.g, door.params(s)
        for kw in (dict(inputs=[], slots=32), dict(inputs=["ab"] * 4097, slots=8), dict(inputs=["a" * 65], slots=32), dict(inputs=["ab"], slots=4),
                   dict(inputs=["ab"] * 2000, slots=32)):
            with pytest.raises(L.AnxError):
                g.debug_scan_pairs(params=p, **dict(SMALL, **kw))
        other = doors("lex")
        with pytest.raises(L.AnxError):   # a batch of another model
            door.g.debug_scan_pairs(batch=other.batch(S.case("lex-1")), **PROD)
        assert L.kernel_time("k_scan")[1] == 0 and L.kernel_time("k_scan_small")[1] == 0
        door.scan(c)
        door.scan(s)
        assert L.kernel_time("k_scan")[1] == 1 and L.kernel_time("k_scan_small")[1] == 1
    finally:
        L.kernel_timer(False)
