"""Conditions on the inputs of tests/test_gpu_score_slots.py, checked without a GPU.

(a) The census: which paths of the scoring kernels (kernels_score.hpp) the pair lists of tests/score_cases.py take, wave by wave, derived
    from the slots and the twin's distances by the conditions written in the kernels.  Every class must be populated under every batch it
    applies to; what cannot be reached is listed with the reason.  Nothing is measured.
(b) Every flagged slot obeys the scan's contract (kernels_scan.hpp, the fused prefilter), recomputed here from the strings.
(c) The pair classes: the (lq, lc) grid, the length borders, the edits the DL forms must get right, symbol codes, case.
(d) The reference of the GPU test, the twin's measures and pair_score, equals the C oracle's on every pair of the cases that lies in the
    oracle's candidate set.

Held unreachable:
  * a query whose kept survivors come from all three kernels (inline, k_score_fast8, k_score_pairs): the inline DL needs the query within
    16 symbols and k_score_pairs (with an inline DL in the batch) an entry beyond 32, more than d <= 3 apart.  Both neighbouring pairs of
    kernels are required instead.  Without the inline DL (D = 0) every pair goes to k_score_pairs.
  * a pair that k_filter_score itself appends to the 8-word kernel's list: with the split prefilter (the default) every selected pair with
    a string of 17..32 symbols and d <= 3 is deferred to k_filter_wide first.  The ANX_FS_SPLIT=0 batch of the GPU test appends them directly.
  * the second unknown code: normalize_to_alphabet maps every unknown character to alphabet.len() + 1; alphabet.len() only exists in the
    anagram hash.  Unknown characters are required on both sides of a pair.
  * the drain rule `nsv >= FS_SURV - 64` in place of `nsv > FS_SURV - 64`: it drains one round early and writes the same records, so no
    output differs; test_queue_capacity_reasoning below pins what the census can say about the rule."""
import random

import pytest

import score_cases as S
from oracle import cwrap as O
from oracle import twin as T

NAMES = list(S.BATCHES)


def _traits(c):
    m = c.model
    return dict(small=m.name == "f", flags=m.bit_planes and not c.stop, D=c.D, dmax=max(c.dq), cut=c.score_threshold > 0.0,
                seg=not c.stop and not m.any_variants)


def required_classes(c):
    t = _traits(c)
    need = ["region_0", "region_63", "region_between", "region_empty", "block_partial_round", "wave_unflagged", "wave_invalid_only",
            "invalid_lane0", "invalid_lane63", "invalid_middle", "form_le8", "form_9_12", "route_lenrej", "route_bandrej", "route_listg"]
    if t["dmax"] <= 3 or c.threshold[0] != "abs":   # (an absolute d >= 4: every query of 13..16 symbols has d > 3 and is not prefiltered)
        need += ["form_13_16"]
    if not t["small"]:
        need += ["region_blocks>1"]
    if t["flags"]:
        need += ["wave_all_flagged", "wave_mixed"]
    if c.stop:
        need += ["route_skipped"]
    if t["D"] > 0:
        need += ["route_inline", "route_listw>list8", "route_listw>bandrej", "kernels_fast8+inline", "kernels_fast8+pairs",
                 "run_start_lane0", "run_end_lane63", "run_of_64", "run_next_wave", "run_other_region", "drain_last_round_only"]
        if t["flags"]:
            need += ["route_short"]
        if not t["small"]:
            need += ["queue_192_then_full", "drain_193_255", "drains>=2_in_block", "runs_64_of_1", "runs_interleaved", "run_next_drain_round",
                     "run_next_block"]
            if t["cut"]:
                need += ["run_below_head", "run_below_tail", "run_below_all"]
            if c.model.have_freq:
                need += ["run_maxfreq_first", "run_maxfreq_last"]
    elif c.threshold[0] != "abs":
        need += ["route_listw>listg"]   # d <= 3 for a string of 17..19 symbols in a batch without the inline DL
    if t["seg"]:
        need += ["seg2_lt", "seg2_eq", "seg2_gt", "seg32_lt", "seg32_gt"] + ([] if t["small"] else ["seg32_eq"])
    return need


@pytest.mark.parametrize("name", NAMES)
def test_every_census_class_is_populated(name):
    c = S.case(name)
    t = S.census(c)
    missing = [k for k in required_classes(c) if t[k] == 0]
    assert not missing, (name, missing)
    assert sum(c.fills) == len(c.slots) <= (2000 if c.model.name == "f" else 40000) and len(c.queries) <= 300 and len(c.model.texts) <= 700
    # the classes that cannot occur do not
    assert t["route_list8"] == 0 and not [k for k in t if k.startswith("kernels_") and k.count("+") > 1]
    if c.D == 0:
        assert not [k for k in t if k.startswith(("run_", "drain", "queue", "kernels_")) and t[k]]
    # the same slots in the smaller blocks the small call uses: every route is still taken, every drain is a last round
    for blk in (256, 512):
        tb = S.census(c, blk=blk)
        assert {k: v for k, v in tb.items() if k.startswith(("route_", "need_"))} == {k: v for k, v in t.items() if k.startswith(("route_", "need_"))}
        assert tb["queue_192_then_full"] == 0 and tb["drain_193_255"] == 0


@pytest.mark.parametrize("name", [n for n in NAMES if S.BATCHES[n][0] in "ade" and not S.BATCHES[n][2]])
def test_short_round_of_byte_rows_queues_beyond_the_querys_d(name):
    """ANX_FS_SPLIT=0 / ANX_FS_PLANES=0 run the short round on byte rows: it tests the batch's D and leaves the query's own d to the drain
    (`has = ld <= d`).  Batches whose queries differ in d must queue pairs that fail there; the symbol-plane round never does."""
    c = S.case(name)
    assert S.census(c, planes=True)["drain_fails_own_d"] == 0
    if c.D >= 2:
        assert S.census(c, planes=False)["drain_fails_own_d"] > 0


def test_queue_capacity_reasoning():
    """FS_SURV = 256 entries, drained above 192.  The census holds waves that reach exactly 192 without a drain and then take 64 more
    (exactly full), and a wave that drains at 193, the smallest fill that does, with a full round behind it: under `nsv > FS_SURV - 63`
    that wave would hold 193 + 64 = 257 entries, one beyond its queue (an out-of-bounds LDS write, which is why that mistake is reasoned
    out here and never run)."""
    for name in ("a-abs2", "a-ratio", "b-abs2", "c-abs3", "d-abs2", "e-abs2"):
        c = S.case(name)
        t = S.census(c)
        assert t["queue_192_then_full"] > 0 and t["drain_at_193_then_full_round"] > 0, name


@pytest.mark.parametrize("name", NAMES)
def test_flagged_slots_obey_the_scans_contract(name):
    c = S.case(name)
    m = c.model
    nflag = 0
    for q, w in c.slots.tolist():
        if q == S.INVALID:
            continue
        assert q < len(c.queries) and (w & 0x3FFFFFF) < len(m.texts)
        if w & S.EXACT:
            assert c.stop
        if w & S.PRE:
            nflag += 1
            s, e = T.normalize_to_alphabet(c.queries[q], m.alphabet), m.norm[w & 0x3FFFFFF]
            d = T.clamp_threshold(c.threshold, len(s), T.MAX_EDIT_DISTANCE)
            assert len(m.alphabet) + 1 <= 32 and not c.stop and not (w & S.EXACT)
            assert len(s) <= 16 and len(e) <= 16 and abs(len(s) - len(e)) <= d <= 3
            assert not S.band_bound_rejects(s, e, d)
            ld = T.damerau_levenshtein(s, e, 12)
            assert ld is None or ld >= abs(len(s) - len(e))
    assert nflag > 100 if (m.bit_planes and not c.stop) else nflag == 0


def test_band_bound_never_rejects_a_pair_within_d():
    """the bound is a necessary condition (kernels_swar.hpp): the expectation of a rejected slot is `no distance`"""
    for name in NAMES:
        c = S.case(name)
        for p in list(c.pairs.values()):
            assert not (p.bandrej and p.ld is not None), (name, c.queries[p.q], c.model.texts[p.e])


@pytest.mark.parametrize("name", NAMES)
def test_pair_classes(name):
    c = S.case(name)
    cv = S.coverage(c)
    grid = [(a, b) for a in range(1, 17) for b in range(1, 17) if abs(a - b) <= 3 and cv[("len", a, b)] == 0]
    assert not grid, grid
    need = ["equal", "ld_eq_d", "ld_eq_d+1", "bandrej", "unk_query", "unk_entry", "top_code", "samecase_false", "upper_query", "upper_entry",
            "repeated", "transposition_first", "transposition_last", "border_16_17", "border_32_33"]
    if max(c.dq) >= 2:
        need += ["transposition", "transposition_with_gap"]
    if c.threshold[0] != "abs":
        need += ["d1", "d2", "d3"]
        if c.model.bit_planes and c.D == 3:
            need += ["d1_in_D3_ld2", "d1_in_D3_ld3"]
    if c.model.any_variants:
        need += ["transparent", "no_rows", "rows>1"]
    if name == "f-abs12":
        need += ["len_240_255", "len_255", "d12"]
    missing = [k for k in need if cv[k] == 0]
    assert not missing, (name, missing)
    if c.model.name == "f":
        assert 240 <= max(len(n) for n in c.model.norm) <= 255


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a-abs3", "a-ratio", "b-abs2", "c-abs3", "d-abs2", "e-abs3", "f-abs12"])
def test_twin_measures_and_score_equal_the_oracles(name):
    c = S.case(name)
    m = c.model
    o = O.OracleModel(alphabet_text=m.alphabet_text())
    o.set_weights(m.weights.ld, m.weights.lcs, m.weights.prefix, m.weights.suffix, m.weights.case)
    for i, w in enumerate(m.texts[:m.nwords]):
        assert o.add(w, m.freqs[i] if m.have_freq else None) == 3 + i
    for ref, text, score in m.variants:
        o.add_variant(3 + ref, text, score, None, True)
    o.build()
    op = O.make_params(("abs", 6), c.threshold, 0, 0.0, 0.0, False, 0.0)
    wanted = {}
    for q, w in c.slots.tolist():
        if q != S.INVALID:
            wanted.setdefault(q, set()).add(w & 0x3FFFFFF)
    rng = random.Random(3)
    npairs = nscores = 0
    for q in rng.sample(sorted(wanted), min(len(wanted), 120)):
        results, pairs, total, _ = o.find_variants(c.queries[q], op, want_pairs=True)
        assert total == len(pairs)
        scores = {}
        for vid, dist, _ in results:
            scores.setdefault(vid, dist)
        for vid, ld, lcs, pre, suf, same in pairs:
            e = vid - 3
            if e not in wanted[q] or e >= len(m.texts) - len(m.transparent_only):
                continue
            p = c.pair(q, e)
            npairs += 1
            if ld < 0:
                assert p.ld is None, (c.queries[q], m.texts[e])
                continue
            assert p.meta == ld | (same << 7) | (lcs << 8) | (pre << 16) | (suf << 24), (c.queries[q], m.texts[e])
            if not m.any_variants:   # (a result row per survivor, its own score)
                assert scores[vid] == p.score, (c.queries[q], m.texts[e])
                nscores += 1
    print(name, "pairs compared:", npairs, "scores:", nscores)
    assert npairs > 300 and (nscores > 100 or m.any_variants)
