"""The anx_gold_summary of a list of anx_gold_eval records, in plain Python integers (helper of test_sweep_cpu.py and test_gpu_sweep.py:
a test helper, not the product).  Records are dicts with eval_twin.FIELDS (eval_twin.expected_record) or a numpy structured array of
VariantModel.GOLD_DTYPE."""
import eval_twin as E

RANK_BINS = 64
KEYS = ("n", "gold_known", "reasons", "rank_hist", "rr_fixed", "n_results", "gained_at_1", "lost_at_1")


def as_dicts(records):
    if isinstance(records, (list, tuple)):
        return list(records)
    cols = {k: records[k].tolist() for k in E.FIELDS}
    return [{k: cols[k][i] for k in E.FIELDS} for i in range(len(records))]


def summarize(records, baseline=None):
    """baseline: the records of the same pairs under the first parameter set (None: these ARE the first set's)."""
    recs = as_dicts(records)
    base = recs if baseline is None else as_dicts(baseline)
    assert len(base) == len(recs)
    s = {"n": len(recs), "gold_known": 0, "reasons": [0] * 8, "rank_hist": [0] * RANK_BINS, "rr_fixed": 0, "n_results": 0, "gained_at_1": 0,
         "lost_at_1": 0}
    for r, b in zip(recs, base):
        s["gold_known"] += r["gold_vocab_id"] != E.NONE
        s["reasons"][r["reason"]] += 1
        s["n_results"] += r["n_results"]
        if r["reason"] == E.RANKED:
            assert r["rank"] >= 0
            s["rank_hist"][min(r["rank"], RANK_BINS - 1)] += 1
            s["rr_fixed"] += (1 << 32) // (r["rank"] + 1)
        at1, base1 = r["reason"] == E.RANKED and r["rank"] == 0, b["reason"] == E.RANKED and b["rank"] == 0
        s["gained_at_1"] += at1 and not base1
        s["lost_at_1"] += base1 and not at1
    return s


def of_product(summary):
    """One element of evaluate_sweep_arrays' summaries in the helper's form."""
    return {"n": int(summary["n"]), "gold_known": int(summary["gold_known"]), "reasons": [int(x) for x in summary["reasons"]],
            "rank_hist": [int(x) for x in summary["rank_hist"]], "rr_fixed": int(summary["rr_fixed"]), "n_results": int(summary["n_results"]),
            "gained_at_1": int(summary["gained_at_1"]), "lost_at_1": int(summary["lost_at_1"])}
