"""The greedy coordinate ascent of anx_fit_confusable_weights in Python, over any evaluator of weight assignments: what a person does
today with one evaluate_sweep_confusables call per round.  Counts are (at1, ranked, rr_fixed) triples of ints."""


def key(c, objective):
    return (c[0], c[2]) if objective == "acc1" else (c[2], c[0])


def with_weight(cur, j, w):
    return tuple(w if x == j else v for x, v in enumerate(cur))


def greedy(evaluate, n_patterns, grid, start=None, objective="acc1", max_rounds=16, min_gain=1):
    """evaluate(rows) -> one counts triple per weight row.  Returns weights, rounds [(pattern, grid index, weight, counts)], stop,
    n_trial_rounds, start, final and the trial tables [round][pattern][grid index] (a skipped trial holds the current counts)."""
    assert objective in ("acc1", "mrr")
    cur = tuple(float(x) for x in (start if start is not None else [1.0] * n_patterns))
    rounds, tables, first, final, stop = [], [], None, None, 0
    while True:
        trials = [(j, g) for j in range(n_patterns) for g in range(len(grid)) if grid[g] != cur[j]]
        got = evaluate([cur] + [with_weight(cur, j, grid[g]) for j, g in trials])
        now, table = got[0], [[got[0]] * len(grid) for _ in range(n_patterns)]
        if first is None:
            first = final = now
        best = None
        for (j, g), c in zip(trials, got[1:]):
            table[j][g] = c
            if best is None or key(c, objective) > key(best[2], objective):   # ties: the smallest pattern, then the smallest grid index
                best = (j, g, c)
        tables.append(table)
        if best is None or not key(best[2], objective) > key(now, objective) or key(best[2], objective)[0] - key(now, objective)[0] < min_gain:
            break
        j, g, final = best
        cur = with_weight(cur, j, grid[g])
        rounds.append((j, g, grid[g], final))
        if len(rounds) == max_rounds:
            stop = 1
            break
    return {"weights": cur, "rounds": rounds, "stop": stop, "n_trial_rounds": len(tables), "start": first, "final": final, "tables": tables}
