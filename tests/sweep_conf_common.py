"""Shared by test_sweep_confusables_cpu.py and test_gpu_sweep_confusables.py: the twelve candidate patterns (plain, with context,
`^` / `$`, multi-option, one non-ASCII), the oracle's match mask of a pair of texts, and the product of a mask's weights as the
reference multiplies them (ascending pattern order, starting from 1.0)."""
import random

from oracle.sesdiff_twin import Confusable, shortest_edit_script

from pairs_conf_common import edit

PATTERNS = ("-[y]+[i]", "-[c]+[k]", "+[e]", "-[s]", "=[a]-[b]", "-[d]=[e]", "^-[a]", "+[z]$", "-[i|y]+[e]", "+[k|s]", "-[ë]+[e]", "-[e]+[a|i]")
LETTERS = "abcdeiyksz"


def oracle_mask(patterns, a, b, memo=None):
    """bit j = patterns[j] is found in shortest_edit_script(a, b) (oracle/sesdiff_twin.py)"""
    if memo is not None and (a, b) in memo:
        return memo[(a, b)]
    script = shortest_edit_script(a, b)
    m = 0
    for j, p in enumerate(patterns):
        if Confusable(p, 1.0).found_in(script):
            m |= 1 << j
    if memo is not None:
        memo[(a, b)] = m
    return m


def weight_of(mask, weights):
    """src/lib.rs:1743-1752 for the patterns of `mask` under `weights`: 1.0 times each, in list order"""
    w = 1.0
    for j, x in enumerate(weights):
        if (mask >> j) & 1:
            w *= x
    return w


def random_pairs(n, seed, letters=LETTERS + "ë"):
    """(word, edited word) over the letters the patterns speak of, 3-13 letters, 1-3 edits"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        w = "".join(rng.choice(letters) for _ in range(rng.randint(3, 13)))
        out.append((w, edit(rng, w, rng.randint(1, 3), letters)))
    return out
