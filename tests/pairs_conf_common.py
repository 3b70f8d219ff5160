"""Shared by test_score_pairs_weighted_cpu.py and test_gpu_score_pairs_weighted.py: the pattern list (confusables10.tsv plus four
added patterns), the hand-made pairs with the weights oracle/confusable_oracle.py gives them, and the random pair generators."""
import os
import random

from analiticcl_amd import synth
from oracle import confusable_oracle as CO
from oracle.sesdiff_twin import Confusable

CONF10 = os.path.join(synth.GOLDEN_DATA, "confusables10.tsv")
ADDED = (("-[ij]+[ÿ]", 1.2), ("-[ſ]+[s]", 1.3), ("^+[ge]=[l]", 0.8), ("-[uu]+[w]$", 1.15))

# (a, b, weight under the 14 patterns)
HAND = (
    ("huys", "huis", 1.1), ("huis", "huys", 1.1), ("cat", "kat", 1.05), ("sien", "zien", 1.05), ("zee", "see", 1.05),
    ("cyrkel", "cirkel", 1.1 * 1.1), ("hebb", "hebbe", 0.95), ("heer", "eer", 0.9), ("vrijheid", "vrÿheid", 1.2),
    ("ſtad", "stad", 1.3), ("loof", "geloof", 0.8), ("vrouuu", "vrouw", 1.15), ("vrouu", "vrouw", 1.0), ("ackte", "akte", 1.0),
    ("aerde", "erde", 1.0), ("huis", "huis", 1.0), ("a", "b", 1.0), ("𝔘nicode", "unicode", 1.0),
    ("é" * 9, "é" * 4 + "a" + "é" * 4, 1.0),
)


def oracle_patterns():
    return CO.read_confusables(CONF10) + [Confusable(s, w) for s, w in ADDED]


def load_patterns(model):
    model.read_confusablelist(CONF10)
    for s, w in ADDED:
        model.add_to_confusables(s, w)


def oracle_weights(pats, pairs):
    """confusable_weight of every pair; equal pairs are computed once"""
    memo = {}
    out = []
    for a, b in pairs:
        if (a, b) not in memo:
            memo[(a, b)] = CO.confusable_weight(pats, a, b)
        out.append(memo[(a, b)])
    return out


def edit(rng, s, n, letters):
    cs = list(s)
    for _ in range(n):
        op = rng.randrange(4)
        if op == 0 and len(cs) > 1:
            del cs[rng.randrange(len(cs))]
        elif op == 1:
            cs.insert(rng.randrange(len(cs) + 1), rng.choice(letters))
        elif op == 2:
            cs[rng.randrange(len(cs))] = rng.choice(letters)
        elif len(cs) > 1:
            p = rng.randrange(len(cs) - 1)
            cs[p], cs[p + 1] = cs[p + 1], cs[p]
    return "".join(cs)


def small_alphabet_pairs(n, seed=11, letters="abcdeiyksz"):
    """words over `letters` of 3-13 letters with 1-3 random edits"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        w = "".join(rng.choice(letters) for _ in range(rng.randint(3, 13)))
        out.append((w, edit(rng, w, rng.randint(1, 3), letters)))
    return out


def lexicon_pairs(words, n, seed=12, letters="iyckszeh"):
    """(lexicon word, the word after 1-3 edits drawn from the letters the patterns speak of)"""
    rng = random.Random(seed)
    return [(w, edit(rng, w, rng.randint(1, 3), letters)) for w in (rng.choice(words) for _ in range(n))]
