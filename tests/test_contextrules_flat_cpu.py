"""The flat form of the context rules (csrc/contextrules_flat.hpp: what the device lattice decoder evaluates) against the parsed
patterns (PatternMatch::matches: what the host decoder evaluates), element by element, through the host-only test hook
anx_debug_contextrule_match: random rule sets over a small model with three lexicon files; every vocabulary id, id 0, and lexicon
masks of 0, every single bit and a few combinations."""
import random

import pytest

import analiticcl_amd as A
from analiticcl_amd import _lib as L

TEST_ALPHABET_TSV = "\n".join(f"{c}\t{c.upper()}" for c in "abcdefghijklmnopqrstuvwxyz") + "\n.\t,\n"
LEXICONS = {"amphibians.tsv": ("salamander", "frog", "toad", "newt"), "reptiles.tsv": ("lizard", "snake", "skink", "newt"),
            "birds.tsv": ("wren", "frog", "snake", "owl", "newt")}
WORDS = sorted({w for ws in LEXICONS.values() for w in ws})
MASKS = [0] + [1 << b for b in range(32)] + [3, 5, 6, 7, 0x80000001, 0xFFFFFFFF]


def model(tmp_path):
    m = A.VariantModel("", alphabet_text=TEST_ALPHABET_TSV, device=-1)
    for name, words in LEXICONS.items():
        f = tmp_path / name
        if not f.exists():
            f.write_text("".join(f"{w}\t2\n" for w in words))
        m.read_lexicon(str(f))
    return m


def atom(rng):
    k = rng.randrange(6)
    return ("?", "^", "@" + rng.choice(list(LEXICONS)))[k] if k < 3 else rng.choice(WORDS)


def element(rng):
    """every form parse_pattern accepts: atom, !x, !!x, a|b|c, !a|b, !(a|b), !(!(a|b)), !(!a|b)"""
    k = rng.randrange(8)
    nots = lambda: "!" * rng.choice((0, 0, 1, 2))  # noqa: E731
    if k == 0:
        return atom(rng)
    if k == 1:
        return "!" + atom(rng)
    if k == 2:
        return "!!" + atom(rng)
    items = "|".join(nots() + atom(rng) for _ in range(rng.randrange(2, 5)))
    if k in (3, 4):
        return items
    if k in (5, 6):
        return "!(" + items + ")"
    return "!(!(" + items + "))"


def check_model(m, nrules):
    nvocab = L.lib().anx_model_vocab_size(m.h)
    assert nvocab == len(WORDS) + 3
    n = 0
    for r, length in enumerate(nrules):
        for c in range(length):
            for vid in range(nvocab + 1):  # (one id beyond the vocabulary too)
                for mask in MASKS:
                    a = m.contextrule_element_matches(r, c, vid, mask, flat=False)
                    b = m.contextrule_element_matches(r, c, vid, mask, flat=True)
                    assert a == b, (r, c, vid, hex(mask))
                    n += 1
    return n


def test_flat_elements_equal_parsed_patterns(tmp_path):
    rng = random.Random(20240917)
    total = 0
    for _ in range(200):
        m = model(tmp_path)
        lens = []
        for _r in range(rng.randrange(1, 5)):
            pat = [element(rng) for _ in range(rng.randrange(1, 5))]
            tags, offs = rng.choice((((), ()), (("t",), ()), (("t", "u"), ("0:1", ":"))))
            m.add_contextrule("; ".join(pat), rng.choice((0.5, 0.9, 1.1, 1.5)), list(tags), list(offs))
            lens.append(len(pat))
        total += check_model(m, lens)
    assert total > 100000


def test_named_forms(tmp_path):
    """The nestings the issue names, with their truth tables spelt out."""
    m = model(tmp_path)
    for pat in ("!(!(frog|toad))", "!!frog", "!frog|toad", "!(frog|!@reptiles.tsv)", "^|owl", "!^", "!?"):
        m.add_contextrule(pat, 1.1)
    check_model(m, [1] * 7)
    ids = {w: i for i in range(3, 3 + len(WORDS)) for w in [m.vocab_text(i)]}
    f = lambda r, w, mask: m.contextrule_element_matches(r, 0, ids.get(w, 0), mask, flat=True)  # noqa: E731
    assert f(0, "frog", 1) and f(0, "toad", 1) and not f(0, "owl", 4)        # !(!(frog|toad)) == frog|toad
    assert f(1, "frog", 1) and not f(1, "toad", 1)                             # !!frog == frog
    assert f(2, "toad", 1) and f(2, "owl", 4) and not f(2, "frog", 1)          # !frog|toad
    assert f(3, "snake", 2) and not f(3, "frog", 1) and not f(3, "owl", 4)     # !(frog|!@reptiles) == !frog & @reptiles
    assert f(4, "owl", 4) and f(4, "zzz", 0) and f(4, "frog", 0) and not f(4, "frog", 1)
    assert f(5, "frog", 1) and not f(5, "zzz", 0) and not f(6, "frog", 1)
    with pytest.raises(A.AnxError):
        m.contextrule_element_matches(7, 0, 3, 1)
    with pytest.raises(A.AnxError):
        m.contextrule_element_matches(0, 1, 3, 1, flat=True)
