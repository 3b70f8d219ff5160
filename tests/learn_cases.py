"""Rows for the fold of learn mode that natural queries do not produce on demand: hand-made edge cases and a seeded random generator,
shared by tests/test_learn_cpu.py (host fold vs the restatement) and tests/test_gpu_learn_fold.py (learn.hip vs both).  Plain Python,
no device.

A case yields one or more CALLS, each `(inputs, rows)` with rows[i] = [(vocab_id, dist_score)] of inputs[i], the arguments of
VariantModel.learn_apply_rows / learn_fold_rows_device and of learn_twin.learn_fold.  The ids of a call are resolved against the twin
model AS IT IS WHEN THE CALL IS DRAWN (`Case.calls(m)` is a generator: fold the call into `m` before asking for the next), so a later
call can name entries an earlier one learned.  Every id is below the vocabulary size of that moment: the entry points reject others."""
import os
import random
from typing import Callable, Iterator, List, Sequence, Tuple

import analiticcl_amd as A
from oracle import twin as T

Call = Tuple[List[str], List[List[tuple]]]

LONG = "pneumonoultramicroscopicsilicovolcanoconiosis" * 2  # 90 bytes
# (text, frequency) in id order from 3 on (0..2 are <bos> <eos> <unk>): short and long, multi-byte, byte-prefixes of one another
LEXICON = [("house", 10), ("mouse", 5), ("horse", 3), ("houses", 2), ("hose", 7), ("a", 40), ("ab", 4), ("abc", 6), ("abcd", 1),
           ("separate", 12), ("receive", 9), ("naïve", 2), ("naïveté", 1), ("straße", 3), ("日本", 8), ("日本語", 5), ("é", 2),
           ("éé", 1), ("I", 50), ("x", 1), (LONG[:64], 2), (LONG[:65], 1), ("the", 99), ("them", 20), ("theme", 4), ("then", 30),
           ("quick", 6), ("quack", 2), ("brown", 5), ("crown", 3), ("ice cream", 2), ("icecream", 1)]
# (reference, [(variant, score)]): the weighted variant list of item 7 -- ReferenceFor links that exist before the first call
VARIANT_LIST = [("house", [("hous", 0.75), ("hause", 0.5)]), ("mouse", [("mous", 0.875)]), ("separate", [("seperate", 0.9375)]),
                ("hose", [("house", 0.25)])]
KINDS = ("plain", "variants")


def build_models(alphabet_file: str, tmp_dir, kind: str, device: int = -1):
    """-> (product VariantModel, twin VariantModel) of LEXICON via add_to_vocabulary; kind "variants": plus VARIANT_LIST through
    read_variants.  device >= 0: the product is built and resident there."""
    g = A.VariantModel(alphabet_file, A.Weights(), device=device)
    m = T.VariantModel(T.read_alphabet(alphabet_file))
    for text, freq in LEXICON:
        assert g.add_to_vocabulary(text, freq) == m.add_to_vocabulary(text, freq)
    if kind == "variants":
        path = os.path.join(str(tmp_dir), "learn_cases.variants.tsv")
        with open(path, "w", encoding="utf-8") as f:
            for ref, vs in VARIANT_LIST:
                f.write(ref + "".join(f"\t{v}\t{s!r}" for v, s in vs) + "\n")
        g.read_variants(path)
        m.read_variants(path)
    else:
        assert kind == "plain"
    if device >= 0:
        g.build()
    return g, m


class Case:
    def __init__(self, name: str, draw: Callable[[object], Iterator[Call]]):
        self.name, self._draw = name, draw

    def calls(self, m) -> Iterator[Call]:
        return self._draw(m)

    def __repr__(self):
        return self.name


# ---- hand-made cases: calls written with texts, [(input, [(result text, score)])] --------------------------------------------------
def _resolve(m, call) -> Call:
    return [s for s, _ in call], [[(m.encoder[t], sc) for t, sc in rs] for _, rs in call]


def _hand(name: str, *calls) -> Case:
    def draw(m):
        for call in calls if len(calls) > 1 else calls * 2:  # (a single call is made twice: the second meets what the first left)
            yield _resolve(m, call)
    return Case(name, draw)


def _block_borders():
    """Runs whose members sit on both sides of the 256-input block borders, with nothing but row-less inputs between them (one run:
    +1), and runs broken by one input with rows right at a border (+1 each)."""
    call = [("junk%d" % i, []) for i in range(1030)]
    for i in (254, 255, 256, 258):      # "house": one run across the border at 256 (257 is row-less junk)
        call[i] = ("house", [("hose", 0.5)])
    call[511] = ("mouse", [("house", 0.25)])   # "mouse" | "the" | "mouse" around the border at 512: two runs
    call[512] = ("the", [("them", 0.125)])
    call[513] = ("mouse", [("house", 0.75)])
    for i in (700, 767, 768, 1023, 1024):      # the unknown "qqq": one run over two borders -> frequency 1
        call[i] = ("qqq", [("quick", 0.5)])
    call[1025] = ("brown", [("crown", 0.5)])
    call[1029] = ("qqq", [("quack", 0.5)])     # ... and a second run -> 2
    return call


HAND_CASES = [
    # 1. several rows per input: duplicate (ref, var) pairs inside one input and across inputs with other scores (ReferenceFor keeps
    #    the first: house -> hause 0.9; VariantOf gets all five), the known input's own id between link rows
    _hand("duplicate_pairs",
          [("hauze", [("house", 0.9), ("house", 0.5), ("mouse", 0.3)]), ("hauze", [("house", 0.1)]), ("xx", [("house", 0.7)]),
           ("hauze", [("mouse", 0.8), ("house", 0.2)])]),
    _hand("own_id_between_links",
          [("house", [("mouse", 0.5), ("house", 1.0), ("horse", 0.4), ("house", 0.9), ("mouse", 0.3)]), ("a", [("a", 1.0)]),
           ("a", [("a", 1.0), ("ab", 0.5)])]),
    # 2. a row-less input between two mentions does not break a run (house +1, "recieve" enters with 1); another string with rows
    #    does (mouse +2, "teh" enters with 2)
    _hand("rowless_between_mentions",
          [("house", [("hose", 0.5)]), ("zzzz", []), ("", []), ("house", [("hose", 0.5)]), ("recieve", [("receive", 0.8)]), ("q", []),
           ("recieve", [("receive", 0.7)]), ("mouse", [("house", 0.1)]), ("teh", [("the", 0.6)]), ("mouse", [("house", 0.1)]),
           ("teh", [("then", 0.6)])]),
    _hand("runs_across_block_borders", _block_borders()),
    # 3. (with ANX_LEARN_HASH_BITS narrowed these collide) unknown strings that are prefixes of one another and of known ones,
    #    interleaved: ids in order of first mention, nothing merged
    _hand("prefix_family",
          [("abcde", [("abcd", 0.5)]), ("ab", [("abc", 0.5)]), ("abcdef", [("abcd", 0.4)]), ("b", [("a", 0.1)]), ("abcde", [("abc", 0.3)]),
           ("ééé", [("éé", 0.5)]), ("é", [("éé", 0.2)]), ("abcdef", [("abcd", 0.4)]), ("b", [("ab", 0.1)]), (LONG[:66], [(LONG[:65], 0.9)]),
           (LONG[:64], [(LONG[:65], 0.8)]), (LONG, [(LONG[:64], 0.7)]), ("ééé", [("é", 0.5)]), ("abcde", [("abcd", 0.5)])]),
    # 4. no rows at all; one input
    _hand("no_rows", [("house", []), ("unknown", []), ("", []), ("house", [])]),
    _hand("one_input", [("hous", [("house", 0.5), ("hose", 0.25)])]),
    _hand("one_input_exact", [("house", [("house", 1.0)])]),
    _hand("one_input_no_rows", [("hous", [])]),
    # 6. a second call: "hauze" and "mauze" were learned by the first (now KNOWN, TRANSPARENT: frequency +1, no new entry), the
    #    pair (house, hauze) exists (ReferenceFor not again, VariantOf again), a learned entry as a row's result, its own id
    _hand("second_call",
          [("hauze", [("house", 0.9)]), ("mauze", [("mouse", 0.8), ("house", 0.3)])],
          [("hauze", [("house", 0.1), ("hauze", 1.0), ("mauze", 0.2)]), ("hauzen", [("hauze", 0.6), ("house", 0.5)]),
           ("mauze", [("hauze", 0.4), ("mouse", 0.7)]), ("mauze", [("hauze", 0.35)])],
          [("hauzen", [("hauze", 0.61)]), ("house", [("hauzen", 0.5)])]),
    # 7. links of the variant list (kind "variants"; in the plain model "hous" ... are simply new): house -> hous exists with 0.75,
    #    so ReferenceFor stays and VariantOf is appended; hose -> house likewise, between two known entries
    _hand("links_before_the_call",
          [("hous", [("house", 0.2), ("mouse", 0.1)]), ("house", [("hose", 0.5), ("horse", 0.4)]), ("seperate", [("separate", 0.5)]),
           ("hous", [("house", 0.3)]), ("mous", [("house", 0.3), ("mouse", 0.4)])]),
]

# ---- the random generator --------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 255, 256, 257, 5000)
# unknown strings (the lexicon's own and the variant list's come on top): typos, multi-byte, 1 and 60-90 bytes, prefix chains.
# The empty string is in: the host fold and the restatement agree on it (it becomes an entry like any other).
UNKNOWN = ["hauze", "mauze", "teh", "recieve", "seperate", "hous", "b", "abcde", "abcdef", "ééé", "naïv", "日", "日本語学", "ß", "z",
           LONG[:66], LONG, LONG[:63] + "é", "<unk>", "", "the ", "ice", "ice crea"]


def draw_call(m, n: int, rng: random.Random) -> Call:
    """One random call against the twin's present vocabulary: strings with replacement from a pool of a few dozen (known, unknown,
    learned before), about a third of the inputs without rows, otherwise 1..4 rows whose ids come from a dozen entries and the
    input's own."""
    vocab = [v.text for v in m.decoder]
    learned = vocab[3 + len(LEXICON):]
    pool = rng.sample([t for t, _ in LEXICON], 14) + rng.sample(UNKNOWN, 14) + rng.sample(learned, min(len(learned), 8))
    ids = rng.sample(range(len(vocab)), 10) + [len(vocab) - 1, 0, 2]
    inputs, rows, s = [], [], None
    for _ in range(n):
        if s is None or rng.random() >= 0.3:   # (else: the previous string again)
            s = rng.choice(pool)
        own = m.encoder.get(s)
        rs = []
        if rng.random() >= 1 / 3:
            for _ in range(rng.randint(1, 4)):
                vid = own if own is not None and rng.random() < 0.25 else rng.choice(ids)
                rs.append((vid, rng.random() * rng.choice((1.0, 1.0, 1e-3, 1e-300, 1e300))))
        inputs.append(s)
        rows.append(rs)
    return inputs, rows


def _random(n: int, seed: int) -> Case:
    def draw(m):
        rng = random.Random(1000 * seed + n)
        first = draw_call(m, n, rng)
        yield first
        again = draw_call(m, n, rng)   # (drawn now: it names what the first call learned)
        yield first[0] + again[0], first[1] + again[1]
    return Case(f"random_n{n}_s{seed}", draw)


def all_cases(seeds: Sequence[int] = (1,)) -> List[Case]:
    return HAND_CASES + [_random(n, s) for n in SIZES for s in seeds]
