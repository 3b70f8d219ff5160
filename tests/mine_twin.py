"""The twin side of anx_mine_confusables, shared by test_mine_cpu.py and test_gpu_mine.py: change sites, pattern texts and the table's
order from oracle.sesdiff_twin.shortest_edit_script, the definition; the random pair set both files use; the library's result in the
same shape, so that a test is one `==`."""
import random

from oracle.sesdiff_twin import shortest_edit_script

FIRST, LAST = 1, 2
UNREPRESENTABLE = 1
_scripts = {}


def script(a: str, b: str):
    k = (a, b)
    if k not in _scripts:
        _scripts[k] = shortest_edit_script(a, b)
    return _scripts[k]


def sites_of(a: str, b: str, context: int = 0, anchors: bool = False):
    """[(a_pos, a_len, b_pos, b_len, flags, text, chars)] of the maximal runs of non-`=` instructions, left to right; chars: every
    character between the text's brackets"""
    s = script(a, b)
    out = []
    apos = bpos = 0
    i = 0
    while i < len(s):
        if s[i][0] == "=":
            apos += len(s[i][1])
            bpos += len(s[i][1])
            i += 1
            continue
        j = i
        while j < len(s) and s[j][0] != "=":
            j += 1
        first, last = i == 0, j == len(s)
        text = "^" if anchors and first else ""
        chars = ""
        if context and i > 0:
            text += "=[" + s[i - 1][1][-context:] + "]"
            chars += s[i - 1][1][-context:]
        a_len = b_len = 0
        for op, t in s[i:j]:
            text += f"{op}[{t}]"
            chars += t
            if op == "-":
                a_len += len(t)
            else:
                b_len += len(t)
        if context and j < len(s):
            text += "=[" + s[j][1][:context] + "]"
            chars += s[j][1][:context]
        if anchors and last:
            text += "$"
        out.append((apos, a_len, bpos, b_len, (FIRST if first else 0) | (LAST if last else 0), text, chars))
        apos += a_len
        bpos += b_len
        i = j
    return out


def twin_result(pairs, counts=None, context: int = 0, anchors: bool = False):
    """(table, site_off, sites): table = [(text, count, sites, flags)] in the issue's order; sites = [(pair, a_pos, a_len, b_pos, b_len,
    pattern, flags)] pair by pair, left to right"""
    acc = {}
    flat = []
    off = [0]
    for p, (a, b) in enumerate(pairs):
        w = 1 if counts is None else int(counts[p])
        for st in sites_of(a, b, context, anchors):
            text = st[5]
            e = acc.setdefault(text, [0, 0, 0])
            e[0] += w
            e[1] += 1
            if any(c in "[]|" for c in st[6]):
                e[2] = UNREPRESENTABLE
            flat.append((p,) + st[:6])
        off.append(len(flat))
    order = sorted(acc, key=lambda t: (-acc[t][0], -acc[t][1], t.encode("utf-8")))
    index = {t: k for k, t in enumerate(order)}
    table = [(t, acc[t][0], acc[t][1], acc[t][2]) for t in order]
    sites = [(p, ap, al, bp, bl, index[text], fl) for p, ap, al, bp, bl, fl, text in flat]
    return table, off, sites


def lib_result(r, with_sites=True):
    """mine_confusables_arrays' dict in twin_result's shape"""
    off, text = r["text_off"].tolist(), r["text"]
    table = [(text[off[k]:off[k + 1]].decode("utf-8"), c, s, f)
             for k, (c, s, f) in enumerate(zip(r["count"].tolist(), r["sites"].tolist(), r["flags"].tolist()))]
    if not with_sites:
        return table
    st = r["site"]
    sites = list(zip(*(st[k].tolist() for k in ("pair", "a_pos", "a_len", "b_pos", "b_len", "pattern", "flags"))))
    return table, r["site_off"].tolist(), sites


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


LETTERS = "abcdefghijklmnopqrstuvwxyzéëïö"


def random_pairs(eng_words, nld_words, n, seed=2024):
    """(edited word, word): one to three random edits of words of the two golden lexicons, half of the pairs from each; and per-pair
    counts 0..4"""
    rng = random.Random(seed)
    pairs, counts = [], []
    for k in range(n):
        w = rng.choice(eng_words if k % 2 == 0 else nld_words)
        pairs.append((edit(rng, w, rng.randint(1, 3), LETTERS), w))
        counts.append(rng.randrange(5))
    return pairs, counts


GRID = [(c, anc) for c in (0, 1, 2) for anc in (False, True)]
