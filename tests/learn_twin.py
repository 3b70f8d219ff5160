"""Restatement of learn mode for the tests: VariantModel::learn_variants' fold (src/lib.rs:1102-1129, add_variant_by_id :478-514,
add_to_vocabulary :900-967 with VocabParams::default().with_vocab_type(TRANSPARENT).with_freq_handling(Max)) and the weighted
variant list writers of `analiticcl learn` (src/bin/analiticcl.rs:186-365), on the state of an oracle.twin.VariantModel.

Learned entries are TRANSPARENT and NOT indexed: the twin's build() would index every entry it holds, so they carry indexed=False
(the reference's build() only hashes INDEXED items, src/lib.rs:198)."""
from typing import Dict, List, Sequence, Tuple

from analiticcl_amd.cli import rust_f64


def add_variant_by_id(m, ref_id: int, variant_id: int, score: float) -> bool:
    if variant_id == ref_id:
        return False
    ref = m.decoder[ref_id]
    if ref.variants is None:
        ref.variants = [("ref_for", variant_id, score)]
    elif not any(k == "ref_for" and y == variant_id for k, y, _ in ref.variants):
        ref.variants.append(("ref_for", variant_id, score))
    var = m.decoder[variant_id]
    if var.variants is None:
        var.variants = [("variant_of", ref_id, score)]
    elif not any(k == "variant_of" and y == variant_id for k, y, _ in var.variants):  # sic: the reference compares with variantid
        var.variants.append(("variant_of", ref_id, score))
    return True


def learn_fold(m, inputs: Sequence[str], rows: Sequence[Sequence[tuple]]) -> int:
    """The fold of one learn_variants call: rows[i] = the ranked [(vocab_id, dist_score, ...)] of inputs[i]."""
    count = 0
    prev = None
    for s, rs in zip(inputs, rows):
        for row in rs:
            vid = m.encoder.get(s)
            if vid is not None:
                if prev != s:
                    m.decoder[vid].frequency += 1
            else:
                vid = m.add_to_vocabulary(s, 1, "max", transparent=True, lexicon_index=0)
                m.decoder[vid].indexed = False
            if row[0] != vid:
                if add_variant_by_id(m, row[0], vid, row[1]):
                    count += 1
            prev = s
    return count


VOCAB_INDEXED, VOCAB_LM, VOCAB_TRANSPARENT = 1, 2, 4


def twin_state(m) -> List[tuple]:
    """Per entry: (text, frequency, vocabtype bits without LM, lexindex, [(kind, id, score)])."""
    out = []
    for v in m.decoder:
        vt = (VOCAB_INDEXED if v.indexed else 0) | (VOCAB_TRANSPARENT if v.transparent else 0)
        kinds = [("ReferenceFor" if k == "ref_for" else "VariantOf", y, s) for k, y, s in (v.variants or [])]
        out.append((v.text, v.frequency, vt, v.lexindex, kinds))
    return out


def product_state(g, first: int = 0) -> List[tuple]:
    """The same view of an analiticcl_amd.VariantModel (entries from `first` on)."""
    out = []
    for vid in range(first, g.vocab_size()):
        out.append((g.vocab_text(vid), g.vocab_frequency(vid), g.vocabtype(vid) & ~VOCAB_LM, g.vocab_lexindex(vid), g.variants(vid)))
    return out


def assert_same_state(g, m, first: int = 0) -> None:
    exp = twin_state(m)[first:]
    got = product_state(g, first)
    assert len(got) == len(exp), (len(got), len(exp))
    for k, (a, b) in enumerate(zip(got, exp)):
        assert a == b, (first + k, a, b)


def _refs(m):
    for v in m.decoder:
        refs = [(y, s) for k, y, s in (v.variants or []) if k == "ref_for"]
        if v.variants is not None and refs:
            yield v, refs


def variant_list_tsv(m) -> str:
    """output_weighted_variants_as_tsv without --multi-output."""
    out = []
    for v, refs in _refs(m):
        out.append(v.text)
        for y, s in refs:
            out.append(f"\t{m.decoder[y].text}\t{rust_f64(s)}")
        out.append("\n")
    return "".join(out)


def _esc(s: str) -> str:
    return s.replace('"', '\\"')


def variant_list_json(m) -> str:
    """output_weighted_variants_as_json without --multi-output (trailing commas and all)."""
    out = ["{\n"]
    for v, refs in _refs(m):
        out.append('    "%s": [ \n' % _esc(v.text))
        for y, s in refs:
            t = m.decoder[y]
            out.append('        { "text": "%s", "score": %s, "freq": %d }, \n' % (_esc(t.text), rust_f64(s), t.frequency))
        out.append("    ]\n")
    out.append("}\n")
    return "".join(out)


def variant_list_multi(m, json: bool) -> Tuple[str, Dict[int, str]]:
    """--multi-output: (standard output, {lexicon index: file content}).  TSV picks lexicon i when (lexindex & (1 << i)) == (i << i)
    (Rust precedence), JSON when lexindex & (1 << i) == 1 << i and swaps the score and freq values."""
    stdout, files = [], {}
    if json:
        stdout.append("{\n")
    for v, refs in _refs(m):
        stdout.append('    "%s": [ \n' % _esc(v.text) if json else v.text)
        for y, s in refs:
            t = m.decoder[y]
            for i in range(len(m.lexicons)):
                if json and t.lexindex & (1 << i) == 1 << i:
                    files[i] = files.get(i, "") + '        { "text": "%s",  "score": %d, "freq": %s }, ' % (_esc(t.text), t.frequency, rust_f64(s))
                elif not json and (t.lexindex & (1 << i)) == (i << i):
                    files[i] = files.get(i, "") + f"\t{t.text}\t{rust_f64(s)}\t{t.frequency}\n"
        stdout.append("    ]\n" if json else "\n")
    if json:
        stdout.append("}\n")
    return "".join(stdout), files
