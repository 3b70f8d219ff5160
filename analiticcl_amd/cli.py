"""`python -m analiticcl_amd query|search|learn|score|evaluate|mine|sweep ...` -- the `analiticcl query` / `search` / `learn` command line
(/root/reference/src/bin/analiticcl.rs) on top of the MI355X engine.

Same option names and defaults (note the CLI's own weight defaults 0.5/0.125/0.125/0.125/0.125, bin:760-800, and
k=3 d=2 n=10, bin:800-817), same TSV / JSON output (bin:21-187).  `query` reads one input per line and runs every
`--batch-size` lines as ONE device batch (the reference: 1000-line rayon batches, bin:416-448); `search` groups lines
into texts like bin:561-636 and decodes them with find_all_matches.  `learn` (bin:484-553) reads the whole input, runs
`--iterations` rounds of learn_variants over it (`--strict`: one string per line, find_variants; otherwise one text per line,
find_all_matches) and writes the weighted variant list (bin:186-365; `-O`: one file per lexicon, with the reference's selection
and field quirks).  `score` has no counterpart in the reference's binary: it reads `a<TAB>b` lines and writes the model's measures
for each pair (score_pairs: the reference's public distance functions, src/distance.rs:101-231, and the score of src/lib.rs:1433-1452); `--weighted` adds the pair's confusable weight under `--confusables`
(src/lib.rs:1733-1756) and score * weight, the dist_score a ranked row carries on such a model.
`evaluate` has none either: it reads `input<TAB>gold` lines, takes the model and parameter options of `query`, and writes per pair the
1-based rank of gold among the ranked variants (`-`: not there), the top variant, gold's score, the pair's edit distance and the stage
that lost a gold that is not ranked (evaluate_arrays); the summary (accuracy@1, MRR, count per reason) goes to stderr or `--summary-json`.
`mine` has none either: it reads `observed<TAB>correct[<TAB>count]` lines (an --errors list, the gold file of `evaluate`, pairs taken from a
learned variant list) and writes the table of the change sites of their edit scripts in confusable-list notation, `pattern<TAB>count<TAB>sites`
(mine_confusables; `--context N`, `--anchors`); `--as-confusables W --min-count N` writes the list `--confusables` reads instead.
`sweep` has none either: it reads the `input<TAB>gold` lines of `evaluate` and a `--grid` of parameter sets (a TSV whose header names
columns among `k d n t T s freq-weight`; every further line is one set in the syntax of those options, absent columns take the command
line's value, the first set is the baseline) and writes one TSV line per set (evaluate_sweep: the set's seven parameters, pairs,
accuracy@1, mrr, ranked share, the eight reason counts, gained@1 / lost@1 against the first set, mean list length).  A grid that also names
any of `w-ld w-lcs w-prefix w-suffix w-case` is a weight grid (evaluate_sweep_weights: absent weight columns take `--weight-*`, the five
weights are printed behind the seven parameters).  `sweep --candidates LIST.tsv --candidate-weights 1.1,0.9` needs no grid: LIST.tsv is a
confusable list (what `mine --as-confusables` writes; its weight column is ignored) of at most 64 candidate patterns, and under the
command line's parameters the output is one TSV line per set (evaluate_sweep_confusables) -- first the baseline with every candidate
off, then one per (pattern, weight) with only that pattern on: pattern, weight, accuracy@1, mrr, gained@1 / lost@1 against the baseline,
the eight reason counts; `--early-confusables` weights before pruning.  With `--fit` the candidates' weights are fitted instead
(fit_confusables: greedy coordinate ascent over `--candidate-weights`, late confusables only; `--fit-objective acc1|mrr`, `--fit-rounds`,
`--fit-min-gain`): the start line (`-`), one line per accepted round -- pattern, weight, accuracy@1, mrr, ranked pairs -- and a `# stop:`
line; `--fit-output OUT.tsv` writes the fitted confusable list.
Not mirrored: index mode,
--interactive buffering semantics (output is flushed per batch).  `--progress` prints the reference's "@ N - processing speed
was R items per second" lines to stderr after every batch (bin:638-654).  `--unicode-offsets` is accepted and, as in the reference
(the flag is looked up under the wrong name, bin:1175), has no effect; `--allow-overlap`, `--lm-order` and `--weight-context` are
accepted and ignored: the reference parses them into SearchParameters fields whose consumers are commented out or absent
(src/lib.rs:1905-1907).  `--debug` / `-D` may stand before or after the mode."""
import argparse
import sys
from decimal import Decimal
from typing import List, Optional

from ._lib import GOLD_REASONS
from .model import SearchParameters, VariantModel, VocabParams, Weights


def rust_f64(x: float) -> str:
    """Rust's `{}` for f64: shortest round-trip digits, never an exponent, no trailing `.0`."""
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    s = format(Decimal(repr(x)), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s if s not in ("", "-") else "0"


def _threshold(v: str):
    """DistanceThreshold::from_str (src/types.rs:85-108): "r;limit", integer, or ratio."""
    if ";" in v:
        r, l = v.split(";", 1)
        return (float(r), int(l))
    try:
        return int(v)
    except ValueError:
        return float(v)


def _esc(s: str) -> str:
    return s.replace('"', '\\"')


EXPLAIN_KEYS = ("ld", "lcs", "prefixlen", "suffixlen", "samecase", "anagram_distance", "len_input", "len_entry", "unweighted_score")


def _explain_value(v: dict, k: str) -> str:
    return rust_f64(v[k]) if k == "unweighted_score" else ("true" if v[k] else "false") if k == "samecase" else str(v[k])


def tsv_line(inp: str, variants: Optional[List[dict]], offset=None, output_lexmatch=False, explain=False) -> str:
    """output_matches_as_tsv / output_result_as_tsv (bin:21-76); `variants` already has the selected one first.
    explain (query --explain, variants from explain_variants): after every variant's score the columns EXPLAIN_KEYS and the text of
    the scored entry (empty unless the row was reached through a variant list)."""
    out = [inp]
    if offset is not None:
        out.append(f"\t{offset[0]}:{offset[1]}")
    for v in variants or []:
        out.append(f"\t{v['text']}\t{rust_f64(v['score'])}\t")
        if explain:
            out.append("\t".join([_explain_value(v, k) for k in EXPLAIN_KEYS] + [v.get("scored", "")]) + "\t")
        if output_lexmatch:
            out.append('\t"' + ";".join(v["lexicons"]) + '"')
    return "".join(out)


def json_item(inp: str, variants: Optional[List[dict]], seqnr: int, offset=None, output_lexmatch=False,
              tag=(), tag_seqnr=(), explain=False) -> str:
    """output_matches_as_json / output_result_as_json (bin:78-187).  explain: the keys EXPLAIN_KEYS (and "scored") in every variant."""
    out = ["    ," if seqnr > 1 else "    ", '{ "input": "%s"' % _esc(inp)]
    if offset is not None:
        out.append(f', "begin": {offset[0]}, "end": {offset[1]}')
    if tag:  # bin:99-121
        out.append(', "tag": [%s], "seqnr": [ %s]' % (",".join('"%s"' % t for t in tag), ",".join(str(n) for n in tag_seqnr)))
    if variants is None:
        out.append(" }\n")
        return "".join(out)
    out.append(', "variants": [ \n')
    items = []
    for v in variants:
        s = '        { "text": "%s", "score": %s, "dist_score": %s, "freq_score": %s' % (
            _esc(v["text"]), rust_f64(v["score"]), rust_f64(v["dist_score"]), rust_f64(v["freq_score"]))
        if "via" in v:
            s += ', "via": "%s"' % _esc(v["via"])
        if explain:
            s += "".join(', "%s": %s' % (k, _explain_value(v, k)) for k in EXPLAIN_KEYS)
            if "scored" in v:
                s += ', "scored": "%s"' % _esc(v["scored"])
        if output_lexmatch:
            s += ', "lexicons": [ %s ]' % ", ".join('"%s"' % _esc(x) for x in v["lexicons"])
        items.append(s + " }")
    out.append(",\n".join(items))
    out.append("\n    ] }\n")
    return "".join(out)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m analiticcl_amd", description=__doc__.split("\n\n")[0])
    p.add_argument("mode", choices=["query", "search", "learn", "score", "evaluate", "mine", "sweep"])
    p.add_argument("files", nargs="*", help="input files (default: standard input)")
    p.add_argument("--lexicon", "-l", action="append", default=[])
    p.add_argument("--variants", "-V", action="append", default=[])
    p.add_argument("--errors", "-E", action="append", default=[])
    p.add_argument("--alphabet", "-a", required=True)
    p.add_argument("--confusables", "-C", action="append", default=[])
    p.add_argument("--early-confusables", action="store_true")
    p.add_argument("--contextrules", "-R", action="append", default=[])
    p.add_argument("--lm", action="append", default=[])
    p.add_argument("--output-lexmatch", action="store_true")
    p.add_argument("--json", "-j", action="store_true")
    p.add_argument("--stop-exact", "-s", action="store_true")
    p.add_argument("--score-threshold", "-t", type=float, default=0.25)
    p.add_argument("--cutoff-threshold", "-T", type=float, default=2.0)
    p.add_argument("--freq-ranking", "-F", type=float, default=None)
    p.add_argument("--weight-ld", type=float, default=0.5)
    p.add_argument("--weight-lcs", type=float, default=0.125)
    p.add_argument("--weight-prefix", type=float, default=0.125)
    p.add_argument("--weight-suffix", type=float, default=0.125)
    p.add_argument("--weight-case", type=float, default=0.125)
    p.add_argument("--max-anagram-distance", "-k", default="3")
    p.add_argument("--max-edit-distance", "-d", default="2")
    p.add_argument("--max-matches", "-n", type=int, default=10)
    p.add_argument("--unicode-offsets", "-u", action="store_true")
    p.add_argument("--per-line", action="store_true")
    p.add_argument("--retain-linebreaks", action="store_true")
    p.add_argument("--max-ngram-order", "-N", type=int, default=3)
    p.add_argument("--max-seq", "-Q", type=int, default=250)
    p.add_argument("--weight-lm", type=float, default=1.0)
    p.add_argument("--weight-variant-model", type=float, default=3.0)
    p.add_argument("--weight-contextrules", type=float, default=1.0)
    p.add_argument("--batch-size", type=int, default=100000, help="query mode: lines per device batch")
    p.add_argument("--weighted", action="store_true", help="score mode: two more columns / keys, weight (the confusable weight of the pair under --confusables) and weighted_score = score * weight")
    p.add_argument("--explain", action="store_true", help="query mode: with every variant its edit distance, common substring / prefix / suffix, case flag, "
                                                           "anagram distance, lengths and unweighted score (and the scored entry of a row reached through a variant list)")
    p.add_argument("--context", type=int, default=0, help="mine mode: code points (0..8) of the neighbouring identities that become part of a pattern")
    p.add_argument("--anchors", action="store_true", help="mine mode: `^` / `$` on a pattern whose site begins / ends the edit script")
    p.add_argument("--as-confusables", type=float, default=None, metavar="W",
                   help="mine mode: write a confusable list (`pattern<TAB>W`) of the representable patterns instead of the table")
    p.add_argument("--min-count", type=int, default=1, help="mine mode, with --as-confusables: only patterns counted at least this often")
    p.add_argument("--summary-json", default=None, help="evaluate mode: write the summary as JSON to this file instead of as text to standard error; "
                                                        "sweep mode: write the summaries as JSON to this file as well")
    p.add_argument("--grid", default=None, help="sweep mode: TSV file of parameter sets; the header names columns among `k d n t T s freq-weight` (and `w-ld w-lcs w-prefix w-suffix w-case`: a weight grid), every further "
                                                "line is one set in the syntax of those options; the first set is the baseline")
    p.add_argument("--candidates", default=None, metavar="LIST.tsv",
                   help="sweep mode: a confusable list of candidate patterns (at most 64; the weight column is ignored): every candidate is tried alone at every --candidate-weights value")
    p.add_argument("--candidate-weights", default=None, metavar="W,W,..", help="sweep mode, with --candidates: the weights to try, comma-separated (each finite, above 0)")
    p.add_argument("--fit", action="store_true",
                   help="sweep mode, with --candidates: fit the candidates' weights on the device by greedy coordinate ascent over --candidate-weights (late confusables only) "
                        "instead of printing the table: the start line, one line per accepted round, the stop reason")
    p.add_argument("--fit-objective", choices=("acc1", "mrr"), default="acc1", help="sweep --fit: what a round improves, accuracy@1 (ties by MRR) or MRR (ties by accuracy@1)")
    p.add_argument("--fit-rounds", type=int, default=16, help="sweep --fit: accepted rounds at most (1..256)")
    p.add_argument("--fit-min-gain", type=float, default=None, metavar="G",
                   help="sweep --fit: the least gain a round must bring, in pairs (acc1, default 1) or in reciprocal rank summed over the pairs (mrr, default 0: any improvement)")
    p.add_argument("--fit-output", default=None, metavar="OUT.tsv", help="sweep --fit: write the fitted confusable list (`pattern<TAB>weight`, the patterns at 1.0 left out) to this file")
    p.add_argument("--index-cache", default=None, help="image of the built model: loaded if the file exists (lexicons are then not read), written after build() otherwise")
    p.add_argument("--device", type=int, default=None)
    p.add_argument("--single-thread", "-1", action="store_true", help="accepted for compatibility, no effect")
    p.add_argument("--interactive", "-x", action="store_true", help="one device batch per input line")
    p.add_argument("--progress", action="store_true", help="Show progress (items per second on stderr after every batch)")
    p.add_argument("--debug", "-D", type=int, default=0, help="debug level 0-4 (passed to the model)")
    p.add_argument("--allow-overlap", action="store_true", help="accepted for compatibility, no effect (as in the reference)")
    p.add_argument("--lm-order", "-L", type=int, default=3, help="accepted for compatibility: the LM is a bigram model (src/lib.rs:2580-2674)")
    p.add_argument("--weight-context", type=float, default=0.0, help="accepted for compatibility, no effect (as in the reference)")
    p.add_argument("--devices", default=None, help="comma-separated HIP device ordinals: one replica of the lexicon per device, batches are "
                                                    "sharded over them inside this process (the reference's rayon fan-out, bin:445-448)")
    p.add_argument("--iterations", "-I", type=int, default=1,
                   help="learn mode: the number of iterations to use for learning (more iterations cover more edit distance)")
    p.add_argument("--multi-output", "-O", action="store_true",
                   help="learn mode: write one weighted variant list per input lexicon (<lexicon>.variants.tsv / .json) instead of "
                        "to standard output")
    p.add_argument("--strict", action="store_true",
                   help="learn mode: the input is itself a list or lexicon, one item per line (find_variants instead of search)")
    return p


class Progress:
    """show_progress (bin:638-654)"""

    def __init__(self, enabled: bool):
        import time
        self.enabled, self.last, self.clock = enabled, time.time(), time.time

    def show(self, seqnr: int, batchsize: int) -> None:
        if not self.enabled:
            return
        now = self.clock()
        elapsed_ms = int((now - self.last) * 1000)
        if now <= self.last or seqnr <= 1 or elapsed_ms <= 0:
            sys.stderr.write(f"@ {seqnr}\n")
        else:
            sys.stderr.write(f"@ {seqnr} - processing speed was {batchsize / (elapsed_ms / 1000.0):.0f} items per second\n")
        self.last = now


def _index_tag(a) -> str:
    """What --index-cache binds the image to: every resource file that enters build() (kind, path, size, SHA-256 of the content),
    in the order given.  (The vocabulary parameters are the CLI's fixed defaults per kind, so they are not part of the tag.)"""
    import hashlib
    import json
    import os
    items = []
    for kind in ("lexicon", "variants", "errors", "lm"):
        for f in getattr(a, kind):
            h = hashlib.sha256()
            with open(f, "rb") as fh:
                for chunk in iter(lambda: fh.read(1 << 20), b""):
                    h.update(chunk)
            items.append([kind, os.path.abspath(f), os.path.getsize(f), h.hexdigest()])
    flags = ("--lexicon", "-l", "--variants", "-V", "--errors", "-E")
    order = [t.split("=", 1)[0] for t in sys.argv if t in flags or any(t.startswith(f + "=") for f in flags if f.startswith("--"))]
    return json.dumps({"resources": items, "argv_order": order}, sort_keys=True)


def make_model(a) -> VariantModel:
    weights = Weights(ld=a.weight_ld, lcs=a.weight_lcs, prefix=a.weight_prefix, suffix=a.weight_suffix, case=a.weight_case)
    devices = [int(x) for x in a.devices.split(",")] if a.devices else None
    model = VariantModel(a.alphabet, weights, debug=a.debug, device=a.device, devices=devices)
    import os
    # The image is bound to what it was built from: alphabet (checked by the library) and the resource files in command-line
    # order with their sizes and content hashes -- an edited lexicon, another variant list or LM makes the tag differ and the
    # model is rebuilt (the reference rebuilds on every start, so it can never be stale)
    tag = _index_tag(a) if a.index_cache else None
    if a.index_cache and os.path.exists(a.index_cache) and VariantModel.index_tag_of(a.index_cache) == tag:
        try:
            model.load_index(a.index_cache)
            loaded = True
        except Exception as e:  # noqa: BLE001 -- another layout (e.g. signature groups), another alphabet, a damaged file: rebuild
            sys.stderr.write(f"[analiticcl_amd] {a.index_cache}: {e}; rebuilding the index\n")
            loaded = False
            model = VariantModel(a.alphabet, weights, debug=a.debug, device=a.device, devices=devices)
        if loaded:
            for filename in a.confusables:
                model.read_confusablelist(filename)
            for filename in a.contextrules:
                model.read_contextrules(filename)
            if a.early_confusables:
                model.set_confusables_before_pruning()
            return model
    # resources in command-line order (bin:1020-1068): lexicons, variant lists, error lists
    order = []
    argv = sys.argv
    for flagset, kind in ((("--lexicon", "-l"), "lexicon"), (("--variants", "-V"), "variants"), (("--errors", "-E"), "errors")):
        values = iter(getattr(a, kind))
        for i, tok in enumerate(argv):
            if tok in flagset or any(tok.startswith(f + "=") for f in flagset if f.startswith("--")):
                try:
                    order.append((i, kind, next(values)))
                except StopIteration:
                    pass
    if len(order) != len(a.lexicon) + len(a.variants) + len(a.errors):  # called programmatically: fall back to kind order
        order = [(0, "lexicon", f) for f in a.lexicon] + [(1, "variants", f) for f in a.variants] + [(2, "errors", f) for f in a.errors]
    for _i, kind, filename in sorted(order, key=lambda t: t[0]):
        if kind == "lexicon":
            model.read_lexicon(filename)
        else:
            model.read_variants(filename, transparent=(kind == "errors"))
    for filename in a.lm:
        model.read_vocabulary(filename, VocabParams(vocabtype="LM"))
    for filename in a.confusables:
        model.read_confusablelist(filename)
    for filename in a.contextrules:  # bin:1097-1109
        model.read_contextrules(filename)
    model.build()
    if a.index_cache:
        model.set_index_tag(tag)
        model.save_index(a.index_cache)
    if a.early_confusables:
        model.set_confusables_before_pruning()
    return model


def make_params(a) -> SearchParameters:
    if a.cutoff_threshold < 1.0 and a.cutoff_threshold != 0.0:
        sys.stderr.write("ERROR: Cutoff-threshold must be >= 1.0, or 0 to disable\n")
        sys.exit(2)
    return SearchParameters(max_anagram_distance=_threshold(a.max_anagram_distance),
                            max_edit_distance=_threshold(a.max_edit_distance), max_matches=a.max_matches,
                            score_threshold=a.score_threshold, cutoff_threshold=a.cutoff_threshold,
                            stop_criterion=a.stop_exact, freq_weight=a.freq_ranking if a.freq_ranking is not None else 0.0,
                            max_ngram=a.max_ngram_order, max_seq=a.max_seq, lm_weight=a.weight_lm,
                            variantmodel_weight=a.weight_variant_model, contextrules_weight=a.weight_contextrules,
                            unicodeoffsets=False)  # the reference reads the flag under the wrong name: inert (bin:1175)


def _lines(files):
    streams = [open(f, encoding="utf-8", newline="") for f in files] or [sys.stdin]
    for st in streams:
        for line in st:
            yield line[:-1] if line.endswith("\n") else line


def run_query(model, params, a, out) -> None:
    seqnr = 0
    batch: List[str] = []
    progress = Progress(a.progress)

    def flush():
        nonlocal seqnr
        if not batch:
            return
        # one device batch, formatted natively (anx_format_query_output = tsv_line / json_item of this module)
        if getattr(a, "explain", False):  # the measures behind every row (explain_variants), formatted here
            for i, r in enumerate(model.explain_variants(batch, params)):
                out.write(json_item(r["input"], r["variants"], seqnr + 1 + i, output_lexmatch=a.output_lexmatch, explain=True) if a.json
                          else tsv_line(r["input"], r["variants"], output_lexmatch=a.output_lexmatch, explain=True) + "\n")
        else:
            out.write(model.query_output(batch, params, a.json, a.output_lexmatch, seqnr + 1))
        seqnr += len(batch)
        out.flush()
        progress.show(seqnr, len(batch))  # bin:477-479
        batch.clear()

    limit = 1 if a.interactive else max(1, a.batch_size)
    for line in _lines(a.files):
        batch.append(line)
        if len(batch) >= limit:
            flush()
    flush()


def run_search(model, params, a, out) -> None:
    """process_search (bin:561-636): consecutive lines form one text up to an empty line (or one text per line)."""
    seqnr = 0
    progress = Progress(a.progress)
    MAX_BATCHSIZE_SEARCH = 100  # bin:17
    lines = _lines(a.files)
    eof = False
    while not eof:
        text = ""
        for i in range(MAX_BATCHSIZE_SEARCH):
            try:
                inp = next(lines)
            except StopIteration:
                eof = True
                break
            if i > 0:
                text += "\n" if a.retain_linebreaks else " "
            text += inp
            if inp == "" or a.per_line:
                break
            if text == "":
                break
        # one text through find_all_matches, formatted natively (anx_format_search_output = tsv_line / json_item above)
        text_out, nmatches = model.search_output([text], params, a.json, a.output_lexmatch, seqnr + 1) if text else ("", 0)
        if seqnr > 0 and nmatches:
            out.write("\n")
        out.write(text_out)
        seqnr += nmatches
        out.flush()
        progress.show(seqnr, nmatches)  # bin:631-634


def _all_lines(files) -> List[str]:
    """BufRead::lines over the whole input: without the "\n" / "\r\n" line ends."""
    out = []
    for line in _lines(files):
        out.append(line[:-1] if line.endswith("\r") else line)
    return out


def _variant_refs(model):
    """(item text, [(variant text, score, freq, lexindex)]) of every item with ReferenceFor links, in vocabulary order."""
    for vid in range(model.vocab_size()):
        refs = [(t, sc) for kind, t, sc in model.variants(vid) if kind == "ReferenceFor"]
        if refs:
            yield model.vocab_text(vid), [(model.vocab_text(t), sc, model.vocab_frequency(t), model.vocab_lexindex(t)) for t, sc in refs]


def write_multi_output(model, json: bool, out) -> None:
    """output_weighted_variants_as_tsv / _as_json with --multi-output (bin:197-233, 271-315): standard output gets the item lines,
    <lexicon>.variants.{tsv,json} the variants.  Kept as the reference writes them: the TSV picks lexicon i when
    `lexindex & (1 << i) == i << i` (Rust precedence: bit 0 clear selects file 0, bit 1 set file 1, never a file >= 2), the JSON
    puts the frequency under "score" and the score under "freq", with no line ends in the files."""
    files = {}

    def fh(i):
        if i not in files:
            files[i] = open(f"{model.lexicons[i]}.variants.{'json' if json else 'tsv'}", "w", encoding="utf-8", newline="")
        return files[i]

    try:
        if json:
            out.write("{\n")
        for text, refs in _variant_refs(model):
            out.write('    "%s": [ \n' % _esc(text) if json else text)
            for vtext, score, freq, lexindex in refs:
                for i in range(len(model.lexicons)):
                    if json and lexindex & (1 << i) == 1 << i:
                        fh(i).write('        { "text": "%s",  "score": %d, "freq": %s }, ' % (_esc(vtext), freq, rust_f64(score)))
                    elif not json and (lexindex & (1 << i)) == (i << i):
                        fh(i).write(f"\t{vtext}\t{rust_f64(score)}\t{freq}\n")
            out.write("    ]\n" if json else "\n")
        if json:
            out.write("}\n")
    finally:
        for f in files.values():
            f.close()


def run_learn(model, params, a, out) -> None:
    """process_learn (bin:484-553): all lines at once, up to --iterations rounds (each rebuilds the model), then the variant list."""
    lines = _all_lines(a.files)
    for i in range(a.iterations):
        count = model.learn_variants(lines, params, strict=a.strict, auto_build=True)
        if a.strict:
            sys.stderr.write(f"(Iteration #{i + 1}: learned {count} variants (out of a total of {len(lines)} input strings)\n")
        else:
            sys.stderr.write(f"(Iteration #{i + 1}: learned {count} variants\n")
        if count == 0 and i + 1 < a.iterations:
            sys.stderr.write("(Halting further iterations)\n")
            break
    if a.multi_output:
        write_multi_output(model, a.json, out)
    else:
        out.write(model.variant_list_output(a.json))
    out.flush()


def score_tsv_line(a: str, b: str, r: dict) -> str:
    """a, b, score, ld, lcs, prefix, suffix, samecase; a pair with a status (an empty side, more than 255 symbols) keeps its two
    strings and gets empty measure columns.  A weighted record (--weighted) has two more columns: weight, weighted_score."""
    weighted = "weight" in r
    if r["status"]:
        return f"{a}\t{b}\t\t\t\t\t\t" + ("\t\t" if weighted else "")
    cols = [a, b, rust_f64(r["score"]), str(r["ld"]), str(r["lcs"]), str(r["prefixlen"]), str(r["suffixlen"]),
            "1" if r["samecase"] else "0"]
    if weighted:
        cols += [rust_f64(r["weight"]), rust_f64(r["weighted_score"])]
    return "\t".join(cols)


def score_json_item(a: str, b: str, r: dict, seqnr: int) -> str:
    head = "    ," if seqnr > 1 else "    "
    if r["status"]:
        return '%s{ "a": "%s", "b": "%s", "status": %d }\n' % (head, _esc(a), _esc(b), r["status"])
    tail = ', "weight": %s, "weighted_score": %s' % (rust_f64(r["weight"]), rust_f64(r["weighted_score"])) if "weight" in r else ""
    return '%s{ "a": "%s", "b": "%s", "score": %s, "ld": %d, "lcs": %d, "prefix": %d, "suffix": %d, "samecase": %s%s }\n' % (
        head, _esc(a), _esc(b), rust_f64(r["score"]), r["ld"], r["lcs"], r["prefixlen"], r["suffixlen"], "true" if r["samecase"] else "false", tail)


def run_score(model, a, out) -> None:
    """`score`: every input line is `a<TAB>b` (a line without a tab: b is empty); the pairs of --batch-size lines are one
    score_pairs call.  The model's lexicons play no part in the numbers: only its alphabet and weights do."""
    seqnr = 0
    pa: List[str] = []
    pb: List[str] = []

    def flush():
        nonlocal seqnr
        if not pa:
            return
        for x, y, r in zip(pa, pb, model.score_pairs(pa, pb, weighted=True) if a.weighted else model.score_pairs(pa, pb)):
            seqnr += 1
            out.write(score_json_item(x, y, r, seqnr) if a.json else score_tsv_line(x, y, r) + "\n")
        out.flush()
        pa.clear()
        pb.clear()

    limit = 1 if a.interactive else max(1, a.batch_size)
    for line in _lines(a.files):
        x, _, y = (line[:-1] if line.endswith("\r") else line).partition("\t")
        pa.append(x)
        pb.append(y.split("\t", 1)[0])
        if len(pa) >= limit:
            flush()
    flush()


def run_mine(model, a, out) -> None:
    """`mine`: every input line is `observed<TAB>correct[<TAB>count]`; all pairs are ONE mine_confusables call (the table is over the
    whole input).  Without lexicons the model is not built and the pairs are scripted on the host."""
    import json
    pa: List[str] = []
    pb: List[str] = []
    pc: List[int] = []
    counted = False
    for line in _lines(a.files):
        f = (line[:-1] if line.endswith("\r") else line).split("\t")
        if len(f) < 2:
            continue
        pa.append(f[0])
        pb.append(f[1])
        if len(f) > 2 and f[2].strip():
            counted = True
            pc.append(int(f[2]))
        else:
            pc.append(1)
    conf = None if a.as_confusables is None else (a.as_confusables, a.min_count)
    r = model.mine_confusables_arrays(pa, pb, pc if counted else None, context=a.context, anchors=a.anchors, as_confusables=conf)
    if conf is not None:
        out.write(r["confusables"])
        return
    off, text = r["text_off"].tolist(), r["text"]
    rows = [(text[off[k]:off[k + 1]].decode("utf-8", "surrogateescape"), int(r["count"][k]), int(r["sites"][k]), not (int(r["flags"][k]) & 1))
            for k in range(len(off) - 1)]
    if a.json:
        json.dump([{"pattern": t, "count": c, "sites": s, "representable": ok} for t, c, s, ok in rows], out, ensure_ascii=False, indent=1)
        out.write("\n")
    else:
        for t, c, s, _ok in rows:
            out.write(f"{t}\t{c}\t{s}\n")


def evaluate_tsv_line(inp: str, gold: str, r: dict, top_text: str) -> str:
    """input, gold, 1-based rank of gold in the ranked variants (`-`: not among them), the text of the top variant (empty: none),
    gold_score (the ranked row's dist_score, else the pair's own score), ld (unbounded Damerau-Levenshtein of the pair), reason"""
    return "\t".join([inp, gold, "-" if r["rank"] is None else str(r["rank"] + 1), top_text, rust_f64(r["gold_score"]), str(r["ld"]), r["reason"]])


def evaluate_summary_text(s: dict) -> str:
    lines = ["pairs: %d" % s["n"], "gold known: %d" % s["gold_known"], "accuracy@1: %s" % rust_f64(s["accuracy_at_1"]),
             "ranked: %s" % rust_f64(s["ranked_share"]), "MRR: %s" % rust_f64(s["mrr"])]
    lines += ["%s: %d" % (k, v) for k, v in s["reasons"].items()]
    return "\n".join(lines) + "\n"


def run_evaluate(model, params, a, out) -> None:
    """`evaluate`: every input line is `input<TAB>gold`; the pairs of --batch-size lines are one evaluate call (the ranked variants stay
    on the device).  One TSV line per pair; the summary over all pairs goes to standard error, or as JSON to --summary-json."""
    import json

    import numpy as np
    pa: List[str] = []
    pg: List[str] = []
    recs = []

    def flush():
        if not pa:
            return
        arr = model.evaluate_arrays(pa, pg, params)
        recs.append(arr)
        for i, (x, y) in enumerate(zip(pa, pg)):
            rk, top = int(arr["rank"][i]), int(arr["top_vocab_id"][i])
            r = {"rank": None if rk < 0 else rk, "gold_score": float(arr["gold_score"][i]), "ld": int(arr["ld"][i]),
                 "reason": GOLD_REASONS[int(arr["reason"][i])]}
            out.write(evaluate_tsv_line(x, y, r, "" if top == 0xFFFFFFFF else model.vocab_text(top)) + "\n")
        out.flush()
        pa.clear()
        pg.clear()

    limit = 1 if a.interactive else max(1, a.batch_size)
    for line in _lines(a.files):
        x, _, y = (line[:-1] if line.endswith("\r") else line).partition("\t")
        pa.append(x)
        pg.append(y.split("\t", 1)[0])
        if len(pa) >= limit:
            flush()
    flush()
    allrec = np.concatenate(recs) if recs else np.zeros(0, dtype=np.dtype(VariantModel.GOLD_DTYPE))
    summary = VariantModel.evaluate_summary(allrec)
    if a.summary_json:
        with open(a.summary_json, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")
    else:
        sys.stderr.write(evaluate_summary_text(summary))


GRID_COLUMNS = ("k", "d", "n", "t", "T", "s", "freq-weight")   # the grid's columns, named after query's options (freq-weight: --freq-ranking)
GRID_WEIGHT_COLUMNS = ("w-ld", "w-lcs", "w-prefix", "w-suffix", "w-case")   # a grid that names one of them is a weight grid (evaluate_sweep_weights)


def parse_grid(lines, a) -> List[dict]:
    """The parameter sets of a `sweep --grid` file.  The first line names tab-separated columns among GRID_COLUMNS; every further
    non-empty line is one set, its cells in the syntax of the options (k / d: an integer, a ratio, or `ratio;limit`; s: 0 or 1).  A
    column the grid does not have takes the command line's value (`a`: the parsed arguments).  -> one dict per set, GRID_COLUMNS -> the
    cell as text, in file order; the first set is the baseline.  The header may also name GRID_WEIGHT_COLUMNS (the five score weights):
    a grid that names any of them is a weight grid, and every set's dict then holds all five (absent ones: --weight-* of the command
    line); a grid without them gives the dicts it always gave."""
    rows = [ln.rstrip("\r\n") for ln in lines]
    rows = [ln for ln in rows if ln.strip()]
    if not rows:
        raise ValueError("grid: no header line")
    header = rows[0].split("\t")
    for c in header:
        if c not in GRID_COLUMNS and c not in GRID_WEIGHT_COLUMNS:
            raise ValueError("grid: unknown column %r (known: %s)" % (c, " ".join(GRID_COLUMNS + GRID_WEIGHT_COLUMNS)))
    if len(set(header)) != len(header):
        raise ValueError("grid: a column is named twice")
    base = {"k": str(a.max_anagram_distance), "d": str(a.max_edit_distance), "n": str(a.max_matches), "t": rust_f64(a.score_threshold),
            "T": rust_f64(a.cutoff_threshold), "s": "1" if a.stop_exact else "0",
            "freq-weight": rust_f64(a.freq_ranking if a.freq_ranking is not None else 0.0)}
    if any(c in GRID_WEIGHT_COLUMNS for c in header):
        base.update({"w-ld": rust_f64(a.weight_ld), "w-lcs": rust_f64(a.weight_lcs), "w-prefix": rust_f64(a.weight_prefix),
                     "w-suffix": rust_f64(a.weight_suffix), "w-case": rust_f64(a.weight_case)})
    sets = []
    for ln in rows[1:]:
        cells = ln.split("\t")
        if len(cells) != len(header):
            raise ValueError("grid: %r has %d cells, the header %d" % (ln, len(cells), len(header)))
        d = dict(base)
        d.update(zip(header, (c.strip() for c in cells)))
        if d["s"] not in ("0", "1"):
            raise ValueError("grid: column s is 0 or 1, not %r" % d["s"])
        sets.append(d)
    if not sets:
        raise ValueError("grid: no parameter set")
    return sets


def grid_params(d: dict, a) -> SearchParameters:
    """One set of parse_grid as SearchParameters (everything the grid cannot name: the command line's)."""
    import copy
    b = copy.copy(a)
    b.max_anagram_distance, b.max_edit_distance, b.max_matches = d["k"], d["d"], int(d["n"])
    b.score_threshold, b.cutoff_threshold, b.stop_exact, b.freq_ranking = float(d["t"]), float(d["T"]), d["s"] == "1", float(d["freq-weight"])
    return make_params(b)


def grid_weights(d: dict) -> Weights:
    """The weights of one set of a weight grid (parse_grid)."""
    try:
        return Weights(**{c[2:]: float(d[c]) for c in GRID_WEIGHT_COLUMNS})
    except ValueError:
        raise ValueError("grid: a weight is not a number in %r" % [d[c] for c in GRID_WEIGHT_COLUMNS])


def sweep_tsv_line(d: dict, s: dict) -> str:
    """The set's parameters (GRID_COLUMNS), pairs, accuracy@1, mrr, ranked share, the eight reason counts (GOLD_REASONS order), gained@1,
    lost@1 against the first set, the mean number of variants per input.  s: VariantModel.sweep_summary.  A set of a weight grid
    prints its five weights (GRID_WEIGHT_COLUMNS) behind the seven parameters."""
    n = s["n"]
    return "\t".join([d[c] for c in GRID_COLUMNS] + [d[c] for c in GRID_WEIGHT_COLUMNS if c in d] + [str(n), rust_f64(s["accuracy_at_1"]), rust_f64(s["mrr"]), rust_f64(s["ranked_share"])] +
                     [str(s["reasons"][r]) for r in GOLD_REASONS] +
                     [str(s["gained_at_1"]), str(s["lost_at_1"]), rust_f64(s["n_results"] / n if n else 0.0)])


CANDIDATES_MAX, CANDIDATE_SETS_MAX = 64, 256   # anx_evaluate_sweep_confusables' limits


def parse_candidates(lines) -> List[str]:
    """The patterns of a `sweep --candidates` file: the first column of every non-empty line of a confusable list, in file order."""
    pats = [ln.rstrip("\r\n").split("\t", 1)[0] for ln in lines]
    pats = [p for p in pats if p.strip()]
    if not pats:
        raise ValueError("candidates: no pattern")
    if len(pats) > CANDIDATES_MAX:
        raise ValueError("candidates: %d patterns, the limit is %d" % (len(pats), CANDIDATES_MAX))
    return pats


def parse_candidate_weights(text) -> List[float]:
    """`--candidate-weights 1.1,1.25,0.9` as floats (finite, above 0)."""
    import math
    if not text or not text.strip():
        raise ValueError("candidate weights: none given (--candidate-weights 1.1,0.9)")
    try:
        ws = [float(c) for c in text.split(",")]
    except ValueError:
        raise ValueError("candidate weights: not a number in %r" % text)
    if any(not math.isfinite(w) or not w > 0.0 for w in ws):
        raise ValueError("candidate weights: every weight is finite and above 0, not %r" % text)
    return ws


def candidate_grid(patterns: List[str], weights: List[float]):
    """The one-pattern-on grid: set 0 is the baseline with every candidate at 1.0, then one set per (pattern, weight) in pattern order
    with only that pattern on.  -> (labels, weights_list): labels[s] = (pattern or "-", weight), weights_list[s] = one weight per pattern."""
    n_sets = 1 + len(patterns) * len(weights)
    if len(patterns) > CANDIDATES_MAX:
        raise ValueError("candidates: %d patterns, the limit is %d" % (len(patterns), CANDIDATES_MAX))
    if n_sets > CANDIDATE_SETS_MAX:
        raise ValueError("candidates: %d patterns x %d weights + the baseline = %d sets, the limit is %d" % (len(patterns), len(weights), n_sets, CANDIDATE_SETS_MAX))
    labels, rows = [("-", 1.0)], [[1.0] * len(patterns)]
    for j, p in enumerate(patterns):
        for w in weights:
            labels.append((p, w))
            rows.append([w if x == j else 1.0 for x in range(len(patterns))])
    return labels, rows


def candidate_tsv_line(label, s: dict) -> str:
    """One set of the candidate sweep: pattern (`-`: the baseline), weight, accuracy@1, mrr, gained@1, lost@1 against the baseline, the
    eight reason counts (GOLD_REASONS order).  s: VariantModel.sweep_summary."""
    return "\t".join([label[0], rust_f64(label[1]), rust_f64(s["accuracy_at_1"]), rust_f64(s["mrr"]), str(s["gained_at_1"]), str(s["lost_at_1"])] +
                     [str(s["reasons"][r]) for r in GOLD_REASONS])


def run_sweep_candidates(model, a, out) -> None:
    """`sweep --candidates`: every candidate pattern alone at every weight over the `input<TAB>gold` lines, in one
    evaluate_sweep_confusables call under the command line's parameters: one TSV line per set (candidate_tsv_line), the baseline first."""
    import json
    if a.grid:
        sys.stderr.write("ERROR: sweep takes --grid or --candidates, not both (the candidates run under the command line's parameters)\n")
        sys.exit(2)
    try:
        with open(a.candidates, encoding="utf-8", newline="") as f:
            patterns = parse_candidates(f.read().split("\n"))
        labels, rows = candidate_grid(patterns, parse_candidate_weights(a.candidate_weights))
    except ValueError as e:
        sys.stderr.write("ERROR: %s\n" % e)
        sys.exit(2)
    pa: List[str] = []
    pg: List[str] = []
    for line in _lines(a.files):
        x, _, y = (line[:-1] if line.endswith("\r") else line).partition("\t")
        pa.append(x)
        pg.append(y.split("\t", 1)[0])
    params = make_params(a)
    summaries = model.evaluate_sweep_confusables(pa, pg, patterns, [params] * len(rows), rows, [bool(a.early_confusables)] * len(rows))
    for lab, s in zip(labels, summaries):
        out.write(candidate_tsv_line(lab, s) + "\n")
    out.flush()
    if a.summary_json:
        with open(a.summary_json, "w") as f:
            json.dump([dict(s, pattern=lab[0], weight=lab[1]) for lab, s in zip(labels, summaries)], f, indent=1)
            f.write("\n")


def fit_args_error(a) -> Optional[str]:
    """What is wrong with a `sweep --fit` command line, before any file is read; None: nothing."""
    if not a.fit:
        if a.fit_output:
            return "--fit-output needs --fit"
        return None
    if not a.candidates:
        return "--fit needs --candidates LIST.tsv and --candidate-weights W,W,.."
    if a.early_confusables:
        return "--fit weights the candidates after pruning (late confusables) only: drop --early-confusables"
    if a.grid:
        return "sweep takes --grid or --candidates, not both (the candidates run under the command line's parameters)"
    if not 1 <= a.fit_rounds <= 256:
        return "--fit-rounds must be in 1..256"
    gain = fit_min_gain_of(a)
    if not gain >= 0.0 or gain == float("inf") or (a.fit_objective == "acc1" and gain != int(gain)):
        return "--fit-min-gain is a number >= 0 (acc1: a whole number of pairs)"
    return None


def fit_min_gain_of(a) -> float:
    return float(a.fit_min_gain) if a.fit_min_gain is not None else (1.0 if a.fit_objective == "acc1" else 0.0)


def fit_tsv_line(pattern: str, weight: float, c: dict) -> str:
    """One line of `sweep --fit`: pattern (`-`: the start), weight, accuracy@1, MRR, ranked pairs.  c: VariantModel.fit_counts_summary."""
    return "\t".join([pattern, rust_f64(weight), rust_f64(c["accuracy_at_1"]), rust_f64(c["mrr"]), str(c["ranked"])])


def fit_list_text(weights: dict) -> str:
    """The fitted list as read_confusablelist reads it: `pattern<TAB>weight`, the weight printed so that it reads back bit for bit."""
    return "".join("%s\t%s\n" % (p, repr(float(w))) for p, w in weights.items())


def run_sweep_fit(model, a, out) -> None:
    """`sweep --candidates --fit`: fit_confusables over the `input<TAB>gold` lines under the command line's parameters."""
    import json
    try:
        with open(a.candidates, encoding="utf-8", newline="") as f:
            patterns = parse_candidates(f.read().split("\n"))
        grid = parse_candidate_weights(a.candidate_weights)
        if len(grid) > 16:
            raise ValueError("candidate weights: %d weights, --fit takes 16 at most" % len(grid))
    except ValueError as e:
        sys.stderr.write("ERROR: %s\n" % e)
        sys.exit(2)
    pa: List[str] = []
    pg: List[str] = []
    for line in _lines(a.files):
        x, _, y = (line[:-1] if line.endswith("\r") else line).partition("\t")
        pa.append(x)
        pg.append(y.split("\t", 1)[0])
    gain = fit_min_gain_of(a)
    fit = model.fit_confusables(pa, pg, patterns, make_params(a), grid, None, a.fit_objective, a.fit_rounds, int(gain) if a.fit_objective == "acc1" else gain)
    out.write(fit_tsv_line("-", 1.0, fit["start"]) + "\n")
    for r in fit["rounds"]:
        out.write(fit_tsv_line(r["pattern"], r["weight"], r) + "\n")
    out.write("# stop: %s after %d rounds\n" % ("no trial improves the objective" if fit["stop"] == "converged" else "--fit-rounds reached", len(fit["rounds"])))
    out.flush()
    if a.fit_output:
        with open(a.fit_output, "w", encoding="utf-8", newline="") as f:
            f.write(fit_list_text(fit["weights"]))
    if a.summary_json:
        with open(a.summary_json, "w") as f:
            json.dump(fit, f, indent=1)
            f.write("\n")


def run_sweep(model, a, out) -> None:
    """`sweep`: the `input<TAB>gold` lines of the input under every parameter set of --grid in one evaluate_sweep call: one TSV line per
    set (sweep_tsv_line), in grid order; --summary-json: the same as a JSON list (the set's parameters under "params")."""
    import json
    if a.fit:
        run_sweep_fit(model, a, out)
        return
    if a.candidates:
        run_sweep_candidates(model, a, out)
        return
    if not a.grid:
        sys.stderr.write("ERROR: sweep needs --grid or --candidates\n")
        sys.exit(2)
    with open(a.grid, encoding="utf-8", newline="") as f:
        sets = parse_grid(f.read().split("\n"), a)
    if len(sets) > 256:
        sys.stderr.write("ERROR: --grid holds more than 256 parameter sets\n")
        sys.exit(2)
    pa: List[str] = []
    pg: List[str] = []
    for line in _lines(a.files):
        x, _, y = (line[:-1] if line.endswith("\r") else line).partition("\t")
        pa.append(x)
        pg.append(y.split("\t", 1)[0])
    if "w-ld" in sets[0]:   # a weight grid: one base run per (k, d, s), every set re-scored and re-ranked on the device
        summaries = model.evaluate_sweep_weights(pa, pg, [grid_params(d, a) for d in sets], [grid_weights(d) for d in sets])
    else:
        summaries = model.evaluate_sweep(pa, pg, [grid_params(d, a) for d in sets])
    for d, s in zip(sets, summaries):
        out.write(sweep_tsv_line(d, s) + "\n")
    out.flush()
    if a.summary_json:
        with open(a.summary_json, "w") as f:
            json.dump([dict(s, params=d) for d, s in zip(sets, summaries)], f, indent=1)
            f.write("\n")


def main(argv=None) -> int:
    a = build_parser().parse_intermixed_args(argv)
    if a.mode == "learn" and not 0 <= a.iterations <= 255:
        sys.stderr.write("ERROR: --iterations must be in 0..255\n")
        return 2
    if a.mode == "mine" and not 0 <= a.context <= 8:
        sys.stderr.write("ERROR: --context must be in 0..8\n")
        return 2
    if a.mode == "mine" and not (a.lexicon or a.variants or a.errors or a.index_cache):
        # nothing to build: the pairs are scripted on the host (the switch ANX_MINE=host), which needs only the library
        from ._lib import set_switch
        set_switch("ANX_MINE", "host")
        weights = Weights(ld=a.weight_ld, lcs=a.weight_lcs, prefix=a.weight_prefix, suffix=a.weight_suffix, case=a.weight_case)
        run_mine(VariantModel(a.alphabet, weights, debug=a.debug, device=a.device), a, sys.stdout)
        return 0
    if a.mode == "sweep" and fit_args_error(a):
        sys.stderr.write("ERROR: %s\n" % fit_args_error(a))
        return 2
    model = make_model(a)
    params = make_params(a)
    out = sys.stdout
    if a.mode == "mine":
        run_mine(model, a, out)
        return 0
    if a.mode == "learn":
        run_learn(model, params, a, out)
        return 0
    if a.mode == "evaluate":
        run_evaluate(model, params, a, out)
        return 0
    if a.mode == "sweep":
        run_sweep(model, a, out)
        return 0
    if a.json:
        out.write("[\n")
    if a.mode == "score":
        run_score(model, a, out)
    else:
        (run_query if a.mode == "query" else run_search)(model, params, a, out)
    if a.json:
        out.write("]\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
