"""anx_batch_fetch_measures without a GPU: the record and the entry points exist in the header, the library and the Python layers and
agree on the layout, a model without a device is refused before any work, `query --explain` parses and formats, and the new kernels'
gfx950 ISA metadata holds what DESIGN.md section 5 states (no scratch, no spills; the pair kernels they restate are unchanged)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import analiticcl_amd as A
from analiticcl_amd import _lib as L
from analiticcl_amd import cli
from analiticcl_amd.model import Batch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "analiticcl_amd", "csrc")
NAMES = ("anx_batch_fetch_measures", "anx_measures_free")
OFFSETS = {"score": 0, "ld": 8, "lcs": 9, "prefixlen": 10, "suffixlen": 11, "len_input": 12, "len_entry": 13, "anagram_distance": 14, "flags": 15}


def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(REPO, "include", "anx.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
        assert hasattr(lib, n), n
    assert L.lib().anx_abi_version() == L.ABI_VERSION == 3


def test_record_layout():
    hdr = open(os.path.join(REPO, "include", "anx.h")).read()
    assert "static_assert(sizeof(anx_row_measures) == 16" in hdr
    dt = np.dtype(Batch.MEASURES_DTYPE)
    assert C.sizeof(L.RowMeasures) == 16 == dt.itemsize
    assert [n for n, _t in L.RowMeasures._fields_] == list(OFFSETS) == list(dt.names)
    for name, off in OFFSETS.items():
        assert getattr(L.RowMeasures, name).offset == off == dt.fields[name][1], name
    # the record as a C compiler lays it out, and the header as plain C
    src = '#include "anx.h"\n#include <stddef.h>\nint a[sizeof(anx_row_measures) == 16 ? 1 : -1];\n' + "".join(
        "int f%d[offsetof(anx_row_measures, %s) == %d ? 1 : -1];\n" % (i, n, o) for i, (n, o) in enumerate(OFFSETS.items()))
    subprocess.run(["cc", "-std=c11", "-fsyntax-only", "-I", os.path.join(REPO, "include"), "-x", "c", "-"], input=src.encode(), check=True)


def test_no_device_is_an_error(tmp_path):
    alphabet = os.path.join(REPO, "tests", "golden", "data", "simple_alphabet.tsv")
    lex = tmp_path / "hand.lexicon"
    lex.write_text("separate\nreceive\n")
    m = A.VariantModel(alphabet, A.Weights(), device=-1)   # host only: never resident on a device
    m.read_lexicon(str(lex))
    m.build()
    p = A.SearchParameters(max_anagram_distance=2, max_edit_distance=1, max_matches=3)
    with pytest.raises(A.AnxError) as e:
        m.explain_variants(["seperate"], p)
    assert e.value.code == L.ANX_ENODEVICE
    rows, offs = C.c_void_p(), C.POINTER(C.c_uint32)()
    assert L.lib().anx_batch_fetch_measures(None, C.byref(rows), C.byref(offs)) == L.ANX_EINVAL
    L.lib().anx_measures_free(None, None)   # like free(NULL)


VARIANTS = [{"text": "separate", "score": 0.75, "dist_score": 0.75, "freq_score": 1.0, "lexicons": ["eng"], "ld": 1, "lcs": 3, "prefixlen": 3,
             "suffixlen": 4, "samecase": True, "anagram_distance": 2, "len_input": 8, "len_entry": 8, "unweighted_score": 0.75},
            {"text": 'quo"te', "score": 0.5, "dist_score": 0.5, "freq_score": 0.25, "via": "qoute", "scored": "qoute", "lexicons": ["eng"], "ld": 2,
             "lcs": 2, "prefixlen": 1, "suffixlen": 2, "samecase": False, "anagram_distance": 0, "len_input": 8, "len_entry": 5, "unweighted_score": 0.625}]


def test_cli_parses_and_formats_explain():
    p = cli.build_parser()
    common = ["-a", "a.tsv", "-l", "l.tsv", "-k", "2", "-d", "1"]
    a = p.parse_intermixed_args(["query"] + common)
    e = p.parse_intermixed_args(["query", "--explain"] + common)
    assert a.explain is False and e.explain is True
    assert {k: v for k, v in vars(a).items() if k != "explain"} == {k: v for k, v in vars(e).items() if k != "explain"}
    assert tuple(cli.EXPLAIN_KEYS) == tuple(A.VariantModel.EXPLAIN_KEYS)
    # without the flag the formatters write what they always wrote
    plain = [{k: v for k, v in x.items() if k not in cli.EXPLAIN_KEYS and k != "scored"} for x in VARIANTS]
    assert cli.tsv_line("seperate", VARIANTS) == cli.tsv_line("seperate", plain) == 'seperate\tseparate\t0.75\t\tquo"te\t0.5\t'
    assert cli.json_item("seperate", VARIANTS, 1) == cli.json_item("seperate", plain, 1)
    line = cli.tsv_line("seperate", VARIANTS, explain=True)
    assert line == ('seperate\tseparate\t0.75\t1\t3\t3\t4\ttrue\t2\t8\t8\t0.75\t\t'
                    '\tquo"te\t0.5\t2\t2\t1\t2\tfalse\t0\t8\t5\t0.625\tqoute\t')
    assert cli.tsv_line("nothing", [], explain=True) == "nothing"
    items = json.loads("[\n" + cli.json_item("seperate", VARIANTS, 1, explain=True) + cli.json_item("x", [], 2, explain=True) + "]\n")
    assert items[1] == {"input": "x", "variants": []}
    v0, v1 = items[0]["variants"]
    for src, got in zip(VARIANTS, (v0, v1)):
        for k in cli.EXPLAIN_KEYS:
            assert got[k] == src[k], k
    assert "scored" not in v0 and v1["scored"] == "qoute" and v1["via"] == "qoute" and v1["text"] == 'quo"te'


KEYS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


def kernels_of(source, tmp_path):
    out = str(tmp_path / (source + ".s"))
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                           "--cuda-device-only", "-o", out, os.path.join(CSRC, source)], stderr=subprocess.DEVNULL)
    text = open(out).read()
    ks = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        ks[m.group(2)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(3)).group(1)) for k in KEYS}
        ks[m.group(2)]["group_segment_fixed_size"] = int(m.group(1))
    return ks, text


def test_explain_kernels_isa_metadata(tmp_path):
    """DESIGN.md section 5 "Measures of the ranked rows": no scratch, no VGPR or SGPR spills; k_row_measures keeps a 16 x 16 byte matrix
    and both strings per lane in LDS (128 lanes x 73 dwords) within 64 VGPRs, computes L1 with v_sad_u8 and writes a record as one
    16-byte store; k_row_measures_long keeps the 255-row matrix in LDS."""
    ks, text = kernels_of("results.hip", tmp_path)
    one = {}
    for kernel in ("k_vocab_entry_scatter", "k_row_measuresENS", "k_row_measures_long"):
        r = [v for n, v in ks.items() if kernel in n]
        assert len(r) == 1, (kernel, sorted(ks))
        assert r[0]["vgpr_spill_count"] == 0 and r[0]["sgpr_spill_count"] == 0 and r[0]["private_segment_fixed_size"] == 0, (kernel, r[0])
        assert r[0]["vgpr_count"] <= 64, (kernel, r[0])
        one[kernel] = r[0]
    assert one["k_vocab_entry_scatter"]["group_segment_fixed_size"] == 0
    assert one["k_row_measuresENS"]["group_segment_fixed_size"] == 128 * 73 * 4
    assert 255 * 261 <= one["k_row_measures_long"]["group_segment_fixed_size"] <= 72 * 1024
    name = [n for n in ks if "k_row_measuresENS" in n][0]
    body = text[text.index(name + ":"):]
    body = body[:body.index("s_endpgm")]
    assert "v_sad_u8" in body and "scratch_" not in body


# k_pairs_short, k_pairs_long<64>, k_pairs_long<255> as the commit before this feature compiled them
PAIRS_BEFORE = ({"vgpr_count": 36, "sgpr_count": 58, "group_segment_fixed_size": 37376, "private_segment_fixed_size": 0},
                {"vgpr_count": 27, "sgpr_count": 63, "group_segment_fixed_size": 5328, "private_segment_fixed_size": 0},
                {"vgpr_count": 29, "sgpr_count": 64, "group_segment_fixed_size": 69376, "private_segment_fixed_size": 0})


def test_pair_kernels_are_unchanged(tmp_path):
    """The explain kernels restate pairs.hip's recurrence instead of sharing it: the pair kernels' metadata is what the commit before
    this feature had (read from its build)."""
    ks, _ = kernels_of("pairs.hip", tmp_path)
    want = {"k_pairs_short": PAIRS_BEFORE[0], "k_pairs_longILi64": PAIRS_BEFORE[1], "k_pairs_longILi255": PAIRS_BEFORE[2]}
    for frag, exp in want.items():
        r = [v for n, v in ks.items() if frag in n]
        assert len(r) == 1, frag
        assert {k: r[0][k] for k in exp} == exp, (frag, r[0])


