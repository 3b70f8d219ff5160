"""Resources of the kernels the small call's confusable chain adds or changes, read from the gfx950 ISA metadata hipcc emits (no GPU
needed): k_small_conf_order (conf.hip: the single-block LDS counting sort that orders the list of rows to weight) and k_small_fetch
(engine.hip: now also reports the chain's counters).  Neither may spill vector registers or use scratch, and the order kernel's
static LDS -- a histogram of the 8192 shape keys -- stays within the 64 KB a block may declare."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "analiticcl_amd", "csrc")
KEYS = ("vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels_of(source, tmp_path):
    out = str(tmp_path / (source + ".s"))
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                           "--cuda-device-only", "-o", out, os.path.join(CSRC, source)], stderr=subprocess.DEVNULL)
    text = open(out).read()
    res = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
        body = m.group(0)
        res[re.search(r"\.name:\s+(\S+)", body).group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", body).group(1)) for k in KEYS}
    return res


def test_new_kernels_neither_spill_nor_use_scratch(tmp_path):
    for source, frag in (("conf.hip", "k_small_conf_order"), ("engine.hip", "k_small_fetch")):
        hit = {n: r for n, r in kernels_of(source, tmp_path).items() if frag in n}
        assert len(hit) == 1, (frag, list(hit))
        for n, r in hit.items():
            assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (n, r)
            if frag == "k_small_conf_order":
                assert 32 * 1024 <= r["group_segment_fixed_size"] <= 64 * 1024, (n, r)
