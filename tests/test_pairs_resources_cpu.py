"""LDS, register and scratch budget of the pair-scoring kernels (analiticcl_amd/csrc/pairs.hip), read from the gfx950 ISA metadata
hipcc emits (no GPU needed).  Both tiers are bound by LDS, so the occupancy DESIGN.md section 5 states follows from the bytes a block
declares: a CU has 160 KiB."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "analiticcl_amd", "csrc")
LDS_PER_CU = 160 * 1024
KEYS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def test_pair_kernels_lds_and_registers(tmp_path):
    out = str(tmp_path / "pairs.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                           "--cuda-device-only", "-o", out, os.path.join(CSRC, "pairs.hip")], stderr=subprocess.DEVNULL)
    text = open(out).read()
    ks = {}
    # (the metadata lists a kernel's fields in alphabetical order: the LDS size stands before the name, the rest behind it)
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        ks[m.group(2)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(3)).group(1)) for k in KEYS[:-1]}
        ks[m.group(2)]["group_segment_fixed_size"] = int(m.group(1))
    short = [r for n, r in ks.items() if "k_pairs_short" in n]
    long64 = [r for n, r in ks.items() if "k_pairs_longILi64E" in n]
    long255 = [r for n, r in ks.items() if "k_pairs_longILi255E" in n]
    assert len(short) == 1 and len(long64) == 1 and len(long255) == 1, sorted(ks)
    for r in short + long64 + long255:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
        assert r["vgpr_count"] <= 64, r  # registers never bind before LDS does
    # a pair per lane: 73 dwords per lane (16 x 16 byte cells, both strings, an odd stride), 128 lanes per block -> 4 blocks = 8 waves per CU
    assert short[0]["group_segment_fixed_size"] == 128 * 73 * 4 and LDS_PER_CU // short[0]["group_segment_fixed_size"] == 4
    # a pair per wave: the byte matrix of 255 x 255 cells fits twice into a CU (a 16-bit cell would fit once)
    assert 255 * 255 <= long255[0]["group_segment_fixed_size"] and LDS_PER_CU // long255[0]["group_segment_fixed_size"] == 2
    # pairs of at most 64 symbols a side: LDS allows more one-wave blocks than the 32 waves a CU holds
    assert LDS_PER_CU // long64[0]["group_segment_fixed_size"] >= 30
