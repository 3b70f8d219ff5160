"""Register / scratch budget of the HIP kernels, read from the gfx950 ISA metadata hipcc emits (no GPU needed).

Round 1 left an unexplained non-termination: with amdgpu_waves_per_eu(8, 8) forced on k_filter_score the GPU suite "did not
finish".  Root cause (tools/build_occ8_probe.sh, tools/occ8_bisect.sh on MI355X, round 2): under the forced 64-VGPR budget the
compiler spills 66-90 SGPRs and up to 28 VGPRs of the instances to scratch, and the D = 0 instance (d > 3, the run of
test_parameter_sets_vs_oracle) dies with a GPU memory access fault; the d = 1..3 instances pass and are no faster (0.445 vs
0.436 ms).  The 72-VGPR footprint came from the 8-word prefilter state, which now lives in k_filter_wide; nothing forces an
occupancy any more.  This test keeps that class of problem from coming back: no kernel of the engine may spill vector
registers or use scratch memory, and the two dominant kernels must keep the occupancy DESIGN.md states."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "analiticcl_amd", "csrc")


def _kernels_of(source, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / (source + ".s"))
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                           "--cuda-device-only", "-o", out, os.path.join(CSRC, source)], stderr=subprocess.DEVNULL)
    text = open(out).read()
    res = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        body = m.group(2)
        res[m.group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", body).group(1))
                           for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    return res


def test_row_kernels_do_not_spill(tmp_path_factory):
    """The one-lane-per-row / one-wave-per-stretch kernels of round 3 (confusable weighting, lattice decoding): their working sets
    live in explicit HBM / LDS buffers, not in compiler-generated scratch."""
    for source, names in (("conf.hip", ("k_conf_script", "k_conf_screen", "k_conf_apply_late")), ("lattice.hip", ("k_lattice",))):
        ks = _kernels_of(source, tmp_path_factory)
        for frag in names:
            hit = [r for n, r in ks.items() if frag in n]
            assert hit, frag
            for r in hit:
                assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (frag, r)
            if frag == "k_lattice":
                # k_lattice (merges: ~10 KB of LDS per wave bound its waves) and k_lattice_lm (no LDS: 8 waves per SIMD as long as it stays
                # within 64 registers); the pop loop keeps its scalar state (winner masks, pop counter) in SGPRs
                assert len(hit) == 4 and all(r["vgpr_count"] <= 64 and r["sgpr_spill_count"] == 0 for r in hit), hit


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    # the kernels of a run and of the small call (engine.hip) and those that take the ranked rows off the device (results.hip)
    res = {}
    for source in ("engine.hip", "results.hip"):
        ks = _kernels_of(source, tmp_path_factory)
        assert ks and not set(ks) & set(res), source
        res.update(ks)
    assert len(res) > 20
    return res


def test_no_kernel_spills_vgprs_or_uses_scratch(kernels):
    for name, r in kernels.items():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)


def test_occupancy_of_the_dominant_kernels(kernels):
    def vgprs(fragment):
        hit = [r["vgpr_count"] for n, r in kernels.items() if fragment in n]
        assert hit, fragment
        return max(hit)
    # round 3: the fused band-match filter in the scan's expansion needs 90 VGPRs -> 5 waves per SIMD (512 / 96), which the
    # kernel's LDS footprint (27.6 KB per 4-wave block) allows as well; without the filter state it was 76 (6 waves)
    assert vgprs("k_scan_bits") <= 96
    # round 4: the production instance of the scan (no StopAtExactMatch / pair-count / keep-all branches) keeps its scalar state in
    # registers: 28 SGPRs spilled into VGPR lanes cost the hot loops 0.05 ms of the kernel's 1.60 (v_readlane / v_writelane + hazards)
    prod = [r for n, r in kernels.items() if "k_scan_bitsILb0" in n]
    assert prod and all(r["sgpr_spill_count"] <= 8 for r in prod), prod
    # round 5: k_scan_adj (the tiles that stream an adjacency list: 99 % of them) runs at 6 waves per SIMD -- <= 80 VGPRs (and 26.6 KB
    # of LDS per block) -- and keeps its scalar state in registers in BOTH instances (the StopAtExactMatch / pair-count one too)
    adj = [r for n, r in kernels.items() if "k_scan_adj" in n]
    assert len(adj) == 2 and all(r["vgpr_count"] <= 80 and r["sgpr_spill_count"] == 0 for r in adj), adj
    # round 4: the instance of k_rank for models without variant lists at freq_weight 0 (what every BASELINE configuration runs)
    simple = [r for n, r in kernels.items() if "k_rankILb1" in n]
    assert simple and all(r["sgpr_spill_count"] == 0 and r["vgpr_count"] <= 72 for r in simple), simple
    # round 6: one pass (DL by diagonals on the slots as they lie, a survivor queue per wave, the tail from the same masks): 6 waves per
    # SIMD on symbol planes (twelve plane registers), 7 on byte rows -- measured: no difference between 6, 7 and 8 (HISTORY.md section 15);
    # the instances with the inline 8-word prefilter only run under ANX_FS_SPLIT=0 (A/B)
    assert vgprs("k_filter_scoreILi2ELb0") <= 80
    assert vgprs("k_filter_scoreILi1ELb0") <= 80
    assert vgprs("k_filter_scoreILi3ELb0") <= 80
    assert vgprs("k_filter_score") <= 112
