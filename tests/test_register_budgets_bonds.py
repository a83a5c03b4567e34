"""CPU tier: register budgets of the bond-guesser kernels.  No kernel may spill.

The pair kernels are chains of dependent loads -- the owner's five words, per candidate an index and five more -- in front of a dozen
float32 operations; the cell-list kernels compute a box index or move one word.  What hides such chains is other waves, so the budget
of EVERY instantiation is 64 registers: eight waves per SIMD, the most the hardware schedules.  The 14 neighbour relations are
unpacked from three constants with shifts, so no table is indexed at run time and nothing goes to scratch.

The float32 arithmetic of the reference must stay separate multiplies, adds and subtractions: a fused multiply-add would change a
squared distance, and with it the list.  The one float64 operation of the pair test (0.6 times the widened sum of the radii) is a
float64 multiply; the box index divides in float32 with the correctly rounded division, whose expansion does use float32
multiply-adds -- so the ban on them covers the pair kernels, where there is no division.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
BUDGET = 64

# (kernel, template arguments as mangled): every instantiation the launch plan can take
KERNELS = [("13k_bond_bounds", ""), ("12k_bond_cells", ""), ("12k_bond_flags", ""), ("12k_bond_ranks", ""), ("14k_bond_scatter", ""),
           ("11k_bond_sort", "")]
KERNELS += [("19k_bond_pairs_thread", f"ILb{b}EE") for b in (0, 1)]
KERNELS += [("17k_bond_pairs_wave", f"ILb{b}EE") for b in (0, 1)]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_bond_kernels_stay_inside_their_register_budgets(tmp_path):
    asm = tmp_path / "capi.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "moleculekit_amd", "csrc", "capi.hip"), "-o", str(asm)],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    assert len(re.findall(r"^\s*\.set (_ZN5mkamd\d+k_bond_\S*)\.num_vgpr, ", text, re.M)) == len(KERNELS), "an instantiation this test does not know"
    for kern, targs in KERNELS:
        m = re.search(r"\.set (_ZN5mkamd" + re.escape(kern + targs) + r"\S*)\.num_vgpr, (\d+)", text)
        assert m, f"{kern}{targs}: kernel not found in the assembly"
        vgpr = int(m.group(2))
        s = re.search(r"\.set " + re.escape(m.group(1)) + r"\.private_seg_size, (\d+)", text)
        scratch = int(s.group(1)) if s else 0
        print(f"{kern}{targs}: {vgpr} VGPRs, {scratch} B of scratch")
        assert vgpr <= BUDGET, f"{kern}{targs}: {vgpr} VGPRs, budget {BUDGET}"
        assert scratch == 0, f"{kern}{targs}: {scratch} B of scratch"
        if "pairs" in kern:
            b = re.search(r"^" + re.escape(m.group(1)) + r":", text, re.M)
            body = text[b.end():text.index(".amdhsa_kernel " + m.group(1), b.end())]
            assert not re.search(r"v_(fma|fmac|fmamk|fmaak|mad|mac|madmk|madak|pk_fma)_(legacy_)?f32", body), f"{kern}{targs}: a float32 multiply-add in the kernel"
            assert not re.search(r"v_(sqrt|rsq|div_scale|div_fmas|div_fixup)_f32", body), f"{kern}{targs}: a float32 root or division in the kernel"
            assert re.search(r"v_(mul|add|sub)_f32", body) and re.search(r"v_mul_f64", body), f"{kern}{targs}: the pair test's arithmetic not found"
