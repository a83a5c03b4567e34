"""CPU tier: register budgets of the group-moment kernels.  No kernel may spill.

k_mom_sums holds, per lane, the frame's affine in double (12 values = 24 registers), the sums in double (center 4, gyration 7,
spherical 6, fluct 1: up to 14 registers), the shift (3 doubles), one atom (3 floats and their 3 doubles), the weight and the
addressing of four arrays -- about 60 values for the centre, 72 for the gyration; the finishing arithmetic of the form in which a
lane group owns its (frame, group) (three double divisions and roots, acos and atan2 for the spherical mode) runs in lane 0 after the
loop and reuses the loop's registers.  The budget is 84 = six waves per SIMD (512 / 84) for every instantiation: the loop is a chain
of dependent gathers (index, then three coordinates) that only other waves hide, and six waves of 64-lane gathers per SIMD already
saturate the address path; the kernel keeps nothing in LDS.  k_mom_fold reads records and finishes: budget 64.  k_mom_mean carries
the affine and three sums (budget 64), k_mom_fluct_atoms the affine and one atom (budget 64)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# mangled name -> max VGPRs; scratch is 0 for all
BUDGETS = {"10k_mom_meanE": 64, "17k_mom_fluct_atomsE": 64}
for mode in (0, 1, 2, 3):
    BUDGETS[f"10k_mom_foldILi{mode}EE"] = 64
    for seg in (0, 1):
        BUDGETS[f"10k_mom_sumsILi{mode}ELb{seg}EE"] = 84


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_moment_kernels_stay_inside_their_register_budgets(tmp_path):
    asm = tmp_path / "capi.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "moleculekit_amd", "csrc", "capi.hip"), "-o", str(asm)],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    for kern, max_vgpr in BUDGETS.items():
        m = re.search(r"\.set (_ZN5mkamd" + re.escape(kern) + r"\S*)\.num_vgpr, (\d+)", text)
        assert m, f"{kern}: kernel not found in the assembly"
        vgpr = int(m.group(2))
        s = re.search(r"\.set " + re.escape(m.group(1)) + r"\.private_seg_size, (\d+)", text)
        scratch = int(s.group(1)) if s else 0
        assert vgpr <= max_vgpr, f"{kern}: {vgpr} VGPRs, budget {max_vgpr}"
        assert scratch == 0, f"{kern}: {scratch} B of scratch"
