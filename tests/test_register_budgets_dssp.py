"""CPU tier: register budgets of the secondary-structure kernels.  No kernel may use scratch.

Every kernel of the family keeps its tables in the frame-minor workspace and only scalars in registers -- the one donor's N, H and
CA (9), one acceptor's CA, O and C (9), the four distances and the two slots in the energy kernels; eight bridge candidates in
k_dssp_local, picked in ascending order by fully unrolled compares so that the array never needs an address.  The build takes 14 to
56 registers (k_dssp_local the most); the budget is 64 for all = eight waves per SIMD (512 / 64): the energy kernels' loads per
acceptor are hidden behind other waves, not behind unrolling.

In the two energy kernels the only fused multiply-adds allowed are those of the correctly rounded roots and quotients of rule 2
(mk_fsqrt_rn: four per root in its two forms; mk_fdiv_rn: five per quotient): 4 roots and 4 quotients = 36.  One more would be a
contraction inside the energy and could move a decision at -0.5 kcal/mol.  So: exactly 36 v_fma_f32 / v_fmac_f32, no v_mad / v_mac /
v_pk_fma, exactly 4 v_sqrt_f32 and 4 v_rsq_f32, no double precision, no atomics anywhere in the family, and at least the 16 separate
multiplies of the 9 A test, the four squared lengths and the scale (a packed v_pk_mul_f32 counts as two: its products are rounded
separately)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

KERNELS = ("15k_dssp_segments", "15k_dssp_backbone", "20k_dssp_energy_frames", "19k_dssp_energy_atoms", "12k_dssp_local", "13k_dssp_sheets",
           "13k_dssp_helix3", "13k_dssp_finish")
MAX_VGPR = 64


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_dssp_kernels_stay_inside_their_register_budgets(tmp_path):
    asm = tmp_path / "capi.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "moleculekit_amd", "csrc", "capi.hip"), "-o", str(asm)],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    for kern in KERNELS:
        m = re.search(r"\.set (_ZN5mkamd" + re.escape(kern) + r"E\S*)\.num_vgpr, (\d+)", text)
        assert m, f"{kern}: kernel not found in the assembly"
        vgpr = int(m.group(2))
        s = re.search(r"\.set " + re.escape(m.group(1)) + r"\.private_seg_size, (\d+)", text)
        scratch = int(s.group(1)) if s else 0
        assert vgpr <= MAX_VGPR, f"{kern}: {vgpr} VGPRs, budget {MAX_VGPR}"
        assert scratch == 0, f"{kern}: {scratch} B of scratch"
        b = re.search(r"^" + re.escape(m.group(1)) + r":", text, re.M)
        body = text[b.end():text.index(".amdhsa_kernel " + m.group(1), b.end())]
        count = lambda pat: len(re.findall(pat, body))  # noqa: E731
        assert count(r"v_(mad|mac|pk_fma)_\w*f32") == 0, f"{kern}: a multiply-add outside the roots and quotients"
        assert count(r"_f64") == 0, f"{kern}: double-precision arithmetic"
        assert count(r"(global|flat)_atomic") == 0, f"{kern}: an atomic"
        if "energy" in kern:
            fused = count(r"v_(fma|fmac)_f32")
            assert fused == 36, f"{kern}: {fused} fused multiply-adds, four roots and four quotients have 36"
            assert count(r"v_sqrt_f32") == 4 and count(r"v_rsq_f32") == 4, f"{kern}: a root besides the four distances'"
            muls = count(r"v_mul_f32") + 2 * count(r"v_pk_mul_f32")
            assert muls >= 16, f"{kern}: {muls} multiplies, the energy has 16"
