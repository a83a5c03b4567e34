"""CPU tier: register budgets of the dihedral kernels.  No kernel may spill.

Both kernels hold one dihedral per lane at a time: 12 coordinates, 9 bond components, 6 cross components, the box (3) and the
addressing -- about 40 values; the terms and sin / cos instantiations take 26-40 registers.  Their budget is 64 = eight waves per SIMD
(512 / 64): the loop over a wave's 16 dihedrals is not unrolled, the 12 coalesced loads of a dihedral are hidden behind OTHER waves,
and the frame kernel's LDS tile (33 KB a block of four waves at two floats per dihedral) allows four blocks a CU = four waves a
SIMD anyway, so 64 registers never bind.  The radians / degrees instantiations carry the float64 atan2 (72-73 registers): budget 84 =
six waves per SIMD, above the four the tile allows.

In the TERMS instantiations the only fused multiply-adds allowed are the four of the correctly rounded root (mk_fsqrt_rn: two in its
short form, two in the form for tiny / special operands, which repair the bare v_rsq_f32 / v_sqrt_f32 estimates): one more would be
a contraction inside the reference's arithmetic and change the bits of (p1, p2).  So: exactly 4 v_fma_f32 / v_fmac_f32, no v_mad /
v_mac / v_pk_fma, exactly one v_sqrt_f32 and one v_rsq_f32 (each followed by its repair), and at least the 22 separate multiplies
of the terms (12 in the two cross products, 9 in the three dot products, 1 by the root; a packed v_pk_mul_f32 counts as two:
its products are rounded separately)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (kernel, template arguments as mangled: wrap, mode) -> max VGPRs; scratch is 0 for all
BUDGETS = {}
for wrap in (0, 1):
    for mode in (0, 1, 2, 3):
        for kern in ("17k_dihedral_frames", "16k_dihedral_atoms"):
            BUDGETS[(kern, f"ILb{wrap}ELi{mode}EE")] = 84 if mode in (1, 2) else 64


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_dihedral_kernels_stay_inside_their_register_budgets(tmp_path):
    asm = tmp_path / "capi.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "moleculekit_amd", "csrc", "capi.hip"), "-o", str(asm)],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    for (kern, targs), max_vgpr in BUDGETS.items():
        m = re.search(r"\.set (_ZN5mkamd" + re.escape(kern + targs) + r"\S*)\.num_vgpr, (\d+)", text)
        assert m, f"{kern}{targs}: kernel not found in the assembly"
        vgpr = int(m.group(2))
        s = re.search(r"\.set " + re.escape(m.group(1)) + r"\.private_seg_size, (\d+)", text)
        scratch = int(s.group(1)) if s else 0
        assert vgpr <= max_vgpr, f"{kern}{targs}: {vgpr} VGPRs, budget {max_vgpr}"
        assert scratch == 0, f"{kern}{targs}: {scratch} B of scratch"
        if "ELi0EE" in targs:                                       # the terms instantiations
            b = re.search(r"^" + re.escape(m.group(1)) + r":", text, re.M)
            body = text[b.end():text.index(".amdhsa_kernel " + m.group(1), b.end())]
            count = lambda pat: len(re.findall(pat, body))  # noqa: E731
            assert count(r"v_(mad|mac|pk_fma)_\w*f32") == 0, f"{kern}{targs}: a multiply-add outside the root"
            assert count(r"v_(fma|fmac)_f32") == 4, f"{kern}{targs}: {count(r'v_(fma|fmac)_f32')} fused multiply-adds, the root has 4"
            assert count(r"v_sqrt_f32") == 1 and count(r"v_rsq_f32") == 1, f"{kern}{targs}: a root besides mk_fsqrt_rn's"
            assert count(r"_f64") == 0, f"{kern}{targs}: double-precision arithmetic in the terms"
            muls = count(r"v_mul_f32") + 2 * count(r"v_pk_mul_f32")      # (a packed multiply rounds its two products separately)
            assert muls >= 22, f"{kern}{targs}: {muls} multiplies, the terms have 22"
