"""CPU tier: register budgets of the ring-interaction kernels.  No kernel may spill.

Every kernel of the family is a chain of dependent loads and float32 operations with little to keep: the pre-pass holds three running
sums, the first three atoms (9 floats) and the float64 temporaries of its divisions and root; the count and fill kernels hold the first
ring's record (9 floats), the box (3), what they have read of the partner's record, a 64-bit mask and -- past the distance tests -- the
temporaries of the float32 acos and its float64 division.  What hides such chains is other waves, so the budget of EVERY instantiation
is 64 registers: eight waves per SIMD, the most the hardware schedules.  (The build takes 13 .. 60.)

The float32 arithmetic of the reference must stay separate multiplies, adds and subtractions: a fused multiply-add anywhere in these
kernels would change a centroid, a normal, a squared distance, a dot product or the restated acosf, and with them pairs and angles.
Divisions and roots go through float64 (ring_div, ring_sqrt), whose expansions use float64 multiply-adds only -- so NO float32
multiply-add of any kind may appear, and no float32 root or division estimate either.
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
KERNELS = [("14k_ring_prepass", f"ILb{b}EE") for b in (0, 1)]
KERNELS += [("15k_ring_partners", f"ILi{k}ELb{b}EE") for k in (1, 2) for b in (0, 1)]
KERNELS += [(name, f"ILi{k}EE") for name in ("18k_ring_count_pairs", "19k_ring_count_frames") for k in (0, 1, 2)]
KERNELS += [("11k_ring_fill", f"ILi{k}ELb{b}EE") for k in (0, 1, 2) for b in (0, 1)]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_ring_kernels_stay_inside_their_register_budgets(tmp_path):
    asm = tmp_path / "capi.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "moleculekit_amd", "csrc", "capi.hip"), "-o", str(asm)],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    assert len(re.findall(r"^\s*\.set (_ZN5mkamd\d+k_ring_\S*)\.num_vgpr, ", text, re.M)) == len(KERNELS), "an instantiation this test does not know"
    for kern, targs in KERNELS:
        m = re.search(r"\.set (_ZN5mkamd" + re.escape(kern + targs) + r"\S*)\.num_vgpr, (\d+)", text)
        assert m, f"{kern}{targs}: kernel not found in the assembly"
        vgpr = int(m.group(2))
        s = re.search(r"\.set " + re.escape(m.group(1)) + r"\.private_seg_size, (\d+)", text)
        scratch = int(s.group(1)) if s else 0
        assert vgpr <= BUDGET, f"{kern}{targs}: {vgpr} VGPRs, budget {BUDGET}"
        assert scratch == 0, f"{kern}{targs}: {scratch} B of scratch"
        b = re.search(r"^" + re.escape(m.group(1)) + r":", text, re.M)
        body = text[b.end():text.index(".amdhsa_kernel " + m.group(1), b.end())]
        assert not re.search(r"v_(fma|fmac|fmamk|fmaak|mad|mac|madmk|madak|pk_fma)_(legacy_)?f32", body), f"{kern}{targs}: a float32 multiply-add in the kernel"
        assert not re.search(r"v_(sqrt|rsq|div_scale|div_fmas|div_fixup)_f32", body), f"{kern}{targs}: a float32 root or division in the kernel"
        if "partners" not in kern or "ILi2E" in targs:                 # (the cation pre-pass only copies positions)
            assert re.search(r"v_(mul|add|sub)_f32", body), f"{kern}{targs}: no separate float32 arithmetic found"
