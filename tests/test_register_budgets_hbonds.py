"""CPU tier: register budgets of the hydrogen-bond kernels.  No kernel may spill.

The count kernels are chains of dependent loads and float32 operations: the box (3), the acceptor (3), per donor row the position it is
measured from (3) and -- with hydrogens -- the wrapped vector heavy - hydrogen and the root of its length (4), a 64-bit mask per row,
and past the distance test the temporaries of the ratio's float64 division and of the restated acosf.  What hides such chains is other
waves, so the budget of EVERY instantiation is 64 registers: eight waves per SIMD, the most the hardware schedules.  That budget is what
sets the rows a frame-lane wave keeps (hbond_kernels.h: hbond_group -- two with hydrogens, four without; three with hydrogens took 68
registers, four 80).  The fill kernels compute nothing.

The float32 arithmetic of the reference must stay separate multiplies, adds and subtractions: a fused multiply-add would change a
squared distance, a dot product or the restated acosf, and with them the list.  Divisions and roots go through float64 (ring_div,
ring_sqrt), whose expansions use float64 multiply-adds only -- so NO float32 multiply-add of any kind may appear in a count kernel, and
no float32 root or division estimate either.
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
KERNELS = [("20k_hbond_count_frames", "ILb0ELi4EE"), ("20k_hbond_count_frames", "ILb1ELi2EE")]
KERNELS += [("19k_hbond_count_pairs", f"ILb{b}EE") for b in (0, 1)]
KERNELS += [("12k_hbond_fill", f"ILb{b}EE") for b in (0, 1)]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_hbond_kernels_stay_inside_their_register_budgets(tmp_path):
    asm = tmp_path / "capi.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "moleculekit_amd", "csrc", "capi.hip"), "-o", str(asm)],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    assert len(re.findall(r"^\s*\.set (_ZN5mkamd\d+k_hbond_\S*)\.num_vgpr, ", text, re.M)) == len(KERNELS), "an instantiation this test does not know"
    for kern, targs in KERNELS:
        m = re.search(r"\.set (_ZN5mkamd" + re.escape(kern + targs) + r"\S*)\.num_vgpr, (\d+)", text)
        assert m, f"{kern}{targs}: kernel not found in the assembly"
        vgpr = int(m.group(2))
        s = re.search(r"\.set " + re.escape(m.group(1)) + r"\.private_seg_size, (\d+)", text)
        scratch = int(s.group(1)) if s else 0
        print(f"{kern}{targs}: {vgpr} VGPRs, {scratch} B of scratch")
        assert vgpr <= BUDGET, f"{kern}{targs}: {vgpr} VGPRs, budget {BUDGET}"
        assert scratch == 0, f"{kern}{targs}: {scratch} B of scratch"
        b = re.search(r"^" + re.escape(m.group(1)) + r":", text, re.M)
        body = text[b.end():text.index(".amdhsa_kernel " + m.group(1), b.end())]
        assert not re.search(r"v_(fma|fmac|fmamk|fmaak|mad|mac|madmk|madak|pk_fma)_(legacy_)?f32", body), f"{kern}{targs}: a float32 multiply-add in the kernel"
        assert not re.search(r"v_(sqrt|rsq|div_scale|div_fmas|div_fixup)_f32", body), f"{kern}{targs}: a float32 root or division in the kernel"
        if "count" in kern:
            assert re.search(r"v_(mul|add|sub)_f32", body), f"{kern}{targs}: no separate float32 arithmetic found"
