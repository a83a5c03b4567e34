"""CPU tier: register budgets of the proximity-selection kernels.  No kernel may spill.

The all-pairs kernel reads its sources through the scalar unit and runs eight float32 operations and a comparison per pair; the cell
kernel reads a 16-byte record per candidate.  What hides their loads is other waves, so the budget of EVERY kernel is 64 registers:
eight waves per SIMD, the most the hardware schedules, as for the bond guesser's and the clash kernels.

The float32 arithmetic of the reference must stay separate multiplies, adds and subtractions (packed or not: v_pk_mul_f32 / v_pk_add_f32
round each half like the scalar instruction): a fused multiply-add would change a squared distance and with it a boolean.  The all-pairs
kernel holds no float32 multiply-add at all.  The cell kernel holds exactly those of the three correctly rounded divisions of the
query's box computation (five each, between v_div_scale and v_div_fixup), which stand in front of the pair loop, and none of any other
kind.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
BUDGET = 64

# every kernel the launch plan can take (none is a template)
KERNELS = ["15k_within_gather", "15k_within_bounds", "14k_within_pairs", "13k_within_pack", "14k_within_cells"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_within_kernels_stay_inside_their_register_budgets(tmp_path):
    asm = tmp_path / "capi.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "moleculekit_amd", "csrc", "capi.hip"), "-o", str(asm)],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    assert len(re.findall(r"^\s*\.set (_ZN5mkamd\d+k_within_\S*)\.num_vgpr, ", text, re.M)) == len(KERNELS), "an instantiation this test does not know"
    for kern in KERNELS:
        m = re.search(r"\.set (_ZN5mkamd" + re.escape(kern) + r"\S*)\.num_vgpr, (\d+)", text)
        assert m, f"{kern}: kernel not found in the assembly"
        vgpr = int(m.group(2))
        s = re.search(r"\.set " + re.escape(m.group(1)) + r"\.private_seg_size, (\d+)", text)
        scratch = int(s.group(1)) if s else 0
        print(f"{kern}: {vgpr} VGPRs, {scratch} B of scratch")
        assert vgpr <= BUDGET, f"{kern}: {vgpr} VGPRs, budget {BUDGET}"
        assert scratch == 0, f"{kern}: {scratch} B of scratch"
        if kern.endswith(("k_within_pairs", "k_within_cells")):
            b = re.search(r"^" + re.escape(m.group(1)) + r":", text, re.M)
            body = text[b.end():text.index(".amdhsa_kernel " + m.group(1), b.end())]
            count = lambda pat: len(re.findall(pat, body))   # noqa: E731
            assert count(r"v_(mad|mac|madmk|madak|fmamk|fmaak|pk_fma)_(legacy_)?f32") == 0, f"{kern}: a float32 multiply-add"
            divisions = count(r"v_div_fixup_f32")
            assert divisions == (3 if kern.endswith("cells") else 0), f"{kern}: {divisions} float32 divisions"
            assert count(r"v_(fma|fmac)_f32") == 5 * divisions, f"{kern}: {count(r'v_(fma|fmac)_f32')} fused multiply-adds outside the {divisions} divisions"
            # the pair loop: in the cell kernel everything behind the last division (a packed instruction is two operations)
            loop = body[body.rindex("v_div_fixup_f32"):] if divisions else body
            ops = lambda one, two: len(re.findall(one, loop)) + 2 * len(re.findall(two, loop))   # noqa: E731
            assert len(re.findall(r"v_(fma|fmac|mad|mac|pk_fma)_(legacy_)?f32", loop)) == 0, f"{kern}: a multiply-add in the pair loop"
            assert ops(r"v_mul_f32", r"v_pk_mul_f32") >= 3 and ops(r"v_(add|sub|subrev)_f32", r"v_pk_add_f32") >= 5, \
                f"{kern}: the pair test's float32 arithmetic not found"
            if not divisions:
                assert count(r"s_load_dwordx(4|8|16)") >= 2, f"{kern}: the sources are not read through the scalar unit"
