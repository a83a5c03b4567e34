"""CPU tier: register budgets of the steric-clash kernels.  No kernel may spill.

The pair kernels read a candidate as one 16-byte record and an index word, run two dozen float32 operations and a root on it, and only
for a hit go on to three float64 products and a short binary search; what hides their loads is other waves, so the budget of EVERY
instantiation is 64 registers: eight waves per SIMD, the most the hardware schedules, as for the bond guesser's kernels.  The 27
neighbour boxes are counted, not tabulated, so nothing is indexed at run time and nothing goes to scratch.

The float32 arithmetic of the reference must stay separate multiplies, adds and subtractions: a fused multiply-add would change a
squared distance, and with it the list.  The one place fused multiply-adds belong is the correctly rounded root (mk_fsqrt_rn: two in
its short form, two in its repair of the special cases), so a pair kernel holds exactly four v_fma_f32, one v_rsq_f32 and one
v_sqrt_f32, no multiply-add of another kind, and no float64 multiply-add at all: the pre-filter is the kd-tree's unfused float64 sum.
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
KERNELS = [("14k_clash_select", ""), ("15k_clash_compact", ""), ("12k_clash_pack", ""), ("14k_clash_owners", "")]
KERNELS += [("20k_clash_pairs_thread", f"ILb{b}EE") for b in (0, 1)]
KERNELS += [("18k_clash_pairs_wave", f"ILb{b}EE") for b in (0, 1)]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_clash_kernels_stay_inside_their_register_budgets(tmp_path):
    asm = tmp_path / "capi.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "moleculekit_amd", "csrc", "capi.hip"), "-o", str(asm)],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    assert len(re.findall(r"^\s*\.set (_ZN5mkamd\d+k_clash_\S*)\.num_vgpr, ", text, re.M)) == len(KERNELS), "an instantiation this test does not know"
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
            count = lambda pat: len(re.findall(pat, body))   # noqa: E731
            assert count(r"v_(mad|mac|madmk|madak|fmamk|fmaak|pk_fma)_(legacy_)?f32") == 0, f"{kern}{targs}: a float32 multiply-add outside the root"
            assert count(r"v_(fma|fmac)_f32") == 4, f"{kern}{targs}: {count(r'v_(fma|fmac)_f32')} fused multiply-adds, the root has 4"
            assert count(r"v_rsq_f32") == 1 and count(r"v_sqrt_f32") == 1, f"{kern}{targs}: one root, in its two forms"
            assert count(r"v_(div_scale|div_fmas|div_fixup)_f32") == 0, f"{kern}{targs}: a float32 division in the kernel"
            assert count(r"v_(fma|fmac|mad)_f64") == 0, f"{kern}{targs}: a float64 multiply-add in the pre-filter"
            assert count(r"v_(pk_)?mul_f32") >= 3 and count(r"v_(pk_add|add|sub|subrev)_f32") >= 4, f"{kern}{targs}: the pair test's float32 arithmetic not found"
            assert count(r"v_mul_f64") >= 3 and count(r"v_add_f64") >= 5, f"{kern}{targs}: the pre-filter's float64 arithmetic not found"
