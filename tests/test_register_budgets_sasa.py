"""CPU tier: register budgets of the surface-area kernels.  k_sasa_count keeps a 16-KB neighbour list in LDS
per workgroup of four waves: nine workgroups fit a compute unit's LDS (nine waves per SIMD), which 56 registers or fewer allow;
the budget of 32 leaves the compiler room without ever making registers the limit.  No kernel may spill."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel-name fragment -> (max VGPRs, max scratch bytes)
BUDGETS = {
    "k_sasa_count": (32, 0),
    "k_sasa_pack": (24, 0),
    "k_sasa_scatter": (24, 0),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_sasa_kernels_stay_inside_their_register_budgets(tmp_path):
    asm = tmp_path / "capi.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "moleculekit_amd", "csrc", "capi.hip"), "-o", str(asm)],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    for frag, (max_vgpr, max_scratch) in BUDGETS.items():
        m = re.search(r"\.set (_ZN5mkamd\d+" + re.escape(frag) + r"\S*)\.num_vgpr, (\d+)", text)
        assert m, f"{frag}: kernel not found in the assembly"
        vgpr = int(m.group(2))
        s = re.search(r"\.set " + re.escape(m.group(1)) + r"\.private_seg_size, (\d+)", text)
        scratch = int(s.group(1)) if s else 0
        assert vgpr <= max_vgpr, f"{frag}: {vgpr} VGPRs, budget {max_vgpr}"
        assert scratch <= max_scratch, f"{frag}: {scratch} B of scratch, budget {max_scratch}"
    # the point loop must stay three subtractions, three multiplies and two adds: a fused multiply-add would change the counts
    m = re.search(r"^(_ZN5mkamd\d+k_sasa_count\S*):", text, re.M)
    body = text[m.end():text.index(".amdhsa_kernel " + m.group(1), m.end())]
    assert not re.search(r"v_(fma|fmac|mad|mac|pk_fma)_f32", body), "k_sasa_count: a fused multiply-add in the kernel"
