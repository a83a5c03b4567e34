"""CPU tier: register budgets of the periodic-wrap kernels.  No kernel may spill.

All three kernels are latency chains, not register problems: what hides a chain of dependent float divisions is other waves, so every
budget is at most 64 VGPRs -- eight waves per SIMD (512 / 64).
k_wrap_lanes holds, per lane, three running centres, the divisor, one atom (3 floats), the temporaries of an IEEE division (scale,
reciprocal, two residuals, quotient: about 8), three translations with their flags, the three box lengths and box centres, and the
addressing of coordinates, box and starts (64-bit base, the loop counter): about 36 values -- budget 40.
k_wrap_waves holds one axis' chain (centre, divisor, the division's temporaries), the three translations and flags every lane gets by
readlane, the chunk loop's addressing and up to 12 floats in flight between global memory and LDS (WRAP_CHUNK * 3 / 64): budget 48.
k_wrap_centre is the same loop with a gather (index, then three floats, per atom) and no apply: budget 32."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# mangled name -> max VGPRs; scratch is 0 for all
BUDGETS = {"13k_wrap_centreE": 32, "12k_wrap_lanesE": 40, "12k_wrap_wavesE": 48}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_wrap_kernels_stay_inside_their_register_budgets(tmp_path):
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
