"""CPU tier: register budgets of the triclinic periodic-wrap kernels.  No kernel may spill.

Like their rectangular siblings these are latency chains, hidden by other waves: every budget is at most 64 VGPRs -- eight waves per
SIMD (512 / 64) -- and each is the count hipcc gives at -O3 plus the sibling file's headroom of a few registers.
k_wrap_cell_prep holds, per lane, the nine float64 box entries, the three half diagonals, and one shift combination's sums, bound and
trial position in float64 (the trial vector itself goes to the frame's record at once): 60, at its launch bound of 64.
k_wrap_cell_lanes holds what k_wrap_lanes holds (three running centres, an atom, the IEEE division's temporaries, addressing) plus
the recentring pair per axis and the decision: three float64 dx with the half diagonals and box entries (rectangular: 37), the search's
start, trial and squared lengths on top (compact: 58), or three float32 centres with float64 shifts (triclinic: 38).
k_wrap_cell_waves keeps the decision in one lane and the chain in three; what every lane holds is the broadcast result: 30 / 30 / 21."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# mangled name (a prefix) -> max VGPRs; scratch is 0 for all.  ILi0E / ILi1E / ILi2E: rectangular / compact / triclinic
BUDGETS = {"16k_wrap_cell_prepE": 64,
           "17k_wrap_cell_lanesILi0EE": 40, "17k_wrap_cell_lanesILi1EE": 62, "17k_wrap_cell_lanesILi2EE": 42,
           "17k_wrap_cell_wavesILi0EE": 34, "17k_wrap_cell_wavesILi1EE": 34, "17k_wrap_cell_wavesILi2EE": 24}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_wrap_cell_kernels_stay_inside_their_register_budgets(tmp_path):
    asm = tmp_path / "capi.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "moleculekit_amd", "csrc", "capi.hip"), "-o", str(asm)],
                          stderr=subprocess.DEVNULL)
    text = asm.read_text()
    assert max(BUDGETS.values()) <= 64
    for kern, max_vgpr in BUDGETS.items():
        m = re.search(r"\.set (_ZN5mkamd" + re.escape(kern) + r"\S*)\.num_vgpr, (\d+)", text)
        assert m, f"{kern}: kernel not found in the assembly"
        vgpr = int(m.group(2))
        a = re.search(r"\.set " + re.escape(m.group(1)) + r"\.num_agpr, (\d+)", text)
        s = re.search(r"\.set " + re.escape(m.group(1)) + r"\.private_seg_size, (\d+)", text)
        scratch = int(s.group(1)) if s else 0
        assert vgpr <= max_vgpr, f"{kern}: {vgpr} VGPRs, budget {max_vgpr}"
        assert (int(a.group(1)) if a else 0) == 0, f"{kern}: accumulation registers in use"
        assert scratch == 0, f"{kern}: {scratch} B of scratch"
