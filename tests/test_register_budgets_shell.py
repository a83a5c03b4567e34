"""CPU tier: register budgets of the shell-count kernels.  No kernel may spill.

k_shell_frames keeps C x NE running counts, 3 C centre coordinates and a batch of 12 second-atom coordinates per lane ((C, NE) =
(4, 5), (2, 9), (1, 17), (1, 33): 44 .. 48 values before any addressing); the build takes 48 .. 74 registers.  The budget of 84 is
what six waves per SIMD allow (512 / 84): the kernel hides its coordinate loads behind other waves, not behind a deep pipeline of
its own.  k_shell_atoms' counts are scalar (a ballot's population), so with up to 9 edges it holds little more than its 3 x JPL
coordinates: 64 registers -- eight waves per SIMD; its waves are short.  With 17 and 33 edges the scalar registers run out (100 are
in use) and the compiler moves counts into vector registers: 84 for 17 edges, 168 for 33 (three waves per SIMD: the 32-shell call
on a single structure is rare and small).  The pair arithmetic of the open (pbc = 0) kernels must stay separate subtractions,
multiplies and adds: a fused multiply-add would change d2 and with it a count."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (kernel, template arguments as mangled) -> max VGPRs; scratch is 0 for all
BUDGETS = {}
for pbc in (0, 1):
    for ne, c in ((5, 4), (9, 2), (17, 1), (33, 1)):
        BUDGETS[("14k_shell_frames", f"ILb{pbc}ELi{ne}ELi{c}EE")] = 84
    for ne, cap in ((5, 64), (9, 64), (17, 84), (33, 168)):
        for jpl in (1, 4):
            BUDGETS[("13k_shell_atoms", f"ILb{pbc}ELi{ne}ELi{jpl}EE")] = cap


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_shell_kernels_stay_inside_their_register_budgets(tmp_path):
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
        if "ILb0E" in targs:
            b = re.search(r"^" + re.escape(m.group(1)) + r":", text, re.M)
            body = text[b.end():text.index(".amdhsa_kernel " + m.group(1), b.end())]
            assert not re.search(r"v_(fma|fmac|mad|mac|pk_fma)_f32", body), f"{kern}{targs}: a fused multiply-add in the open kernel"
            assert not re.search(r"v_sqrt_f32|v_rsq_f32", body), f"{kern}{targs}: a root in the kernel"
