"""GPU tier (-m gpu): the device arithmetic under the bit-exact kernels, operation by operation ("arithmetic
probe").

``Context.arith_probe`` runs one kernel per operation that calls the product's own device function (csrc/arith_probe.h) on the vectors
of tests/arith_cases.py -- every special and their cross products, every float32 exponent, the edges of every branch, 2^24 and more
arguments of the restated acosf -- and the result is held against an independent numpy reference bit for bit (a NaN for a NaN).  The
same cases and assertions run on the host emulation in tests/test_arith_cpu.py; what only this tier can show is the device lowering:
the denormal mode, the division and root expansions, what the compiler makes of `fp contract(off)` and of the opaque float64 detour.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import arith_cases as AC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(hip_ctx):
    return hip_ctx.arith_probe


def test_the_probe_writes_its_elements_and_nothing_else(hip_ctx):
    """lengths around a wave and a block: the elements are the reference's, and -- read back with room behind them -- the sentinel
    stays where no element is"""
    import torch
    from moleculekit_amd import _lib
    dev = torch.device("cuda", hip_ctx.device)
    x = AC.unary32()[0]
    for n in (1, 63, 65, 255, 257, 1000):
        a, b = np.ascontiguousarray(x[100:100 + n]), np.ascontiguousarray(x[5000:5000 + n])
        da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        out = torch.full((n + 300,), -3.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        _lib._check(_lib.load().mkamd_selftest_arith(hip_ctx._h, _lib.ARITH_OPS["fadd"][0], n, da.data_ptr(), db.data_ptr(), None, out.data_ptr()))
        hip_ctx.synchronize()
        h = out.cpu().numpy()
        assert not AC.compare(h[:n], AC.reference("fadd", a, b)).size and (h[n:] == -3.0).all(), n
    with pytest.raises(ValueError, match="unknown"):
        _lib._check(_lib.load().mkamd_selftest_arith(hip_ctx._h, len(_lib.ARITH_OPS), 4, da.data_ptr(), db.data_ptr(), None, out.data_ptr()))
    with pytest.raises(ValueError, match="NULL"):
        _lib._check(_lib.load().mkamd_selftest_arith(hip_ctx._h, _lib.ARITH_OPS["fadd"][0], 4, da.data_ptr(), None, None, out.data_ptr()))


@pytest.mark.parametrize("group", list(AC.GROUPS))
def test_operations_match_their_references_on_the_device(probe, group):
    AC.check_group(probe, group)


def test_acosf_and_the_folded_angle_match_the_restatement_on_the_device(probe):
    AC.check_acos(probe)
