"""CPU tier: the class flush of the tile kernels (round 11) on the host emulation of the product's kernels -- one
scalar branch on `fast` per class, the cutoff applied to the class minimum as a MASKED minimum (mk_min_bits_where, csrc/kernels.h; the
emulation compiles its plain C++ form).  The batches of tests/class_flush_cases.py, one item per case, at both depths: the handle call
with the cover fold on and off, the plain call and force_general are bit for bit the same, within tests/cases.py: TOL of the oracle, and
show what the cases were built for (a voxel at exactly 5 A stays out, one 1e-3 A nearer comes in, an atom on a voxel centre gives 1.0f).
The mutation check: with the helper ignoring the cutoff (-DMK_DIAG=512) the same comparison must fail."""
import numpy as np
import pytest

from tests import class_flush_cases as CF
from tests import emu_build as E
from tests import emu_class_flush_build as EF
from tests import emu_cover_fold_build as EC
from tests.cases import TOL, oracle_lattice

CHAIN = dict(prepass_mode=0, tile_team=0, tile_items=0, direct=0)

_plain = {}


def plain(K):
    """the plain call's features of a batch, computed once"""
    if K not in _plain:
        xyz, offs, sig, org, nv = CF.batch(K)
        out, err = E.voxelize_lattice(xyz, offs, sig, org, nv, 1.0, tile_k=K, **CHAIN)
        assert err == 0
        out.setflags(write=False)
        _plain[K] = out
    return _plain[K]


@pytest.mark.parametrize("K", [4, 8])
def test_every_path_flushes_the_same_bits(K):
    xyz, offs, sig, org, nv = CF.batch(K)
    ref = plain(K)
    on = EC.voxelize(xyz, offs, sig, org, nv, tile_k=K)
    off = EC.voxelize(xyz, offs, sig, org, nv, tile_k=K, cover_fold=-1)
    gen, err = E.voxelize_lattice(xyz, offs, sig, org, nv, 1.0, tile_k=K, force_general=True, **CHAIN)
    assert on["err"] == 0 and off["err"] == 0 and err == 0
    assert int(on["masks"][0]) & EC.class_bit(on["table"], np.float32(1.7))            # the fold is live: 1.7 A is covered by channel 7
    assert np.array_equal(on["out"], ref) and np.array_equal(off["out"], ref) and np.array_equal(gen, ref)
    exp = oracle_lattice(xyz, offs, sig.astype(np.float64), org, nv, 1.0)
    worst = np.abs(ref.astype(np.float64) - exp).max()
    print("K = %d: max-abs-err against the oracle %.3e" % (K, worst))
    assert worst <= TOL
    CF.check_values(ref, K)


def test_a_team_of_waves_flushes_the_same_bits():
    """one item per call, a team of four waves per tile: every wave flushes its own partial minima"""
    K = 8
    xyz, offs, sig, org, nv = CF.batch(K)
    ref = plain(K)
    for b in range(len(offs) - 1):
        a0, a1 = int(offs[b]), int(offs[b + 1])
        team, err = E.voxelize_lattice(xyz[a0:a1], np.array([0, a1 - a0]), sig[a0:a1], org[b:b + 1], nv, 1.0, tile_k=K, prepass_mode=0, tile_team=1,
                                       tile_items=0, direct=0)
        assert err == 0 and np.array_equal(team[0], ref[b]), CF.ITEMS[b]


@pytest.mark.parametrize("K", [4, 8])
def test_the_mutant_that_ignores_the_cutoff_is_caught(K):
    xyz, offs, sig, org, nv = CF.batch(K)
    ref = plain(K)
    mut = EF.mutant_handle(xyz, offs, sig, org, nv, tile_k=K)
    mplain, err = EF.mutant_plain(xyz, offs, sig, org, nv, 1.0, tile_k=K, **CHAIN)
    assert mut["err"] == 0 and err == 0
    assert not np.array_equal(mut["out"], ref) and not np.array_equal(mplain, ref)
    # ... at the very voxels the case was built for: exactly 5 A from the lone atom, which the cutoff keeps at 0.0f
    ring = CF.at_exactly_five(K)
    assert mplain[0][ring, 0].any() and mut["out"][0][ring, 0].any()
    with pytest.raises(AssertionError):
        CF.check_values(mplain, K)
