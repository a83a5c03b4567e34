"""GPU tier of the surface area (moleculekit_amd/sasa.py): the kernels on the device bit-equal to the float32 restatement
(tests/sasa_restatement.py), MetricSasa against the arrays the reference holds for its own test at the reference's tolerances
(atom 0.1, residue 0.3, atom selection 1e-2 square Angstrom).  Reads nothing of the reference: tests/golden only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sasa_cases as C  # noqa: E402
import sasa_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def S():
    from moleculekit_amd import sasa
    return sasa


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def dev_call(S, torch, xyz_nm, radii_nm, **kw):
    """mkamd_sasa_dev on nanometre inputs as they are (coord_div = 1): the restatement's inputs, no unit conversion in between"""
    from moleculekit_amd import _lib
    N, Fr = xyz_nm.shape[1], xyz_nm.shape[0]
    mapping = kw.get("mapping")
    mapping = np.arange(N, dtype=np.int32) if mapping is None else np.ascontiguousarray(mapping, np.int32)
    mask = np.ones(N, np.int32) if kw.get("sel") is None else np.asarray(kw["sel"]).astype(np.int32)
    out = kw.get("out")
    out = np.zeros((Fr, int(mapping.max()) + 1), F32) if out is None else out
    d = [torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in (xyz_nm, radii_nm, mapping, mask, out)]
    ctx = _lib.default_context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    _lib._check(_lib.load().mkamd_sasa_dev(ctx._h, d[0].data_ptr(), N, Fr, d[1].data_ptr(), int(kw.get("n_points", 960)), d[2].data_ptr(),
                                           d[3].data_ptr(), 1.0, d[4].data_ptr(), out.shape[1]))
    return d[4].cpu().numpy()


@pytest.fixture(scope="module")
def restated():
    xyz, rad, mapping = C.fixture_nm()
    return xyz, rad, mapping, R.areas(xyz, rad, 960)


def test_fixture_frames_bit_equal_to_the_restatement(S, torch, restated):
    xyz, rad, mapping, area = restated
    assert np.array_equal(bits(dev_call(S, torch, xyz, rad)), bits(area))
    exp = R.scatter(area, mapping, np.ones(4480, bool), np.zeros((2, 277), F32))
    assert np.array_equal(bits(dev_call(S, torch, xyz, rad, mapping=mapping)), bits(exp))
    # the public calls, from Angstrom: the division by 10 happens on the device (tensor API) / in the host entry point
    mol, g = C.fixture()
    p = g["protein"]
    rad_A = np.array([1.2 if e == "H" else 1.7 if e == "C" else 1.55 if e == "N" else 1.52 if e == "O" else 1.8 for e in g["element"][p]], F32) + F32(1.4)
    exp_A = R.areas(xyz, rad_A / F32(10), 960) * 100
    xa = torch.as_tensor(np.ascontiguousarray(np.transpose(mol.coords[p], (2, 0, 1))), device="cuda")
    got = S.sasa_trajectory(xa, rad_A)
    assert got.shape == (2, 4480) and got.dtype == torch.float32
    assert np.array_equal(bits(got.cpu().numpy()), bits(exp_A))
    host = S.sasa(mol.coords, rad_A, keep=p)
    assert np.array_equal(bits(host), bits(exp_A))


@pytest.mark.parametrize("n_points", [1, 60, 960, 1000])
@pytest.mark.parametrize("n", [1, 2, 7, 300, 5000])
def test_globules_bit_equal_to_the_restatement(S, torch, n, n_points):
    xyz, rad = C.globule(n, seed=n + n_points)
    assert np.array_equal(bits(dev_call(S, torch, xyz, rad, n_points=n_points)), bits(R.sasa(xyz, rad, n_points)))


def test_isolated_buried_subset_and_residue_mapping(S, torch):
    n = 960
    r = F32(0.31)
    got = dev_call(S, torch, np.zeros((1, 1, 3), F32), np.array([r]), n_points=n)
    assert got[0, 0] == ((F32(4.0 * np.pi / n) * F32(n)) * r) * r
    xyz = np.array([[[0.0, 0.0, 0.0], [0.05, 0.0, 0.0]]], F32)
    got = dev_call(S, torch, xyz, np.array([0.2, 1.0], F32), n_points=n)
    assert got[0, 0] == 0.0 and got[0, 1] > 0.0
    xyz, rad = C.globule(300, seed=5, frames=3)
    rng = np.random.default_rng(5)
    sel = rng.random(300) < 0.4
    mapping = np.cumsum(rng.random(300) < 0.2).astype(np.int32)
    pre = np.full((3, int(mapping.max()) + 1), -1, F32)
    got = dev_call(S, torch, xyz, rad, n_points=60, mapping=mapping, sel=sel, out=pre.copy())
    assert np.array_equal(bits(got), bits(R.sasa(xyz, rad, 60, mapping=mapping, sel=sel, out=pre.copy())))
    # more neighbours than the kernel's list in LDS holds
    from moleculekit_amd import _lib  # noqa: F401
    xyz, _ = C.globule(1224, seed=2)
    xyz = (xyz * F32(0.25)).astype(F32)
    rad = np.full(1224, 0.9, F32)
    sel = np.zeros(1224, bool)
    sel[::97] = True
    assert np.array_equal(bits(dev_call(S, torch, xyz, rad, n_points=60, sel=sel)), bits(R.sasa(xyz, rad, 60, sel=sel)))


def test_metricsasa_atom_mode_against_the_reference_held_array(S):
    mol, g = C.fixture()
    got = S.MetricSasa(g["protein"], mode="atom").project(mol)
    d = np.abs(got - g["sasa_atom"])
    print(f"atom: max |diff| {d.max():.3g}, entries outside 0.1: {int((d > 0.1).sum())}")
    assert got.shape == (2, 4480) and got.dtype == np.float32
    assert np.allclose(got, g["sasa_atom"], atol=0.1), f"Failed with max diff {d.max()}"


def test_metricsasa_residue_mode_against_the_reference_held_array(S):
    mol, g = C.fixture()
    got = S.MetricSasa(g["protein"], mode="residue").project(mol)
    d = np.abs(got - g["sasa_residue"])
    print(f"residue: max |diff| {d.max():.3g}, entries outside 0.3: {int((d > 0.3).sum())}")
    assert got.shape == (2, 277)
    assert np.allclose(got, g["sasa_residue"], atol=0.3), f"Failed with max diff {d.max()}"


def test_metricsasa_selection_and_filtering(S):
    """the reference's test_selection_and_filtering"""
    mol, g = C.fixture()
    p = g["protein"]
    one = S.MetricSasa([20], mode="atom").project(mol)          # filtersel "all": MOL and the ions stay in the system
    ref = S.MetricSasa(p, filtersel="all", mode="atom").project(mol)
    assert one.shape == (2, 1)
    assert np.allclose(one, ref[:, [20]], atol=1e-2), f"max diff {np.abs(one - ref[:, [20]]).max()}"
    alone = S.MetricSasa([20], filtersel=[20], mode="atom").project(mol)
    assert not np.allclose(alone, ref[:, [20]], atol=1e-2)


def test_two_runs_bitwise_equal_and_batch_equals_frame_by_frame(S, torch):
    xyz, rad, mapping = C.fixture_nm()
    rng = np.random.default_rng(3)
    big = np.ascontiguousarray((np.repeat(xyz, 32, axis=0) * F32(10) + rng.uniform(-0.02, 0.02, size=(64, 4480, 3)).astype(F32)).astype(F32))
    rad_A = (rad * F32(10)).astype(F32)
    t = torch.as_tensor(big, device="cuda")
    a = S.sasa_trajectory(t, rad_A, atom_mapping=mapping).cpu().numpy()
    b = S.sasa_trajectory(t, rad_A, atom_mapping=mapping).cpu().numpy()
    assert a.shape == (64, 277) and np.array_equal(bits(a), bits(b))
    for f in (0, 1, 31, 63):
        assert np.array_equal(bits(S.sasa_trajectory(t[f], rad_A, atom_mapping=mapping).cpu().numpy()[0]), bits(a[f])), f
    one_by_one = np.concatenate([S.sasa_trajectory(t[f:f + 1], rad_A, atom_mapping=mapping).cpu().numpy() for f in range(64)])
    assert np.array_equal(bits(one_by_one), bits(a))
    out = torch.full((64, 277), -5.0, device="cuda")
    assert S.sasa_trajectory(t, rad_A, atom_mapping=mapping, out=out) is out and np.array_equal(bits(out.cpu().numpy()), bits(a))


def test_coincident_atoms_raise(S, torch):
    xyz = np.array([[[0.0, 0.0, 0.0], [1e-5, 0.0, 0.0], [10.0, 0.0, 0.0]]], F32)       # Angstrom: 1e-6 nm apart
    with pytest.raises(ValueError, match="on top of one another"):
        S.sasa_trajectory(torch.as_tensor(xyz, device="cuda"), np.full(3, 3.0, F32))
    with pytest.raises(ValueError, match="on top of one another"):
        S.sasa(np.ascontiguousarray(np.transpose(xyz, (1, 2, 0))), np.full(3, 3.0, F32))
    # and the context is usable afterwards
    ok = S.sasa_trajectory(torch.as_tensor(xyz[:, [0, 2]], device="cuda"), np.full(2, 3.0, F32), n_points=60).cpu().numpy()
    assert np.all(ok == ok[0, 0]) and ok[0, 0] > 0
