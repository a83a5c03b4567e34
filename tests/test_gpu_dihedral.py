"""GPU tier of the dihedral angles (moleculekit_amd/dihedral.py): the conditions of tests/test_dihedral_cpu.py
on the device -- tensor route and host route, both lane assignments forced through the context's avoid bits (1024: not the
frame-lane kernel, 2048: not the dihedral-lane kernel), the kernel taken asserted through last_dist_kernel().  Terms bit-equal to
the numpy restatement; angle, degrees and sin / cos no further from the float64 function of the terms than the restatement itself
(E_ref computed here from the restatement over >= 100 000 values, no margin); collinear and NaN cases exactly; MetricDihedral on the
carried trajectory against the reference-held array.  Reads tests/golden only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dihedral_cases as C  # noqa: E402
import dihedral_restatement as R  # noqa: E402
from test_dihedral_cpu import check_accuracy, synthetic_sets  # noqa: E402

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
KERNELS = (("k_dihedral_frames", 2048), ("k_dihedral_atoms", 1024))


@pytest.fixture(scope="module")
def ctx():
    from moleculekit_amd import _lib
    c = _lib.default_context()
    yield c
    c.set_dist_kernels(0)


@pytest.fixture(scope="module")
def real():
    from moleculekit_amd.dihedral import Dihedral
    mol, g = C.fixture()
    quads = np.array(Dihedral.dihedralsToIndexes(mol, Dihedral.proteinDihedrals(mol, mol.protein), mol.protein), np.int64)
    return mol, g, quads, R.terms(mol.coords, quads)


def both_routes(ctx, coords, quads, box, mode, avoid):
    """the host route's result, after asserting that the tensor route gives the same bits and that the forced kernel ran"""
    import torch
    from moleculekit_amd.dihedral import dihedral_trajectory, dihedrals
    ctx.set_dist_kernels(avoid)
    try:
        host = dihedrals(coords, quads, box=box, out=mode, ctx=ctx)
        k_host = ctx.last_dist_kernel()
        dev = dihedral_trajectory(torch.as_tensor(coords).cuda(), quads, box=None if box is None else torch.as_tensor(box).cuda(),
                                  out=mode, ctx=ctx)
        torch.cuda.synchronize()
        k_dev = ctx.last_dist_kernel()
    finally:
        ctx.set_dist_kernels(0)
    name = [n for n, a in KERNELS if a == avoid]
    if name:
        assert name[0] in k_host and name[0] in k_dev, (k_host, k_dev)
    assert C.bit_equal(dev.cpu().numpy(), host), "tensor route and host route differ"
    return host


def all_cases():
    cases = [(c, q, None) for c, q in C.scale_cases() + C.shape_cases()]
    c, q, b = C.periodic_case()
    return cases + [(c, q, b), (c, q, np.zeros_like(b))] + [C.collinear_case() + (None,), C.nan_case() + (None,)]


def test_terms_bit_equal_every_case_both_kernels_both_routes(ctx, real):
    mol, _, quads, t = real
    for coords, q, box in all_cases() + [(mol.coords, quads, None), (mol.coords, quads, mol.box)]:
        want = R.terms(coords, q, box)
        for name, avoid in KERNELS:
            got = both_routes(ctx, coords, q, box, "terms", avoid)
            assert got.shape == want.shape and C.bit_equal(got, want), \
                f"{name} {coords.shape} {q.shape}: {int((got.view(U32) != want.view(U32)).sum())} of {want.size} terms differ"
    assert C.bit_equal(R.terms(mol.coords, quads), t)


def test_host_route_packed_and_whole_array_uploads_bit_equal(ctx):
    """The host route uploads only the rows of the atoms the quads name when those are at most a quarter of a > 1-MB array
    (csrc/host_pack.h; smaller arrays never pack): 150 quads drawn unsorted and with repeats from 600 of 3000 atoms, 40 frames
    (1.44 MB), with and without a box -- packed (mask 0) and with the whole array uploaded (avoid bit 32), the restatement's bits."""
    from moleculekit_amd.dihedral import dihedrals
    rng = np.random.default_rng(61)
    N, F = 3000, 40
    box = (np.array([20.0, 24.0, 16.0])[:, None] + rng.uniform(-1, 1, size=(3, F))).astype(F32)
    steps = rng.normal(size=(N, 3, F))
    walk = np.cumsum(steps * (1.5 / np.linalg.norm(steps, axis=1, keepdims=True)), axis=0)
    coords = np.ascontiguousarray((walk - np.floor(walk / box[None]) * box[None]).astype(F32))
    quads = rng.permutation(N)[:600][rng.integers(0, 600, size=(150, 4))].astype(U32)
    named = np.unique(quads)
    assert len(named) * 4 <= N and len(named) < quads.size and np.any(np.diff(quads.ravel().astype(np.int64)) < 0)
    for b in (None, box):
        want = R.terms(coords, quads, b)
        for mask in (0, 32):
            ctx.set_dist_kernels(mask)
            try:
                got = dihedrals(coords, quads, box=b, out="terms", ctx=ctx)
            finally:
                ctx.set_dist_kernels(0)
            assert got.shape == want.shape and C.bit_equal(got, want), (b is not None, mask)


def test_plan_chooses_by_frames(ctx):
    for F, name in ((1, "k_dihedral_atoms"), (63, "k_dihedral_atoms"), (64, "k_dihedral_frames"), (200, "k_dihedral_frames")):
        coords, quads = C.random_case(40, 33, F, 5)
        both_routes(ctx, coords, quads, None, "sincos", 0)
        assert name in ctx.last_dist_kernel(), (F, ctx.last_dist_kernel())


def test_accuracy_synthetic_sets(ctx):
    check_accuracy(lambda c, q, b, mode, avoid: both_routes(ctx, c, q, b, mode, {2: 2048, 1: 1024}[avoid]), synthetic_sets(), "synthetic")


def test_accuracy_real_trajectory(ctx, real):
    mol, _, quads, _ = real
    check_accuracy(lambda c, q, b, mode, avoid: both_routes(ctx, c, q, b, mode, {2: 2048, 1: 1024}[avoid]), [(mol.coords, quads, None)], "real")


def test_collinear_and_nan_exactly(ctx):
    coords, quads = C.collinear_case()
    ncoords, nquads = C.nan_case()
    hit = np.zeros((ncoords.shape[2], nquads.shape[0]), bool)
    hit[2] = np.any(nquads == 5, axis=1)
    hit[65] |= np.any(nquads == 9, axis=1)
    for _, avoid in KERNELS:
        sc = both_routes(ctx, coords, quads, None, "sincos", avoid)
        assert np.all(sc[:, 0] == 0) and np.all(sc[:, 1] == 1) and np.all(sc[:, 4] == 0) and np.all(sc[:, 5] == 1)
        for mode in ("radians", "degrees"):
            a = both_routes(ctx, coords, quads, None, mode, avoid)
            assert np.all(a[:, 0] == 0) and np.all(a[:, 2] == 0) and np.all(a[:, 1] != 0)
            assert np.array_equal(np.isnan(both_routes(ctx, ncoords, nquads, None, mode, avoid)), hit)
        assert np.array_equal(np.isnan(both_routes(ctx, ncoords, nquads, None, "sincos", avoid)), np.repeat(hit, 2, axis=1))
        t = both_routes(ctx, ncoords, nquads, None, "terms", avoid)
        assert np.array_equal(np.isnan(t[..., 0]), hit) and np.array_equal(np.isnan(t[..., 1]), hit)


def test_metricdihedral_end_to_end(ctx, real):
    from moleculekit_amd.dihedral import MetricDihedral
    mol, g, quads, t = real
    met = MetricDihedral(protsel=mol.protein)
    got = met.project(mol)
    assert got.shape == (200, 1104) and got.dtype == F32
    assert np.allclose(got, g["ref"], atol=1e-3)                                      # the reference's own assertion
    restated = R.project(t, True)
    rad, deg, sc = R.truth(t)
    e_ref = R.worst(restated, sc)
    d_got, d_res = float(np.abs(got - g["ref"]).max()), float(np.abs(restated - g["ref"]).max())
    print(f"max|got - held| {d_got:.3e}; max|restatement - held| {d_res:.3e}; E_ref {e_ref:.3e}")
    assert d_got <= d_res + e_ref
    degrees = MetricDihedral(protsel=mol.protein, sincos=False).project(mol)
    assert degrees.shape == (200, 552) and R.worst(degrees, deg) <= R.worst(R.project(t, False), deg)
    assert np.allclose(np.sin(np.deg2rad(degrees)), got[:, 0::2], atol=1e-3) and np.allclose(np.cos(np.deg2rad(degrees)), got[:, 1::2], atol=1e-3)
    m = met.getMapping(mol)
    assert len(m["description"]) == 1104 and list(m["atomIndexes"])[2] == list(quads[1])
    assert list(m["description"])[0].startswith("Sine of angle of (") and list(m["description"])[1].startswith("Cosine of angle of (")


def test_dialanine_literals(ctx):
    from moleculekit_amd.dihedral import MetricDihedral
    mol, sel, expected = C.dialanine()
    got = MetricDihedral(protsel=sel).project(mol)
    assert ctx.last_dist_kernel().startswith("mkamd::k_dihedral_atoms")
    assert np.allclose(expected, got)


def test_library_refusals(ctx):
    import ctypes
    from moleculekit_amd import _lib
    L = _lib.load()
    coords, quads = C.random_case(10, 3, 2, 1)
    out = np.zeros((2, 6), F32)
    p = _lib._ptr

    def call(coords_p=p(coords), N=10, F=2, box=None, bf=2, quads_p=p(quads), D=3, mode=3, out_p=p(out)):
        return L.mkamd_dihedrals_host(ctx._h, coords_p, N, F, box, bf, quads_p, D, mode, out_p)

    assert call() == 0
    for kw, msg in ((dict(mode=4), "mode"), (dict(N=5), "out of range"), (dict(coords_p=None), "NULL"), (dict(out_p=None), "NULL"),
                    (dict(box=p(np.zeros((3, 3), F32)), bf=3), "box"), (dict(F=1 << 30, D=1 << 30), "too large")):
        assert call(**kw) != 0
        with pytest.raises(Exception, match=msg):
            _lib._check(call(**kw))
    assert call() == 0                                                                # the context stays usable
