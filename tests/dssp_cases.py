"""tests/dssp_cases.py -- TEST INFRASTRUCTURE: backbones for the secondary-structure tests (CPU tier and GPU tier share them).

Seeded synthetic backbones built from ideal internal geometry (bond lengths and angles of Engh and Huber, torsions of the textbook
conformations), strands laid side by side as rigid bodies, the degenerate inputs of DESIGN.md section 19, and the golden structures
(tests/golden/dssp_cases.npz) with seeded noise.  A case is (coords float32 [N, 3, F], ca, nco, proline, chain).
"""
from __future__ import annotations

import os

import numpy as np

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dssp_cases.npz")

# Engh and Huber: bond lengths (A) and angles (degrees) of the peptide backbone
B_N_CA, B_CA_C, B_C_N, B_C_O = 1.458, 1.525, 1.329, 1.231
A_N_CA_C, A_CA_C_N, A_C_N_CA, A_CA_C_O = 111.0, 116.2, 121.7, 120.8
ALPHA, H310, PI, BETA_ANTI, BETA_PAR = (-57.0, -47.0), (-49.0, -26.0), (-57.0, -70.0), (-139.0, 135.0), (-119.0, 113.0)


def _place(a, b, c, bond, angle, torsion):
    """the atom bonded to c at `bond`, with angle (b, c, new) and torsion (a, b, c, new), in degrees"""
    angle, torsion = np.deg2rad(angle), np.deg2rad(torsion)
    bc = (c - b) / np.linalg.norm(c - b)
    n = np.cross(b - a, bc)
    n /= np.linalg.norm(n)
    m = np.cross(n, bc)
    d = np.array([-bond * np.cos(angle), bond * np.sin(angle) * np.cos(torsion), bond * np.sin(angle) * np.sin(torsion)])
    return c + d[0] * bc + d[1] * m + d[2] * n


def chain_from_torsions(phipsi, omega=180.0):
    """[(phi, psi)] per residue -> float64 [R, 4, 3]: N, CA, C, O"""
    R = len(phipsi)
    out = np.zeros((R, 4, 3))
    n = np.array([0.0, 0.0, 0.0])
    ca = np.array([B_N_CA, 0.0, 0.0])
    ang = np.deg2rad(A_N_CA_C)
    c = ca + B_CA_C * np.array([-np.cos(ang), np.sin(ang), 0.0])
    for r in range(R):
        if r > 0:
            pn, pca, pc = out[r - 1, 0], out[r - 1, 1], out[r - 1, 2]
            n = _place(pn, pca, pc, B_C_N, A_CA_C_N, phipsi[r - 1][1])
            ca = _place(pca, pc, n, B_N_CA, A_C_N_CA, omega)
            c = _place(pc, n, ca, B_CA_C, A_N_CA_C, phipsi[r][0])
        out[r, 0], out[r, 1], out[r, 2] = n, ca, c
        out[r, 3] = _place(n, ca, c, B_C_O, A_CA_C_O, phipsi[r][1] + 180.0)
    return out


def case_from_residues(res, proline=None, chain=None, frames=1, noise=0.0, seed=0):
    """float [R, 4, 3] (N, CA, C, O) -> a case; atoms in file order N, CA, C, O per residue"""
    R = len(res)
    xyz = np.asarray(res, np.float64).reshape(R * 4, 3)
    coords = np.repeat(xyz[:, :, None], frames, axis=2)
    if noise:
        coords = coords + np.random.default_rng(seed).normal(0.0, noise, coords.shape)
    base = 4 * np.arange(R)
    return (np.ascontiguousarray(coords, F32), (base + 1).astype(np.int32), np.stack([base, base + 2, base + 3], 1).astype(np.int32),
            np.zeros(R, np.int32) if proline is None else np.asarray(proline, np.int32),
            np.zeros(R, np.int32) if chain is None else np.asarray(chain, np.int32))


def strand_frame(res):
    """centre, axis (N -> C end), and two perpendiculars of a strand's CA trace"""
    ca = res[:, 1]
    centre = ca.mean(0)
    _, _, vt = np.linalg.svd(ca - centre)
    axis = vt[0] if np.dot(vt[0], ca[-1] - ca[0]) > 0 else -vt[0]
    u = vt[1]
    return centre, axis, u, np.cross(axis, u)


def lay_beside(res, theta, shift, dist, anti, phi=0.0, frame=None):
    """a rigid copy of a strand: turned by theta (degrees) about its axis, reversed about the first perpendicular where anti, moved
    `dist` along the perpendicular at angle phi (degrees, from the first towards the second) and `shift` along the axis"""
    centre, axis, u, v = strand_frame(res) if frame is None else frame
    t, ph = np.deg2rad(theta), np.deg2rad(phi)
    p = res - centre
    a, b, c = p @ axis, p @ u, p @ v
    b, c = b * np.cos(t) - c * np.sin(t), b * np.sin(t) + c * np.cos(t)
    if anti:
        a, c = -a, -c                                               # half a turn about u
    return (centre + (a + shift)[..., None] * axis + (b + dist * np.cos(ph))[..., None] * u + (c + dist * np.sin(ph))[..., None] * v)


# (theta, shift, dist, anti, phi) that pair a copy with the strand it was copied from: found once by a scan over the restatement
# (the placements with the most E labels)
PAIR_ANTI = (15.0, 0.0, 4.5, True, 0.0)
PAIR_PAR = (-30.0, -1.0, 4.8, False, 60.0)


def hairpin(n=8, **kw):
    s = chain_from_torsions([BETA_ANTI] * n)
    return case_from_residues(np.concatenate([s, lay_beside(s, *PAIR_ANTI)]), **kw)


def parallel_sheet(n=8, strands=3, **kw):
    s = chain_from_torsions([BETA_PAR] * n)
    frame, parts = strand_frame(s), [s]
    for _ in range(strands - 1):
        parts.append(lay_beside(parts[-1], *PAIR_PAR, frame=frame))
    return case_from_residues(np.concatenate(parts), **kw)


def bulged_ladder(n=10, **kw):
    """a hairpin whose second strand carries one residue more in its middle, pushed out of the sheet: two ladders, one bulge"""
    s = chain_from_torsions([BETA_ANTI] * n)
    frame = strand_frame(s)
    t = lay_beside(s, *PAIR_ANTI, frame=frame)
    h = n // 2 + 1
    extra = t[h - 1] + 5.0 * frame[3]       # (a copy of the residue in front of it: the next residue's hydrogen keeps its direction)
    return case_from_residues(np.concatenate([s, t[:h], extra[None], t[h:]]), **kw)


def swapped_partner(n=12, **kw):
    """strand A, then the copy of its second half, then the copy of its first half: the ladder that starts later on A has its
    partners EARLIER in the sequence -- the difference rule 5 takes as an unsigned number is negative"""
    s = chain_from_torsions([BETA_PAR] * n)
    t = lay_beside(s, *PAIR_PAR)
    h = n // 2
    return case_from_residues(np.concatenate([s, t[h + 1:], t[:h]]), **kw)


def golden_case(structure, frames=1, noise=0.0, seed=0):
    """a golden structure's backbone (tests/golden/dssp_cases.npz) as a case, and its naming fields"""
    g = np.load(GOLDEN)
    f = {k: g[f"{structure}_{k}"] for k in ("name", "resname", "resid", "insertion", "chain", "segid")}
    name = f["name"]
    res = np.cumsum(np.r_[True, (f["resid"][1:] != f["resid"][:-1]) | (f["insertion"][1:] != f["insertion"][:-1]) | (f["chain"][1:] != f["chain"][:-1])]) - 1
    R = int(res[-1]) + 1
    ca = np.zeros(R, np.int32)
    nco = np.zeros((R, 3), np.int32)
    for k, a in enumerate(name):
        if a == "CA":
            ca[res[k]] = k
        else:
            nco[res[k], "NCO".index(a)] = k
    coords = np.repeat(g[f"{structure}_coords"], frames, axis=2).astype(np.float64)
    if noise:
        coords = coords + np.random.default_rng(seed).normal(0.0, noise, coords.shape)
    proline = (f["resname"][ca] == "PRO").astype(np.int32)
    chain = np.unique(f["chain"][ca], return_inverse=True)[1].astype(np.int32)
    return (np.ascontiguousarray(coords, F32), ca, nco, proline, chain), f


def cases():
    """name -> case: every path of the rules at the smallest sizes that reach it"""
    out = {}
    out["alpha"] = case_from_residues(chain_from_torsions([ALPHA] * 20))
    out["h310"] = case_from_residues(chain_from_torsions([H310] * 12))
    out["pi_in_alpha"] = case_from_residues(chain_from_torsions([ALPHA] * 8 + [PI] * 8 + [ALPHA] * 8))
    out["hairpin"] = hairpin()
    out["parallel_sheet"] = parallel_sheet()
    out["bulge"] = bulged_ladder()
    out["swapped_partner"] = swapped_partner()
    # two chains: the break inside a would-be turn (a helix cut in two) and inside a would-be bridge window (a strand cut in two)
    out["helix_two_chains"] = case_from_residues(chain_from_torsions([ALPHA] * 16), chain=[0] * 7 + [1] * 9)
    out["hairpin_two_chains"] = hairpin(chain=[0] * 3 + [1] * 13)
    out["hairpin_chain_per_strand"] = hairpin(chain=[0] * 8 + [1] * 8)
    # prolines at donor positions
    out["helix_prolines"] = case_from_residues(chain_from_torsions([ALPHA] * 16), proline=[0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0])
    out["hairpin_prolines"] = hairpin(proline=[0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0])
    for R in (1, 2, 5, 6, 7):
        out[f"alpha_{R}"] = case_from_residues(chain_from_torsions([ALPHA] * R))
    # two atoms closer than 0.5 A: the N of residue 6 next to the O of residue 2 (E = -9.9 whatever the rest)
    c = case_from_residues(chain_from_torsions([ALPHA] * 14))
    c[0][c[2][6, 0]] = c[0][c[2][2, 2]] + F32(0.2)
    out["close_atoms"] = c
    # C and O of residue 5 coincide: residue 6 has no direction for its hydrogen (H = N)
    c = case_from_residues(chain_from_torsions([ALPHA] * 14))
    c[0][c[2][5, 2]] = c[0][c[2][5, 1]]
    out["coincident_c_o"] = c
    c = case_from_residues(chain_from_torsions([ALPHA] * 14), frames=3)
    c[0][c[1][6], 1, 1] = np.nan
    out["nan_coordinate"] = c
    out["helix_noise_frames"] = case_from_residues(chain_from_torsions([ALPHA] * 12 + [BETA_ANTI] * 4), frames=66, noise=0.25, seed=3)
    return out


def noisy_3ptb(frames=130):
    """3PTB with seeded Gaussian noise of 0.3 A: energies near -0.5 and bends near 70 degrees in some frame or other"""
    return golden_case("3ptb", frames=frames, noise=0.3, seed=11)[0]
