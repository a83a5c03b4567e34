"""tools/bench_rings.py -- time the fused ring-interaction call beside a torch composition of the same work on the same device.

    python tools/bench_rings.py [--reps 20] [--warmup 3] [--out results.json]

Shapes: one pose (150 protein rings x 3 ligand rings x 1 frame), a protein's own rings (150 x 150 over 2 048 frames), cation-pi (150
rings x 200 cations x 2 048 frames).  The composition does what a torch user would write: gather the rings' atoms, mean, cross product
and normalisation per (ring, frame); minimum image, distance test, acos, thresholds and ``nonzero`` per (ring, partner, frame).  It is
NOT bit-faithful to the reference (torch's float32 acos, fused multiply-adds at the compiler's pleasure) -- it is the yardstick for
time only; the number of pairs it reports is printed beside the fused call's.

Both are timed with a host clock around work that ends in a device synchronise, alternating, after a warm-up of every shape; the
median and the spread (min .. max) of ``--reps`` repetitions are reported, one JSON line per shape.  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_system(seed, n_rings, n_second, F, kind, extent):
    """six-rings with random centres and orientations in a periodic cube; partners: rings (pipi) or single atoms (cationpi)"""
    rng = np.random.default_rng(seed)

    def ring(centre):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        ang = 2 * np.pi * np.arange(6) / 6
        return centre + 1.39 * (np.cos(ang)[:, None] * q[0] + np.sin(ang)[:, None] * q[1])

    atoms = []
    rings1 = []
    for _ in range(n_rings):
        rings1.append(np.arange(len(atoms), len(atoms) + 6, dtype=np.uint32))
        atoms.extend(ring(rng.uniform(0, extent, 3)))
    second = []
    for _ in range(n_second):
        if kind == "pipi":
            second.append(np.arange(len(atoms), len(atoms) + 6, dtype=np.uint32))
            atoms.extend(ring(rng.uniform(0, extent, 3)))
        else:
            second.append(len(atoms))
            atoms.append(rng.uniform(0, extent, 3))
    base = np.asarray(atoms)                                            # [N, 3]
    coords = (base[:, :, None] + 0.3 * rng.normal(size=(len(atoms), 3, F))).astype(np.float32)
    box = np.full((3, F), extent, np.float32)
    return coords, box, rings1, (second if kind == "pipi" else np.asarray(second, np.uint32))


def torch_composition(torch, kind, coords, box, rings1, second, thr):
    """-> number of reported pairs (the lists are built: nonzero, gathers of distance and angle)"""
    def records(rings):
        idx = torch.as_tensor(np.stack(rings).astype(np.int64), device=coords.device)       # [R, 6]
        xyz = coords[idx]                                                                    # [R, 6, 3, F]
        mean = xyz.mean(dim=1)
        n = torch.linalg.cross(xyz[:, 0] - xyz[:, 2], xyz[:, 1] - xyz[:, 2], dim=1)
        return mean, n / n.norm(dim=1, keepdim=True), xyz[:, 0]

    def wrapped_d2(a, b):                                               # [R1, 1, 3, F], [1, R2, 3, F]
        d = a - b
        d = torch.where((d.abs() > box / 2) & (box != 0), d - box * torch.round(d / box), d)
        return (d * d).sum(dim=2)

    def fold(dot):
        ang = torch.acos(dot.double()) * 57.29578
        return torch.where(ang > 90, 180 - ang, ang)

    m1, n1, f1 = records(rings1)
    if kind == "pipi":
        m2, n2, f2 = records(second)
        near = wrapped_d2(f1[:, None], f2[None]) <= 225
        d2 = wrapped_d2(m1[:, None], m2[None])
        ang = fold((n1[:, None] * n2[None]).sum(dim=2))
        hit = near & (((d2 < thr[0] ** 2) & (ang <= thr[1])) | ((d2 < thr[2] ** 2) & (ang >= thr[3])))
    else:
        pos = coords[torch.as_tensor(second.astype(np.int64), device=coords.device)]        # [C, 3, F]
        d2 = wrapped_d2(m1[:, None], pos[None])
        v = pos[None] - m1[:, None]
        v = v / v.norm(dim=2, keepdim=True)
        ang = 90 - fold((n1[:, None] * v).sum(dim=2))
        hit = (d2 <= thr[0] ** 2) & (ang >= thr[1])
    where = hit.permute(2, 0, 1).nonzero()                              # frame, r1, r2: the reference's order
    dist = d2.permute(2, 0, 1)[hit.permute(2, 0, 1)].sqrt()
    angle = ang.permute(2, 0, 1)[hit.permute(2, 0, 1)].float()
    return int(where.shape[0]), dist, angle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rings: no GPU visible (there is no CPU fallback)")
    from moleculekit_amd import interactions as I
    from moleculekit_amd import _lib

    shapes = [("pose_150x3_f1", "pipi", 150, 3, 1, 30.0, (4.4, 30.0, 5.5, 60.0)),
              ("protein_150x150_f2048", "pipi", 150, 150, 2048, 40.0, (4.4, 30.0, 5.5, 60.0)),
              ("cationpi_150x200_f2048", "cationpi", 150, 200, 2048, 40.0, (5.0, 60.0))]
    results = []
    for name, kind, n1, n2, F, extent, thr in shapes:
        coords, box, rings1, second = make_system(7, n1, n2, F, kind, extent)
        d_coords, d_box = torch.as_tensor(coords, device="cuda"), torch.as_tensor(box, device="cuda")
        atoms = np.concatenate(rings1 + (second if kind == "pipi" else []))
        s1 = (6 * np.arange(n1 + 1)).astype(np.uint32)
        sec = (6 * np.arange(n2 + 1) + 6 * n1).astype(np.uint32) if kind == "pipi" else second

        def fused():
            offs, pairs, da = I.ring_interactions_trajectory(kind, d_coords, d_box, atoms, s1, sec, thr)
            torch.cuda.synchronize()
            return int(offs[-1])

        def composed():
            n, _, _ = torch_composition(torch, kind, d_coords, d_box[None, None], rings1, second, thr)
            torch.cuda.synchronize()
            return n

        for _ in range(args.warmup):
            n_fused, n_comp = fused(), composed()
        t = {"fused": [], "torch": []}
        for _ in range(args.reps):                                     # alternating: both see the same neighbours on the machine
            for key, fn in (("fused", fused), ("torch", composed)):
                t0 = time.perf_counter()
                fn()
                t[key].append((time.perf_counter() - t0) * 1e3)
        med = {k: float(np.median(v)) for k, v in t.items()}
        row = dict(shape=name, kind=kind, rings=n1, partners=n2, frames=F, pair_tests=n1 * n2 * F, pairs_fused=n_fused, pairs_torch=n_comp,
                   fused_ms=med["fused"], fused_min_ms=min(t["fused"]), fused_max_ms=max(t["fused"]),
                   torch_ms=med["torch"], torch_min_ms=min(t["torch"]), torch_max_ms=max(t["torch"]),
                   torch_over_fused=med["torch"] / med["fused"], reps=args.reps, library=_lib.version() if hasattr(_lib, "version") else "")
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
