"""tools/bench_hbonds.py -- time the fused hydrogen-bond call beside a torch composition of the same test and beside the contact-list
call at the same number of pair tests, on the same device.

    python tools/bench_hbonds.py [--reps 10] [--warmup 2] [--out results.json] [--only NAME]

Shapes: a ligand pose against a protein (5 + 1 000 donor rows, 8 + 1 000 acceptors, 1 frame, the two molecules as the two selections);
a protein's own bonds (1 000 x 1 000, ``sel2=None``, 2 048 frames); a water bridge's first shell (25 donor rows and 25 acceptors of a
selection against 10 000 waters -- 20 000 donor rows, 10 000 acceptors --, 256 frames).  The pair tests of a shape are its ALLOWED pairs
times its frames.

The composition does what a torch user would write: gather the atoms, minimum image of both vectors, the distance test, ``acos`` of the
clamped ratio, the angle test and ``nonzero`` -- over as many frames at a time as keep a temporary under 256 MB.  It is NOT bit-faithful
to the reference (torch's float32 acos, fused multiply-adds at the compiler's pleasure): it is the yardstick for time only; the number
of bonds it reports is printed beside the fused call's.  The contact-list call (hydrogens x acceptors within the distance threshold,
periodic) is the per-pair cost yardstick: the same number of pair tests, no angle.

All are timed with a host clock around work that ends in a device synchronise, alternating, after a warm-up of every shape; the median
and the spread (min .. max) of ``--reps`` repetitions are reported, one JSON line per shape.  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_system(seed, groups, F, extent):
    """`groups`: (donor rows, acceptors, hydrogens per heavy atom) per molecule class -> coords [N, 3, F], box, and per class the donor
    rows [n, 2] and acceptors [m].  Heavy atoms sit at random in a periodic cube, hydrogens 1 A from them; acceptors at random."""
    rng = np.random.default_rng(seed)
    base, out = [], []
    for nd, na, per in groups:
        donors = []
        for r in range(nd):
            if r % per == 0:
                heavy = len(base)
                base.append(rng.uniform(0, extent, 3))
            v = rng.normal(size=3)
            donors.append((heavy, len(base)))
            base.append(base[heavy] + v / np.linalg.norm(v))
        acc = []
        for _ in range(na):
            acc.append(len(base))
            base.append(rng.uniform(0, extent, 3))
        out.append((np.asarray(donors, np.uint32).reshape(-1, 2), np.asarray(acc, np.uint32)))
    base = np.asarray(base, np.float32)
    coords = np.empty((len(base), 3, F), np.float32)
    for f0 in range(0, F, 64):                                          # (in slabs: a float64 normal of the whole array is gigabytes)
        n = min(64, F - f0)
        coords[:, :, f0:f0 + n] = base[:, :, None] + (0.3 * rng.standard_normal((len(base), 3, n), dtype=np.float32))
    return coords, np.full((3, F), extent, np.float32), out


def torch_composition(torch, coords, box, blocks, thr_d, thr_ang_deg, budget=256 << 20):
    """blocks: (donor rows [n, 2], acceptors [m]) -- every row against every acceptor of its block -> number of bonds reported"""
    F = coords.shape[2]
    total = 0
    thr2, thr_ang = thr_d * thr_d, thr_ang_deg / 57.29578

    def wrap(d, bx):
        return torch.where((d.abs() > bx / 2) & (bx != 0), d - bx * torch.round(d / bx), d)

    for donors, acceptors in blocks:
        if len(donors) == 0 or len(acceptors) == 0:
            continue
        dh = torch.as_tensor(donors.astype(np.int64), device=coords.device)
        ac = torch.as_tensor(acceptors.astype(np.int64), device=coords.device)
        step = max(1, min(F, budget // (len(donors) * len(acceptors) * 12)))
        for f0 in range(0, F, step):
            c, bx = coords[:, :, f0:f0 + step], box[:, f0:f0 + step]
            heavy, hyd, pa = c[dh[:, 0]], c[dh[:, 1]], c[ac]             # [n, 3, f], [n, 3, f], [m, 3, f]
            va = wrap(pa[None] - hyd[:, None], bx)                       # [n, m, 3, f]
            vb = wrap(heavy - hyd, bx)                                   # [n, 3, f]
            d2a, d2b = (va * va).sum(dim=2), (vb * vb).sum(dim=1)
            ratio = ((va * vb[:, None]).sum(dim=2) / (d2a.sqrt() * d2b.sqrt()[:, None])).clamp(-1, 1)
            hit = (d2a <= thr2) & (d2a != 0) & (d2b != 0)[:, None] & (torch.acos(ratio) > thr_ang) & (dh[:, 0, None] != ac[None])[:, :, None]
            where = hit.permute(2, 0, 1).nonzero()                      # frame, donor row, acceptor: the reference's order
            triples = torch.stack([dh[where[:, 1], 0], dh[where[:, 1], 1], ac[where[:, 2]]], dim=1)
            total += int(triples.shape[0])
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one shape by name")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition (a profiler run of the library's kernels)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_hbonds: no GPU visible (there is no CPU fallback)")
    from moleculekit_amd import _lib
    from moleculekit_amd import hbonds as H

    # name, molecule classes (donor rows, acceptors, hydrogens per heavy atom), frames, extent, intra
    shapes = [("pose_ligand_protein_f1", [(1000, 1000, 1), (5, 8, 1)], 1, 40.0, False),
              ("protein_intra_1000x1000_f2048", [(1000, 1000, 1)], 2048, 40.0, True),
              ("waterbridge_50_x_10000_waters_f256", [(25, 25, 1), (20000, 10000, 2)], 256, 67.0, False)]
    results = []
    ctx = _lib.default_context(0)
    for name, groups, F, extent, intra in shapes:
        if args.only and args.only != name:
            continue
        coords, box, mols = make_system(7, groups, F, extent)
        N = coords.shape[0]
        donors = np.concatenate([m[0] for m in mols])
        acceptors = np.concatenate([m[1] for m in mols])
        sel1 = np.zeros(N, np.uint32)
        sel1[np.concatenate([mols[0][0].ravel(), mols[0][1]])] = 1
        sel2 = None
        if intra:
            blocks = [(mols[0][0], mols[0][1])]
        else:
            sel2 = np.zeros(N, np.uint32)
            sel2[np.concatenate([mols[1][0].ravel(), mols[1][1]])] = 1
            blocks = [(mols[0][0], mols[1][1]), (mols[1][0], mols[0][1])]  # donors of one selection against acceptors of the other
        tests = sum(len(d) * len(a) for d, a in blocks) * F
        d_coords, d_box = torch.as_tensor(coords, device="cuda"), torch.as_tensor(box, device="cuda")
        chains = np.zeros(N, np.uint32)
        chains[acceptors] = 1                                           # hydrogens and acceptors in different chains: every pair is wrapped
        d_chains = torch.as_tensor(chains.view(np.int32), device="cuda")
        d_blocks = [(torch.as_tensor(np.ascontiguousarray(d[:, 1]).view(np.int32), device="cuda"), len(d),
                     torch.as_tensor(a.view(np.int32), device="cuda"), len(a)) for d, a in blocks]

        def fused():
            offs, triples = H.hbonds_trajectory(d_coords, d_box, donors, acceptors, sel1, sel2, ctx=ctx)
            torch.cuda.synchronize()
            return int(offs[-1])

        def composed():
            n = torch_composition(torch, d_coords, d_box, blocks, 2.5, 120.0)
            torch.cuda.synchronize()
            return n

        def contacts():
            n = 0
            for h, nh, a, na in d_blocks:
                offs, _, _ = ctx.contacts_trajectory_dev(d_coords, F, d_box, h, nh, a, na, d_chains, False, True, 2.5)
                n += int(offs[-1])
            ctx.synchronize()
            return n

        fns = [("fused", fused), ("contacts", contacts)] + ([] if args.no_torch else [("torch", composed)])
        counts = {}
        for _ in range(args.warmup):
            for key, fn in fns:
                counts[key] = fn()
        t = {k: [] for k, _ in fns}
        for _ in range(args.reps):                                     # alternating: all see the same neighbours on the machine
            for key, fn in fns:
                t0 = time.perf_counter()
                fn()
                t[key].append((time.perf_counter() - t0) * 1e3)
        med = {k: float(np.median(v)) for k, v in t.items()}
        row = dict(shape=name, donor_rows=len(donors), acceptors=len(acceptors), frames=F, pair_tests=tests, bonds_fused=counts["fused"],
                   bonds_torch=counts.get("torch"), contacts=counts["contacts"],
                   fused_ms=med["fused"], fused_min_ms=min(t["fused"]), fused_max_ms=max(t["fused"]),
                   contacts_ms=med["contacts"], contacts_min_ms=min(t["contacts"]), contacts_max_ms=max(t["contacts"]),
                   fused_ns_per_test=med["fused"] * 1e6 / tests, contacts_ns_per_test=med["contacts"] * 1e6 / tests,
                   fused_over_contacts=med["fused"] / med["contacts"], reps=args.reps)
        if not args.no_torch:
            row.update(torch_ms=med["torch"], torch_min_ms=min(t["torch"]), torch_max_ms=max(t["torch"]), torch_over_fused=med["torch"] / med["fused"])
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
