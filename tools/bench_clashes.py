"""tools/bench_clashes.py -- time the steric-clash device call beside two yardsticks that exist without it: the package's all-pairs
contact list at the same cut-off on the same device, and the numpy restatement of the reference's search on the host; and sweep the
two launch plans of the pair kernels over the number of owners, which is what the plan's crossover is read from.

    python tools/bench_clashes.py [--reps 10] [--warmup 2] [--out results.json] [--only NAME] [--no-host] [--no-sweep]

Shapes: 3PTB against itself (1 639 atoms, tests/golden/channels_3ptb.npz, its file bonds as exclusions); a 40-atom ligand against a
20 000-atom receptor (carbons on a jittered 1.9 A lattice, the ligand a random walk through its middle); 100 000 and 1 000 000 atoms at
water density against themselves (waters on a jittered lattice, 3.1 A apart, their O-H bonds as exclusions).
The sweep: 300 000 atoms at water density, the owners a random subset of 32 .. 262 144 of them against all, each timed with a thread
per owner and with a wave per owner.

The contact list (every pair i < j within the clash cutoff, non-periodic) tests N (N - 1) / 2 pairs: it is timed where that is below
2^32, the most one contact-list call takes.  It is NOT the same list (no radii, no exclusions): it is the yardstick for what an
all-pairs search costs on the same device.  The restatement (tests/clashes_restatement.py) is numpy over all pairs in chunks: timed
once, on the shapes of at most 20 040 atoms, unless --no-host.  Nothing is compared against the code under test but the NUMBER of rows,
which is printed beside the restatement's.

Device calls are timed with a host clock around work that ends in a device synchronise, alternating, after a warm-up of every shape; the
median and the spread (min .. max) of ``--reps`` repetitions are reported, one JSON line per shape.  The exclusion table is built
before the clock starts: it belongs to the topology, not to the frame.  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NO_BONDS = np.zeros((0, 2), np.uint32)


def ptb():
    d = np.load(os.path.join(ROOT, "tests", "golden", "channels_3ptb.npz"))
    return d["coords"].astype(np.float32), d["element"], d["bonds"].astype(np.uint32), None, None


def ligand_receptor(n_receptor=20000, n_ligand=40, seed=5):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n_receptor ** (1.0 / 3.0)))
    idx = np.arange(n_receptor)
    receptor = np.stack([idx % side, idx // side % side, idx // (side * side)], axis=1) * 1.9 + rng.uniform(-0.3, 0.3, size=(n_receptor, 3))
    steps = rng.normal(size=(n_ligand, 3))
    ligand = receptor.mean(axis=0) + np.cumsum(steps / np.linalg.norm(steps, axis=1, keepdims=True) * 1.5, axis=0)
    coords = np.concatenate([receptor, ligand]).astype(np.float32)
    n = len(coords)
    sel1, sel2 = np.zeros(n, bool), np.zeros(n, bool)
    sel1[n_receptor:], sel2[:n_receptor] = True, True
    return coords, np.array(["C"] * n), np.stack([np.arange(n_receptor, n - 1), np.arange(n_receptor + 1, n)], axis=1).astype(np.uint32), sel1, sel2


def waters(n_atoms, seed=3):
    rng = np.random.default_rng(seed)
    n = -(-n_atoms // 3)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    idx = np.arange(n)
    centres = np.stack([idx % side, idx // side % side, idx // (side * side)], axis=1) * 3.1 + rng.uniform(-0.3, 0.3, size=(n, 3))
    a, b = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b -= a * (a * b).sum(axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    half = np.deg2rad(104.5) / 2.0
    coords = np.stack([centres, centres + 0.9572 * (np.cos(half) * a + np.sin(half) * b), centres + 0.9572 * (np.cos(half) * a - np.sin(half) * b)],
                      axis=1).reshape(-1, 3)[:n_atoms]
    element = np.where(np.arange(n_atoms) % 3 == 0, "O", "H")
    o = np.arange(0, n_atoms - 2, 3)
    bonds = np.concatenate([np.stack([o, o + 1], axis=1), np.stack([o, o + 2], axis=1)]).astype(np.uint32)
    return coords.astype(np.float32), element, bonds, None, None


def timed(fns, warmup, reps):
    counts = {}
    for _ in range(warmup):
        for key, fn in fns:
            counts[key] = fn()
    t = {k: [] for k, _ in fns}
    for _ in range(reps):                                              # alternating: all see the same neighbours on the machine
        for key, fn in fns:
            t0 = time.perf_counter()
            fn()
            t[key].append((time.perf_counter() - t0) * 1e3)
    return counts, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one shape by name")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement on the host")
    ap.add_argument("--no-sweep", action="store_true", help="skip the plan sweep over the owner count")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_clashes: no GPU visible (there is no CPU fallback)")
    from moleculekit_amd import _lib
    from moleculekit_amd import clashes as CL

    overlap = 0.6
    shapes = [("3ptb_self", ptb), ("ligand40_receptor20k", ligand_receptor), ("water_100k", lambda: waters(100000)), ("water_1m", lambda: waters(1000000))]
    results = []
    ctx = _lib.default_context(0)
    for name, make in shapes:
        if args.only and args.only != name:
            continue
        coords, element, bonds, sel1, sel2 = make()
        N = len(coords)
        radii = CL.clash_radii(element)
        cutoff = CL.clash_cutoff(radii.max(), overlap)
        ex = CL.clash_exclusions(bonds, N)
        d_coords, d_radii = torch.as_tensor(coords, device="cuda"), torch.as_tensor(radii, device="cuda")
        d_sel1 = torch.as_tensor(np.ones(N, bool) if sel1 is None else sel1, device="cuda")
        d_sel2 = None if sel2 is None else torch.as_tensor(sel2, device="cuda")
        d_frame = d_coords.reshape(N, 3, 1).contiguous()                # the contact list's [N, 3, F] layout
        d_all = torch.arange(N, dtype=torch.int32, device="cuda")
        d_chains = torch.zeros(N, dtype=torch.int32, device="cuda")
        d_box = torch.zeros((3, 1), dtype=torch.float32, device="cuda")   # (not read without pbc; the entry point wants one)
        all_pairs = N * (N - 1) // 2
        noted = {}

        def clashes():
            pairs, _, _ = CL.find_clashes_tensor(d_coords, d_radii, d_sel1, d_sel2, overlap, ex, float(radii.max()), ctx=ctx)
            torch.cuda.synchronize()
            noted["pair_kernel"] = ctx.last_dist_kernel()
            return int(pairs.shape[0])

        def contacts():
            offs, _, _ = ctx.contacts_trajectory_dev(d_frame, 1, d_box, d_all, N, d_all, N, d_chains, True, False, cutoff)
            ctx.synchronize()
            return int(offs[-1])

        fns = [("clashes", clashes)] + ([("contacts", contacts)] if all_pairs < 2 ** 32 else [])
        counts, t = timed(fns, args.warmup, args.reps)
        med = {k: float(np.median(v)) for k, v in t.items()}
        row = dict(shape=name, atoms=N, owners=int(N if sel1 is None else sel1.sum()), cutoff=cutoff, rows=counts["clashes"], clashes_ms=med["clashes"],
                   clashes_min_ms=min(t["clashes"]), clashes_max_ms=max(t["clashes"]), pair_kernel=noted["pair_kernel"], reps=args.reps)
        if "contacts" in med:
            row.update(all_pairs=all_pairs, contacts=counts["contacts"], contacts_ms=med["contacts"], contacts_min_ms=min(t["contacts"]),
                       contacts_max_ms=max(t["contacts"]), contacts_over_clashes=med["contacts"] / med["clashes"])
        if not args.no_host and N <= 20040:
            import clashes_restatement as R
            t0 = time.perf_counter()
            host = R.find_clashes(coords, radii, bonds, sel1, sel2, overlap)
            row.update(restatement_ms=(time.perf_counter() - t0) * 1e3, restatement_rows=int(len(host[0])))
        print(json.dumps(row), flush=True)
        results.append(row)

    if not args.no_sweep and not args.only:
        coords, element, bonds, _, _ = waters(300000)
        N = len(coords)
        radii = CL.clash_radii(element)
        ex = CL.clash_exclusions(bonds, N)
        d_coords, d_radii = torch.as_tensor(coords, device="cuda"), torch.as_tensor(radii, device="cuda")
        d_all = torch.ones(N, dtype=torch.bool, device="cuda")
        perm = np.random.default_rng(7).permutation(N)
        for owners in (32, 128, 512, 2048, 8192, 16384, 32768, 65536, 131072, 262144):
            d_sel1 = torch.as_tensor(np.sort(perm[:owners]), device="cuda")
            noted = {}

            def run(avoid, key):
                def fn():
                    ctx.set_clash_plan(avoid)
                    try:
                        pairs, _, _ = CL.find_clashes_tensor(d_coords, d_radii, d_sel1, d_all, overlap, ex, float(radii.max()), ctx=ctx)
                        torch.cuda.synchronize()
                        noted[key] = ctx.last_dist_kernel()
                    finally:
                        ctx.set_clash_plan(0)
                    return int(pairs.shape[0])
                return fn

            counts, t = timed([("thread", run(CL.AVOID_WAVE, "thread")), ("wave", run(CL.AVOID_THREAD, "wave"))], args.warmup, args.reps)
            assert counts["thread"] == counts["wave"] and noted == {"thread": CL.THREAD_KERNEL, "wave": CL.WAVE_KERNEL}
            row = dict(shape="sweep_water_300k", atoms=N, owners=owners, rows=counts["wave"], reps=args.reps)
            for k in ("thread", "wave"):
                row.update({f"{k}_ms": float(np.median(t[k])), f"{k}_min_ms": min(t[k]), f"{k}_max_ms": max(t[k])})
            print(json.dumps(row), flush=True)
            results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
