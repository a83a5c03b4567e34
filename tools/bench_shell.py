"""tools/bench_shell.py -- measurements of the shell-count row (moleculekit_amd/shell.py, csrc/shell_kernels.h).

Per shape (one JSON line each), on device-resident tensors, three rounds with the routes ALTERNATING inside a round:
  fused_ms    (a) shell_counts_trajectory: the fused kernels, no distance matrix
  matrix_ms   (b) what the library offered before: mkamd_dist_trajectory_dev into a [F, n1 * n2] float32 tensor, then torch comparisons
              and sums on the device (one `d <= edge` pass per edge, differenced); "n/a" where the matrix does not fit --route-b-gib
  numpy_s     (c) the numpy restatement of the reference's histogram (tests/shell_restatement.py) on distances of the same library's
              host call -- only for shapes of at most --numpy-pairs pairs
and from (a): pairs per second and the share of the vector-FP32 peak, counting the instructions the kernels issue per pair (8 for
d2 -- three subtractions, three multiplies, two adds, none fused --, 27 more where the pair takes the image shift, and 2 per edge in
the frame-lane kernel / 1 in the atom-lane kernel): instructions x 64 lanes against 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz.
Every leg asserts that (a) and (b) give the same counts before it times anything.

    python tools/bench_shell.py [--reps R] [--rounds 3] [--shapes a,b,...]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_shell.py` in a run of its own.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9          # vector instructions x lanes per second, whole chip
SHAPES = {                                     # name: (n1, n2, F, periodic, symmetric)
    "ca_ligand_200": (277, 9, 200, True, False),
    "ca_water_2048": (277, 10000, 2048, True, False),
    "self_300_2048": (300, 300, 2048, False, True),
    "one_centre_20000": (1, 20000, 1, True, False),
    "self_3000_one_frame": (3000, 3000, 1, False, True),
}


def _timed(fn, reps):
    import torch
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t))


def _case(n1, n2, F, symmetric, seed):
    rng = np.random.default_rng(seed)
    n = n1 if symmetric else n1 + n2
    box_len = max(30.0, (n2 / 0.0334) ** (1.0 / 3.0))          # water's number density, at least 30 Angstrom
    coords = rng.uniform(0, box_len, size=(n, 3, F)).astype(np.float32)
    box = np.full((3, F), box_len, np.float32)
    sel1 = np.arange(n1, dtype=np.uint32)
    sel2 = sel1 if symmetric else np.arange(n1, n1 + n2, dtype=np.uint32)
    chains = np.ones(n, np.uint32)
    chains[sel2] = 2
    return coords, box, sel1, sel2, chains


def run_shape(name, reps, rounds, route_b_gib, numpy_pairs):
    import torch
    from moleculekit_amd import _lib, shell
    n1, n2, F, periodic, symmetric = SHAPES[name]
    coords, box, sel1, sel2, chains = _case(n1, n2, F, symmetric, seed=len(name))
    edges = np.arange(0, 15, 3)
    dev = torch.device("cuda", 0)
    ctx = _lib.default_context(0)
    dc, db = torch.as_tensor(coords, device=dev), torch.as_tensor(box, device=dev)
    d1, d2, dch = (torch.as_tensor(a.view(np.int32), device=dev) for a in (sel1, sel2, chains))
    out = torch.empty((F, n1, 4), dtype=torch.int32, device=dev)
    pairs = n1 * n2 * F

    def fused():
        shell.shell_counts_trajectory(dc, db, sel1, sel2, chains, edges, symmetric=symmetric, pbc=periodic, out=out, ctx=ctx)

    matrix_fits = pairs * 4 / 2 ** 30 <= route_b_gib
    dist = torch.empty((F, n1 * n2), dtype=torch.float32, device=dev) if matrix_fits else None
    t_edges = torch.as_tensor(edges.astype(np.float32), device=dev)

    def matrix():
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        ctx.dist_trajectory_dev(dc, F, db, d1, n1, d2, n2, dch, False, periodic, False, dist)
        d = dist.view(F, n1, n2)
        running = torch.stack([(d <= t_edges[e]).sum(dim=2, dtype=torch.int32) for e in range(5)], dim=2)
        return running[:, :, 1:] - running[:, :, :-1]

    fused()
    torch.cuda.synchronize()
    kernel = ctx.last_dist_kernel()
    if matrix_fits:
        assert torch.equal(matrix(), out), f"{name}: the fused counts are not the matrix route's"
    rows = []
    for _ in range(rounds):
        a = _timed(fused, reps)
        b = _timed(matrix, reps) if matrix_fits else None
        rows.append((a, b))
    fused_ms = float(np.median([r[0] for r in rows]))
    matrix_ms = float(np.median([r[1] for r in rows])) if matrix_fits else None
    per_pair = 8 + (27 if periodic and not symmetric else 0) + (5 if "atoms" in kernel else 10)
    rate = pairs / (fused_ms * 1e-3)
    res = dict(shape=name, n1=n1, n2=n2, frames=F, periodic=periodic, symmetric=symmetric, kernel=kernel,
               build=_lib.load().mkamd_version().decode(), rounds=[[round(a, 4), None if b is None else round(b, 4)] for a, b in rows],
               fused_ms=round(fused_ms, 4), matrix_ms="n/a" if matrix_ms is None else round(matrix_ms, 4),
               ratio_matrix_over_fused="n/a" if matrix_ms is None else round(matrix_ms / fused_ms, 2),
               pairs_per_s=float(f"{rate:.4g}"), instructions_per_pair=per_pair,
               share_of_valu_peak=round(rate * per_pair / LANE_OPS_PER_S, 4))
    if pairs <= numpy_pairs:
        import shell_restatement as R
        t0 = time.perf_counter()
        R.counts(R.gpu_dist, coords, box, sel1, sel2, chains, edges, symmetric=symmetric, pbc=periodic)
        res["numpy_s"] = round(time.perf_counter() - t0, 3)
    del dist
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--route-b-gib", type=float, default=64.0, help="largest distance matrix route (b) may allocate")
    ap.add_argument("--numpy-pairs", type=float, default=2e7)
    a = ap.parse_args()
    for name in a.shapes.split(","):
        if name not in SHAPES:
            raise SystemExit(f"unknown shape {name}")
        print(json.dumps(run_shape(name, a.reps, a.rounds, a.route_b_gib, a.numpy_pairs)), flush=True)


if __name__ == "__main__":
    main()
