"""tools/bench_align.py -- measurements of the alignment row (moleculekit_amd/align.py, csrc/align_kernels.h).

Legs (one JSON line each):
  apply_30k       kabsch_transforms + apply_transforms on a device-resident 30 000 atoms x 2 048 frames (737 MB), 3 000-atom
                  selection; apply's rate as a fraction of 8 TB/s (it moves 2 x 737 MB)
  transforms      kabsch_transforms alone: us per 1 000 frames for 23- and 3 000-atom selections, and one frame of 100 000 atoms
  metricrmsd      the MetricRmsd shape (4 507 atoms, 200 frames, 301 selected) end to end from host arrays
  xtc_stream      iterVoxelizeXTC on a 30 000-atom trajectory with and without align=, alternated in one process
  cpu_baseline    the float64 numpy per-frame loop (SVD Kabsch + transform) for the apply_30k and metricrmsd shapes

    python tools/bench_align.py [--reps R] [--legs a,b,...]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_align.py` in a run of its own.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def _traj(rng, N, F, base=64):
    ref = (rng.normal(size=(N, 3)) * 20).astype(np.float32)
    one = np.stack([(ref @ _rot(rng).T + rng.uniform(-50, 50, 3) + rng.normal(scale=0.5, size=(N, 3))).astype(np.float32)
                    for _ in range(min(base, F))])
    return np.ascontiguousarray(np.resize(one, (F, N, 3))), ref


def _timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best.append(a.elapsed_time(b))
    return float(np.median(best)), float(min(best))


def leg_apply(dev, reps):
    import torch
    from moleculekit_amd import align
    rng = np.random.default_rng(1)
    N, F, n = 30000, 2048, 3000
    xyz, ref = _traj(rng, N, F)
    sel = np.sort(rng.choice(N, n, replace=False))
    d_xyz, d_ref = torch.as_tensor(xyz, device=dev), torch.as_tensor(ref, device=dev)
    out = torch.empty_like(d_xyz)
    aff, _ = align.kabsch_transforms(d_xyz, d_ref, sel)
    t_tr, _ = _timed(lambda: align.kabsch_transforms(d_xyz, d_ref, sel), reps)
    t_ap, t_ap_min = _timed(lambda: align.apply_transforms(d_xyz, aff, out=out), reps)
    bytes_moved = 2 * d_xyz.numel() * 4
    return dict(leg="apply_30k", atoms=N, frames=F, sel=n, MB=round(d_xyz.numel() * 4 / 1e6), transforms_ms=round(t_tr, 3),
                apply_ms=round(t_ap, 3), apply_TBs=round(bytes_moved / (t_ap * 1e-3) / 1e12, 3),
                apply_fraction_of_8TBs=round(bytes_moved / (t_ap * 1e-3) / 1e12 / HBM_TBS, 3), total_ms=round(t_tr + t_ap, 3))


def leg_transforms(dev, reps):
    import torch
    from moleculekit_amd import align
    rng = np.random.default_rng(2)
    res = dict(leg="transforms")
    for N, F, n in ((3000, 1000, 23), (30000, 1000, 3000)):
        xyz, ref = _traj(rng, N, F)
        sel = np.arange(n)
        d_xyz, d_ref = torch.as_tensor(xyz, device=dev), torch.as_tensor(ref, device=dev)
        t, _ = _timed(lambda: align.kabsch_transforms(d_xyz, d_ref, sel), reps)
        res[f"us_per_1000_frames_sel{n}"] = round(t * 1e3, 1)
    xyz, ref = _traj(rng, 100000, 1)
    d_xyz, d_ref = torch.as_tensor(xyz, device=dev), torch.as_tensor(ref, device=dev)
    t, _ = _timed(lambda: align.kabsch_transforms(d_xyz, d_ref, np.arange(100000)), reps)
    res["us_one_frame_100k_atoms"] = round(t * 1e3, 1)
    return res


def leg_metricrmsd(dev, reps):
    import torch
    from moleculekit_amd import align
    rng = np.random.default_rng(3)
    N, F = 4507, 200
    coords = np.ascontiguousarray(_traj(rng, N, F)[0].transpose(1, 2, 0))           # host [N, 3, F], Molecule.coords
    ca = np.sort(rng.choice(N, 301, replace=False))

    def run():
        x = torch.as_tensor(np.ascontiguousarray(coords.transpose(2, 0, 1)), device=dev)
        return align.rmsd_trajectory(x, x[0], ca, ca).cpu().numpy()

    run()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
    t_host = []
    for _ in range(max(1, reps // 4)):
        c = coords.copy()
        t0 = time.perf_counter()
        align._pp_align(c, c, ca, ca, np.arange(F), 0, False, inplace=True)
        t_host.append(time.perf_counter() - t0)
    return dict(leg="metricrmsd", atoms=N, frames=F, sel=301, end_to_end_ms=round(1e3 * float(np.median(ts)), 3),
                pp_align_host_ms=round(1e3 * float(np.median(t_host)), 3))


def leg_xtc(dev, reps):
    import torch
    from moleculekit_amd import batch, xtc
    rng = np.random.default_rng(4)
    N, base, F = 30000, 64, 2048
    # frames close to the reference (rotations of a few degrees, shifts of an Angstrom): the aligned and the plain stream
    # voxelize the same atoms, so the difference is the alignment's cost (large random motions would move atoms out of the grid)
    ref = (rng.normal(size=(N, 3)) * 20).astype(np.float32)
    xyz = np.empty((base, N, 3), np.float32)
    for f in range(base):
        w = rng.normal(scale=0.03, size=3)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        q, r = np.linalg.qr(np.eye(3) + K)
        R = q * np.sign(np.diag(r))
        xyz[f] = ref @ R.T + rng.uniform(-1, 1, 3) + rng.normal(scale=0.5, size=(N, 3))
    nm = np.ascontiguousarray((xyz * np.float32(0.1)).transpose(1, 2, 0))
    sig = rng.uniform(1.0, 2.0, size=(N, 8)).astype(np.float32)
    sel = np.arange(0, N, 10)
    center = ref[sel].astype(np.float64).mean(0)
    res = dict(leg="xtc_stream", atoms=N, frames=F, sel=len(sel))
    with tempfile.TemporaryDirectory() as d:
        one = os.path.join(d, "one.xtc")
        xtc.write_xtc(one, nm, np.zeros((3, 3, base), np.float32), np.zeros(base, np.float32), np.arange(base))
        blob = open(one, "rb").read()
        fn = os.path.join(d, "big.xtc")
        with open(fn, "wb") as fh:
            for _ in range(F // base):
                fh.write(blob)

        def run(al):
            t0 = time.perf_counter()
            n = 0
            for _, f in batch.iterVoxelizeXTC(fn, sig, center, [24, 24, 24], 1.0, pbc=False, chunk=1024, align=al):
                n += f.shape[0]
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        run(None)
        run((ref[sel], sel))
        plain, aligned = [], []
        for _ in range(reps):
            plain.append(run(None))
            aligned.append(run((ref[sel], sel)))
    p, a = float(np.median(plain)), float(np.median(aligned))
    res.update(plain_ms=round(1e3 * p, 2), aligned_ms=round(1e3 * a, 2), overhead=round(a / p - 1.0, 4),
               plain_frames_per_s=round(F / p), aligned_frames_per_s=round(F / a))
    return res


def _kabsch_np(P, Q):
    cP, cQ = P.mean(0), Q.mean(0)
    V, S, Wt = np.linalg.svd((P - cP).T @ (Q - cQ))
    Z = np.eye(3)
    Z[2, 2] = np.sign(np.linalg.det(Wt.T) * np.linalg.det(V))
    R = Wt.T @ Z @ V.T
    return R, cQ - R @ cP


def leg_cpu(reps):
    rng = np.random.default_rng(5)
    res = dict(leg="cpu_baseline")
    for name, N, F, n in (("apply_30k_per_1000_frames", 30000, 64, 3000), ("metricrmsd", 4507, 200, 301)):
        xyz, ref = _traj(rng, N, F)
        sel = np.arange(n)
        t0 = time.perf_counter()
        for f in range(F):
            R, t = _kabsch_np(xyz[f][sel].astype(np.float64), ref[sel].astype(np.float64))
            _ = (xyz[f].astype(np.float64) @ R.T + t).astype(np.float32)
        dt = time.perf_counter() - t0
        res[name + "_ms"] = round(1e3 * dt * (1000 / F if name.startswith("apply") else 1.0), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--legs", default="apply_30k,transforms,metricrmsd,xtc_stream,cpu_baseline")
    args = ap.parse_args()
    import torch
    from moleculekit_amd import _lib
    dev = torch.device("cuda", _lib.default_context().device)
    legs = args.legs.split(",")
    for leg, fn in (("apply_30k", leg_apply), ("transforms", leg_transforms), ("metricrmsd", leg_metricrmsd), ("xtc_stream", leg_xtc)):
        if leg in legs:
            print(json.dumps(fn(dev, args.reps)), flush=True)
    if "cpu_baseline" in legs:
        print(json.dumps(leg_cpu(args.reps)), flush=True)


if __name__ == "__main__":
    main()
