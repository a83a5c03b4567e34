"""tools/bench_sasa.py -- measurements of the surface-area row (moleculekit_amd/sasa.py, csrc/sasa_kernels.h).

Legs (one JSON line each):
  protein_F1 / protein_F64 / protein_F2048   the fixture protein (4 480 atoms, 960 points; frames 0 and 1 of tests/golden repeated
                                             with a small per-frame displacement) on a device-resident tensor
  system_30k                                 a 30 000-atom globule at protein density, 64 frames
  cpu_baseline                               the float32 numpy restatement (tests/sasa_restatement.py) on one protein frame, on
                                             this box: the only baseline there is -- the reference's mdtraj is not installed

Per GPU leg: ms per call (median of --reps, events around the call, after a warm-up call), frames/s, pair tests/s and the fraction
of the 157.3 TFLOP/s vector-FP32 peak.  The pair tests of a frame are COUNTED on the host for frame 0 and taken for every frame:
N (N - 1) neighbour tests of the scan (exact) plus the point-neighbour tests a lane makes up to and including the first neighbour
that buries its point, neighbours taken in atom order (the kernel's list order depends on the waves' timing, so this is an
estimate of what ran, not a count of it).  A test is 3 subtractions, 3 multiplies and 2 adds = 8 flop, none of them fused by
design (a fused multiply-add would change the counts), so half the peak is the ceiling.

    python tools/bench_sasa.py [--reps R] [--legs a,b,...]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_sasa.py` in a run of its own.
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

PEAK_TFLOPS = 157.3
FLOP_PER_TEST = 8


def _timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t)), float(min(t))


def _tests_per_frame(x_nm, r_nm, n_points, sample=400):
    """(scan tests, estimated point tests) of one frame; the point tests from a sample of atoms, scaled"""
    import sasa_restatement as R
    N = len(x_nm)
    pts = R.sphere_points(n_points)
    rng = np.random.default_rng(0)
    pick = rng.choice(N, min(sample, N), replace=False)
    total = 0
    for i in pick:
        d2 = R._d2(x_nm[i], x_nm)
        cut = r_nm[i] + r_nm
        nb = np.flatnonzero((d2 < cut * cut) & (np.arange(N) != i))
        if len(nb) == 0:
            continue
        p = x_nm[i] + r_nm[i] * pts
        buried = R._d2(p[:, None, :], x_nm[nb][None, :, :]) < (r_nm[nb] * r_nm[nb])[None, :]
        first = np.where(buried.any(1), buried.argmax(1) + 1, len(nb))
        total += int(first.sum())
    return N * (N - 1), int(total * (N / len(pick)))


def _gpu_leg(name, xyz_A, rad_A, n_points, reps, dev):
    import torch
    from moleculekit_amd import sasa
    t = torch.as_tensor(xyz_A, device=dev)
    ms, ms_min = _timed(lambda: sasa.sasa_trajectory(t, rad_A, n_points=n_points), reps)
    F, N = xyz_A.shape[:2]
    scan, point = _tests_per_frame(xyz_A[0] / np.float32(10), rad_A / np.float32(10), n_points)
    tests = (scan + point) * F
    rate = tests / (ms * 1e-3)
    return dict(leg=name, atoms=N, frames=F, n_points=n_points, ms=round(ms, 3), ms_min=round(ms_min, 3), frames_per_s=round(F / (ms * 1e-3), 1),
                scan_tests_per_frame=scan, point_tests_per_frame_est=point, pair_tests_per_s=float(f"{rate:.4g}"),
                fraction_of_vector_fp32_peak=round(rate * FLOP_PER_TEST / (PEAK_TFLOPS * 1e12), 4))


def _protein(F):
    import sasa_cases as C
    from moleculekit_amd._sasa_radii import ATOMIC_RADII
    mol, g = C.fixture()
    p = g["protein"]
    two = np.ascontiguousarray(np.transpose(mol.coords[p], (2, 0, 1)))
    rng = np.random.default_rng(F)
    xyz = np.resize(two, (F, 4480, 3)) + rng.uniform(-0.02, 0.02, size=(F, 1, 3)).astype(np.float32)
    rad = (np.array([ATOMIC_RADII[e] for e in g["element"][p]], np.float32) + np.float32(0.14)) * np.float32(10)
    return np.ascontiguousarray(xyz, np.float32), rad.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="protein_F1,protein_F64,protein_F2048,system_30k,cpu_baseline")
    a = ap.parse_args()
    legs = a.legs.split(",")
    import sasa_cases as C
    for leg in legs:
        if leg.startswith("protein_F"):
            xyz, rad = _protein(int(leg[len("protein_F"):]))
            print(json.dumps(_gpu_leg(leg, xyz, rad, 960, a.reps, "cuda:0")), flush=True)
        elif leg == "system_30k":
            x, r = C.globule(30000, seed=30, frames=64)
            print(json.dumps(_gpu_leg(leg, np.ascontiguousarray(x * np.float32(10)), (r * np.float32(10)).astype(np.float32), 960,
                                      max(1, a.reps // 2), "cuda:0")), flush=True)
        elif leg == "cpu_baseline":
            import sasa_restatement as R
            xyz, rad = _protein(1)
            t0 = time.perf_counter()
            R.areas(xyz / np.float32(10), rad / np.float32(10), 960)
            dt = time.perf_counter() - t0
            print(json.dumps(dict(leg=leg, what="the float32 numpy restatement, one thread, one protein frame (4 480 atoms, 960 points)",
                                  s_per_frame=round(dt, 2), frames_per_s=round(1.0 / dt, 4))), flush=True)
        else:
            raise SystemExit(f"unknown leg {leg}")


if __name__ == "__main__":
    main()
