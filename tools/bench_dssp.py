#!/usr/bin/env python3
"""Secondary structure: the device call (moleculekit_amd.dssp.dssp_trajectory, resident tensors) under each energy plan, against the
numpy restatement of the same rules on the host (tests/dssp_restatement.py, timed on a few frames and scaled to the call's frames).

Workloads: (a) the 3PTB backbone (223 residues), 1 frame; (b) the same over 2 048 frames of seeded noise; (c) a 1 000-residue
synthetic chain (helices and strands from ideal geometry) over 2 048 noisy frames.  Per workload and plan: the median time of the
call (events around it, warm-up calls first, three rounds with the plans alternating, the median round) and the frames per second.
Then both systems over 1 ... 256 frames under both plans: the frame count at which they cross.  The device's codes are
asserted equal to the restatement's on the timed frames of the restatement before anything is timed.

    python tools/bench_dssp.py [--json] [--only abc] [--no-sweep]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PLANS = (("frames", 2), ("acceptors", 1))           # name, Context.set_dssp_plan mask that forces it


def synthetic_chain(n_res, frames, seed):
    import dssp_cases as C
    rng = np.random.default_rng(seed)
    torsions = []
    while len(torsions) < n_res:
        kind = (C.ALPHA, C.BETA_ANTI, C.H310, (-70.0, 150.0))[rng.integers(0, 4)]
        torsions += [kind] * int(rng.integers(4, 16))
    return C.case_from_residues(C.chain_from_torsions(torsions[:n_res]), frames=frames, noise=0.3, seed=seed)


def timed(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def both_plans(ctx, coords, rest, calls, warmup):
    """median-round time in ms of each plan, the plans alternating"""
    from moleculekit_amd.dssp import dssp_trajectory
    rounds = {name: [] for name, _ in PLANS}
    for _ in range(3):
        for name, mask in PLANS:
            ctx.set_dssp_plan(mask)
            try:
                rounds[name].append(timed(lambda: dssp_trajectory(coords, *rest, simplified=False, ctx=ctx), calls, warmup))
            finally:
                ctx.set_dssp_plan(0)
    return {name: sorted(ts)[1] for name, ts in rounds.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--only", default="abc")
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    import torch
    import dssp_cases as C
    import dssp_restatement as R
    from moleculekit_amd import _lib
    from moleculekit_amd.dssp import dssp_trajectory
    ctx = _lib.default_context()
    workloads = {"a": ("3PTB backbone x 1", lambda: C.noisy_3ptb(1), 4, 20), "b": ("3PTB backbone x 2 048", lambda: C.noisy_3ptb(2048), 4, 10),
                 "c": ("1 000-residue chain x 2 048", lambda: synthetic_chain(1000, 2048, 23), 1, 3)}
    rows = []
    for key in args.only:
        label, make, host_frames, calls = workloads[key]
        coords, *rest = make()
        F = coords.shape[2]
        hf = min(host_frames, F)
        t0 = time.perf_counter()
        want = R.dssp(coords[:, :, :hf], *rest)[2]
        host_ms_per_frame = (time.perf_counter() - t0) * 1e3 / hf
        d = torch.as_tensor(coords).cuda()
        for name, mask in PLANS:
            ctx.set_dssp_plan(mask)
            try:
                got = dssp_trajectory(d, *rest, simplified=False, ctx=ctx).cpu().numpy()
            finally:
                ctx.set_dssp_plan(0)
            assert np.array_equal(got[:hf], want), f"{label}: the {name} plan differs from the restatement"
        ms = both_plans(ctx, d, rest, calls, 2)
        rows.append(dict(workload=key, label=label, residues=int(rest[0].shape[0]), frames=F, host_ms_per_frame=host_ms_per_frame,
                         **{f"{name}_ms": ms[name] for name, _ in PLANS},
                         **{f"{name}_frames_per_s": F / (ms[name] * 1e-3) for name, _ in PLANS},
                         host_over_best=host_ms_per_frame * F / min(ms.values())))
    sweeps = {}
    if not args.no_sweep:
        for label, make, counts in (("3PTB backbone", lambda: C.noisy_3ptb(256), (1, 2, 4, 8, 16, 32, 48, 64, 96, 128, 160, 192, 224, 256)),
                                    ("1 000-residue chain", lambda: synthetic_chain(1000, 256, 23), (1, 8, 16, 32, 48, 64, 96, 128, 256))):
            coords, *rest = make()
            sweep = []
            for F in counts:
                d = torch.as_tensor(np.ascontiguousarray(coords[:, :, :F])).cuda()
                ms = both_plans(ctx, d, rest, 10, 2)
                sweep.append(dict(n_frames=F, frames_ms=ms["frames"], acceptors_ms=ms["acceptors"]))
            # the first frame count from which the frames plan stays the faster one
            cross = None
            for s in reversed(sweep):
                if s["frames_ms"] > s["acceptors_ms"]:
                    break
                cross = s["n_frames"]
            sweeps[label] = dict(residues=int(rest[0].shape[0]), sweep=sweep, frames_plan_wins_from=cross)
    if args.json:
        print(json.dumps(dict(workloads=rows, sweeps=sweeps)))
        return
    print("| workload | residues x frames | frames plan ms | acceptors plan ms | host restatement ms / frame | host / best plan |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| ({r['workload']}) {r['label']} | {r['residues']} x {r['frames']} | {r['frames_ms']:.3f} | {r['acceptors_ms']:.3f} | "
              f"{r['host_ms_per_frame']:.1f} | {r['host_over_best']:.0f} |")
    for label, sw in sweeps.items():
        print(f"\n| {label}: frames | frames plan ms | acceptors plan ms |\n|---|---|---|")
        for s in sw["sweep"]:
            print(f"| {s['n_frames']} | {s['frames_ms']:.3f} | {s['acceptors_ms']:.3f} |")
        print(f"\n{label} ({sw['residues']} residues): the frames plan is the faster one from {sw['frames_plan_wins_from']} frames on")


if __name__ == "__main__":
    main()
