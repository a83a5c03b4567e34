#!/usr/bin/env python3
"""Periodic wrap (moleculekit_amd.wrap.wrap_trajectory) beside a torch.clone of the same tensor on the same device in the same run: the
clone is one read and one write of the trajectory, the floor of an out-of-place pass.

Shapes: (a) 30 000 atoms x 2 048 frames: one 4 480-atom chain, 8 506 waters of 3 atoms and 2 ions; (b) the topology of the reference's
wrapping fixture (tests/golden: 167 262 atoms in 43 129 groups, chains of 467 to 3 384 atoms, 134-atom lipids, waters, ions) x 64
frames.  The atoms are spread over two box lengths per axis, so most groups move.  Cases: in place and out of place, the centre given
and the centre selected (the chain / the four chains).  Before an in-place call the unwrapped coordinates are copied back, outside
the timed window: a second wrap of wrapped coordinates would move nothing and write nothing.  Per case: events around each call, 3
warm-up calls, 20 timed calls, three rounds with the wrap and the clone alternating, the median round.  In place and out of place
are asserted bit-equal before anything is timed.

    python tools/bench_wrap.py [--json] [--only ab]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def timed(fn, before=None, calls=20, warmup=3):
    import torch
    ts = []
    for i in range(warmup + calls):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def topology(key):
    """(group starts, centre selection)"""
    if key == "a":
        sizes = np.r_[4480, np.full(8506, 3), 1, 1]
        return np.r_[0, np.cumsum(sizes)].astype(np.uint32), np.arange(4480, dtype=np.uint32)
    z = np.load(os.path.join(ROOT, "tests", "golden", "wrap_cases.npz"))
    return z["group_starts"], np.arange(6814, dtype=np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--only", default="ab")
    args = ap.parse_args()
    import torch
    from moleculekit_amd import _lib, wrap
    ctx = _lib.default_context()
    dev = torch.device("cuda", 0)
    shapes = {"a": ("one 4 480-atom chain + waters", 2048), "b": ("6X18 topology", 64)}
    rows = []
    for key in args.only:
        label, F = shapes[key]
        starts, centersel = topology(key)
        N, G = int(starts[-1]), int(starts.size) - 1
        g = torch.Generator(device="cuda").manual_seed(23)
        box = (60.0 + 5.0 * torch.rand(3, F, device=dev, generator=g)).contiguous()
        gid = torch.as_tensor(np.repeat(np.arange(G), np.diff(starts.astype(np.int64))), device=dev)
        centres = (torch.rand(F, G, 3, device=dev, generator=g) * 2.0 - 0.5) * box.T[:, None, :]
        orig = (centres[:, gid, :] + 1.5 * torch.randn(F, N, 3, device=dev, generator=g)).contiguous()
        del centres
        work, out = orig.clone(), torch.empty_like(orig)
        centre = [30.0, 30.0, 30.0]
        for how, kw in (("centre given", dict(center=centre)), ("centre selected", dict(centersel=centersel))):
            wrap.wrap_trajectory(orig, box, starts, out=out, ctx=ctx, **kw)
            kernel = ctx.last_dist_kernel()
            work.copy_(orig)
            wrap.wrap_trajectory(work, box, starts, out=work, ctx=ctx, **kw)
            assert torch.equal(work.view(torch.int32), out.view(torch.int32)), "in place and out of place differ"
            moved = float((out != orig).any(dim=2).float().mean())
            for place, fn, before in (("out of place", lambda: wrap.wrap_trajectory(orig, box, starts, out=out, ctx=ctx, **kw), None),
                                      ("in place", lambda: wrap.wrap_trajectory(work, box, starts, out=work, ctx=ctx, **kw), lambda: work.copy_(orig))):
                rounds = sorted((timed(fn, before), timed(lambda: orig.clone())) for _ in range(3))
                t_w, t_c = rounds[1]
                rows.append(dict(shape=key, label=label, N=N, F=F, G=G, case=f"{place}, {how}", kernel=kernel.replace("mkamd::", ""),
                                 atoms_moved=moved, wrap_ms=t_w, clone_ms=t_c, ratio=t_w / t_c))
        del orig, work, out
    if args.json:
        print(json.dumps(rows))
        return
    print("| shape | N x F, groups | case | kernels | atoms moved | wrap ms | clone ms | wrap / clone |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| ({r['shape']}) {r['label']} | {r['N']} x {r['F']}, {r['G']} | {r['case']} | {r['kernel']} | {r['atoms_moved']:.2f} | "
              f"{r['wrap_ms']:.4f} | {r['clone_ms']:.4f} | {r['ratio']:.2f} |")


if __name__ == "__main__":
    main()
