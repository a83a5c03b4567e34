#!/usr/bin/env python3
"""Periodic wrap of a triclinic box (moleculekit_amd.wrap.wrap_cell_trajectory), all three unit cells, beside the rectangular
wrap_trajectory of the same tensor (its kernels are wrap_kernels.h's, unchanged) and a torch.clone of it, on the same device in the
same run.

Shapes: those of tools/bench_wrap.py -- (a) 30 000 atoms x 2 048 frames: one 4 480-atom chain, 8 506 waters and 2 ions; (b) the
topology of the reference's wrapping fixture x 64 frames -- in a rhombic dodecahedron (angles 60, 60, 90) of the volume of the
rectangular wrap's box of that frame (edge = (volume * sqrt 2)^(1/3)).  The atoms are spread over two box lengths per axis.  The cell
is centred on the chain(s).  Cases: the three unit cells, in place and out of place.  Before an in-place call the unwrapped coordinates
are copied back, outside the timed window (a second wrap of wrapped coordinates would take no steps).  Per case: events around each
call, 3 warm-up calls, 20 timed calls, three rounds with the cell wrap, the rectangular wrap and the clone alternating, the median round
(by the cell wrap's time).  In place and out of place are asserted bit-equal, and the status words zero, before anything is timed.

    python tools/bench_wrap_cell.py [--json] [--only ab]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_wrap import timed, topology  # noqa: E402


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
        edge = (box.double().prod(dim=0) * 2.0 ** 0.5) ** (1.0 / 3.0)                       # [F]: the dodecahedron of the same volume
        lengths = edge.cpu().numpy()[None, :].repeat(3, axis=0)
        boxvectors = torch.as_tensor(wrap.box_vectors(lengths, np.array([60.0, 60.0, 90.0])[:, None].repeat(F, axis=1)), device=dev)
        work, out = orig.clone(), torch.empty_like(orig)
        kw = dict(centersel=centersel, ctx=ctx, check=False)
        for cell in ("rectangular", "compact", "triclinic"):
            _, status = wrap.wrap_cell_trajectory(orig, boxvectors, starts, cell, out=out, **kw)
            kernel = ctx.last_dist_kernel()
            work.copy_(orig)
            wrap.wrap_cell_trajectory(work, boxvectors, starts, cell, out=work, **kw)
            assert torch.equal(work.view(torch.int32), out.view(torch.int32)), "in place and out of place differ"
            assert not status.cpu().numpy().any(), wrap.status_error(status.cpu().numpy())
            for place, fn, rect, before in (
                    ("out of place", lambda: wrap.wrap_cell_trajectory(orig, boxvectors, starts, cell, out=out, **kw),
                     lambda: wrap.wrap_trajectory(orig, box, starts, centersel=centersel, out=out, ctx=ctx), None),
                    ("in place", lambda: wrap.wrap_cell_trajectory(work, boxvectors, starts, cell, out=work, **kw),
                     lambda: wrap.wrap_trajectory(work, box, starts, centersel=centersel, out=work, ctx=ctx), lambda: work.copy_(orig))):
                rounds = sorted((timed(fn, before), timed(rect, before), timed(lambda: orig.clone())) for _ in range(3))
                t_w, t_r, t_c = rounds[1]
                rows.append(dict(shape=key, label=label, N=N, F=F, G=G, case=f"{cell}, {place}", kernel=kernel.replace("mkamd::", ""),
                                 cell_ms=t_w, rect_ms=t_r, clone_ms=t_c, over_rect=t_w / t_r, over_clone=t_w / t_c))
        del orig, work, out
    if args.json:
        print(json.dumps(rows))
        return
    print("| shape | N x F, groups | unit cell | kernels | cell wrap ms | rectangular wrap ms | clone ms | cell / rectangular | cell / clone |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| ({r['shape']}) {r['label']} | {r['N']} x {r['F']}, {r['G']} | {r['case']} | {r['kernel']} | {r['cell_ms']:.4f} | "
              f"{r['rect_ms']:.4f} | {r['clone_ms']:.4f} | {r['over_rect']:.2f} | {r['over_clone']:.2f} |")


if __name__ == "__main__":
    main()
