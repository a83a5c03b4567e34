#!/usr/bin/env python3
"""Golden fixtures for the XTC decoders on streams the REFERENCE writes (tests/test_xtc_reference_streams.py, GPU tier).

    python3 tests/golden/make_golden_xtc_reference.py

The seeded trajectories of tests/xtc_cases.py compressed by the reference's own ``write_xtc`` (oracle/xtcref.py, built from
the reference tree by ``oracle.build_ref_xtc()``) -> tests/golden/xtc_reference/<name>.xtc, and what the reference's own
``read_xtc`` decodes from exactly those files (coords float32 [F,N,3] nm, box vectors [F,3,3], time, step, precision) ->
<name>_decoded.npz.  Stores DATA only; the GPU tier reads them without the reference."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle.xtcref import ref_read_xtc  # noqa: E402
from tests import xtc_cases  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "xtc_reference")


def fixture_cases():
    """The named cases small enough to commit (the flag-free stream with 4 frames instead of 24)."""
    keep = []
    for c in xtc_cases.named_cases(seed=0):
        if c.name == "flag_free":
            c = xtc_cases.flag_free_then_edge(np.random.default_rng(6), F=4)
        keep.append(c)
    return keep


def main():
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for c in fixture_cases():
        fn = xtc_cases.write(c, os.path.join(OUT, c.name + ".xtc"))
        coords, box, time, step, prec = ref_read_xtc(fn, c.coords.shape[1])
        np.savez_compressed(os.path.join(OUT, c.name + "_decoded.npz"), coords=coords, box=box, time=time, step=step, precision=prec)
        total += os.path.getsize(fn) + os.path.getsize(os.path.join(OUT, c.name + "_decoded.npz"))
        print(f"{c.name}: {coords.shape[1]} atoms x {coords.shape[0]} frames, {os.path.getsize(fn)} bytes")
    print(f"total {total} bytes")


if __name__ == "__main__":
    main()
