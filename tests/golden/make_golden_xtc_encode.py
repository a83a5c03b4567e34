#!/usr/bin/env python3
"""Golden INPUTS for the device XTC writer (tests/test_gpu_xtc_encode.py; tests/test_xtc_encode_cpu.py checks them).

    python3 tests/golden/make_golden_xtc_encode.py

The trajectories of ``make_golden_xtc_reference.fixture_cases()`` as data -> tests/golden/xtc_encode_inputs.npz (per case
``<name>__coords`` float32 [F, N, 3] nm, ``<name>__box`` float32 [F, 3, 3], ``<name>__precision`` float32 [F]), so that the GPU tier
does not rest on a random generator's stream.  Before it stores them, the script asserts that the reference's writer
(oracle/xtcref.py) turns exactly these arrays into exactly the committed tests/golden/xtc_reference/<name>.xtc.  Stores DATA only."""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from make_golden_xtc_reference import OUT as REF_DIR, fixture_cases  # noqa: E402
from oracle.xtcref import ref_write_xtc  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "xtc_encode_inputs.npz")


def main():
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        for c in fixture_cases():
            F = c.coords.shape[0]
            coords = np.ascontiguousarray(c.coords, np.float32)
            box = np.ascontiguousarray(c.box, np.float32)
            prec = np.ascontiguousarray(np.broadcast_to(np.asarray(c.precision, np.float32), (F,)))
            fn = os.path.join(tmp, c.name + ".xtc")
            ref_write_xtc(fn, coords, box, precision=prec)
            with open(fn, "rb") as a, open(os.path.join(REF_DIR, c.name + ".xtc"), "rb") as b:
                assert a.read() == b.read(), f"{c.name}: the reference writer does not reproduce the committed file from these inputs"
            arrays[c.name + "__coords"], arrays[c.name + "__box"], arrays[c.name + "__precision"] = coords, box, prec
            print(f"{c.name}: {coords.shape[1]} atoms x {F} frames")
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
