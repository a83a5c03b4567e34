#!/usr/bin/env python3
"""Golden fixture for the periodic wrap (moleculekit_amd/wrap.py).  DATA only: nothing of the reference is run.

    MOLECULEKIT_REF_TESTS=<reference>/tests python3 tests/golden/make_golden_wrap.py

The reference tests Molecule.wrap on `tests/test_wrapping/6X18.{psf,xtc}` (167 262 atoms, one frame, a rectangular box of
94.93 x 95.56 x 178.05 A): test_wrapping.py::test_orthogonal_wrapping asserts that the mean position of all atoms is more than 100 A
from the literal centre before wrapping and less than 1 A after.  This script stores what a test of the same needs without the
reference:

  tests/golden/wrap/wrap_6X18.xtc  test_wrapping/6X18.xtc, byte for byte (623 296 B).  In a directory of its own: every trajectory
                                   under tests/golden/xtc/ is also a fixture of the damaged-stream driver (tests/emu_xtc_damage_build.py),
                                   whose committed case list (tests/golden/xtc_damage_cases.json) numbers its cases over those files
  tests/golden/wrap_cases.npz      (compressed)
    group_starts [43 130] uint32   the start of every bonded group and the number of atoms at the end, derived from
                                   test_wrapping/6X18_expected_group_mask.npy (the group index of every atom; it is non-decreasing,
                                   asserted here: every group is a contiguous run)
    center [3] float32             the literal centre of test_wrapping.py: [94.64, 3.69, 1.11]
"""
import os
import shutil

import numpy as np

REF_TESTS = os.environ["MOLECULEKIT_REF_TESTS"]            # the reference's tests/ directory
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    src = os.path.join(REF_TESTS, "test_wrapping")
    os.makedirs(os.path.join(OUT, "wrap"), exist_ok=True)
    xtc = os.path.join(OUT, "wrap", "wrap_6X18.xtc")
    shutil.copyfile(os.path.join(src, "6X18.xtc"), xtc)
    assert os.path.getsize(xtc) == 623296
    mask = np.load(os.path.join(src, "6X18_expected_group_mask.npy")).astype(np.int64).reshape(-1)
    assert mask.size == 167262 and np.all(np.diff(mask) >= 0), "the group mask must be non-decreasing (contiguous groups)"
    starts = np.r_[0, np.flatnonzero(np.diff(mask)) + 1, mask.size].astype(np.uint32)
    assert starts.size == 43130
    np.savez_compressed(os.path.join(OUT, "wrap_cases.npz"), group_starts=starts, center=np.array([94.64, 3.69, 1.11], np.float32))
    print(xtc, os.path.getsize(xtc), "groups", starts.size - 1, "largest", int(np.diff(starts.astype(np.int64)).max()))


if __name__ == "__main__":
    main()
