"""tests/golden/make_golden_bonds.py -- writes tests/golden/bond_cases.npz: what the REFERENCE returns on the golden cases of
tests/bonds_cases.py, as data.  Not run by the suite; nothing of the reference is in this file or in the npz but its results.

It needs the reference's bond guesser with its compiled pair loop, which takes Cython and a C++ compiler and is done once, in a
scratch directory OUTSIDE this repository (nothing compiled is ever committed) -- a stub package that holds nothing but the guesser:

    mkdir -p /tmp/refbonds/moleculekit && cd /tmp/refbonds/moleculekit
    : > __init__.py
    cp $MOLECULEKIT_REF/moleculekit/bondguesser.py .
    cp $MOLECULEKIT_REF/moleculekit/bondguesser_utils/bondguesser_utils.pyx .
    cython -3 --cplus bondguesser_utils.pyx
    g++ -O2 -fPIC -shared -fwrapv -fno-strict-aliasing $(python3-config --includes) \\
        -I$(python -c "import numpy; print(numpy.get_include())") bondguesser_utils.cpp \\
        -o bondguesser_utils$(python3-config --extension-suffix)

    MOLECULEKIT_REF_BONDS=/tmp/refbonds python tests/golden/make_golden_bonds.py

``MOLECULEKIT_REF_BONDS``: the directory that holds the stub package.

The npz holds, per golden case NAME, the inputs as they went to the reference -- ``NAME/coords`` float32 [N, 3], ``NAME/radii`` float32
[N], ``NAME/is_h`` uint32 [N], ``NAME/grid_cutoff`` float64, and ``NAME/element`` / ``NAME/name`` for the cases that went through
``guess_bonds`` (a SimpleNamespace with numAtoms, frame, numFrames, coords, element, name) instead of ``bond_grid_search`` -- and what
it returned: ``NAME/pairs`` uint32 [n, 2], in its order.

Asserted before anything is written: the reference's list of the 3PTB case IS the ``bonds`` array of tests/golden/channels_3ptb.npz;
every case meant to hold both bonds and rejected in-grid pairs does (tests/bonds_cases.py: check, on the restatement, and the
reference's list is not empty); the cases with ``element`` send the reference the radii, flags and cut-off the case carries.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import bonds_cases as C  # noqa: E402


def main():
    sys.path.insert(0, os.environ["MOLECULEKIT_REF_BONDS"])
    import moleculekit.bondguesser as ref  # the stub package: the reference's guesser

    C.check()
    out = {}
    for name in C.GOLDEN:
        c = C.case(name)
        if "element" in c:
            seen = {}
            search = ref.bond_grid_search

            def spy(coords, grid_cutoff, is_hydrogen, radii, *a, **k):
                seen.update(coords=coords, grid_cutoff=grid_cutoff, is_h=is_hydrogen, radii=radii)
                return search(coords, grid_cutoff, is_hydrogen, radii, *a, **k)

            ref.bond_grid_search = spy
            try:
                pairs = ref.guess_bonds(C.as_mol(c))
            finally:
                ref.bond_grid_search = search
            assert np.array_equal(seen["coords"], c["coords"]) and np.array_equal(seen["radii"], c["radii"]) and seen["radii"].dtype == np.float32
            assert np.array_equal(seen["is_h"], c["is_h"]) and float(seen["grid_cutoff"]) == c["grid_cutoff"]
            out[f"{name}/element"], out[f"{name}/name"] = c["element"], c["name"]
        else:
            pairs = ref.bond_grid_search(c["coords"], c["grid_cutoff"], c["is_h"], c["radii"])
        assert pairs.dtype == np.uint32 and pairs.ndim == 2 and pairs.shape[1] == 2
        if name == "3ptb":
            assert np.array_equal(pairs, c["expected"]), "the reference's 3PTB list is not the fixture's bonds"
        if name in C.MIXED:
            assert len(pairs), f"{name}: no bond"
        out[f"{name}/coords"], out[f"{name}/radii"], out[f"{name}/is_h"] = c["coords"], c["radii"], c["is_h"]
        out[f"{name}/grid_cutoff"] = np.float64(c["grid_cutoff"])
        out[f"{name}/pairs"] = pairs
        same = np.array_equal(pairs, C.restated(name)[0])
        print(f"{name}: {len(pairs)} pairs, restatement {'equal' if same else 'DIFFERENT'}")
    path = os.path.join(HERE, "bond_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
