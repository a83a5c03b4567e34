"""tests/golden/make_golden_wrap_cell.py -- writes tests/golden/wrap_cell_cases.npz: what the REFERENCE computes on the golden subset of
tests/wrap_cell_cases.py, as data.  Not run by the suite; nothing of the reference is in this file or in the npz but its results.

It needs the reference's ``wrapping`` module compiled, which takes Cython and a C compiler and is done once, in a scratch directory
OUTSIDE this repository (nothing compiled is ever committed):

    mkdir /tmp/refwrap && cd /tmp/refwrap
    cp $MOLECULEKIT_REF/moleculekit/wrapping/wrapping.pyx .
    cython -3 wrapping.pyx
    gcc -O2 -fPIC -shared -fwrapv -fno-strict-aliasing $(python3-config --includes) \\
        -I$(python -c "import numpy; print(numpy.get_include())") wrapping.c -o wrapping$(python3-config --extension-suffix)

    MOLECULEKIT_REF=<the reference's checkout> MOLECULEKIT_REF_WRAPPING=/tmp/refwrap python tests/golden/make_golden_wrap_cell.py

``MOLECULEKIT_REF_WRAPPING``: the directory that holds the compiled module; ``MOLECULEKIT_REF``: the reference's source tree, from
which ``moleculekit/unitcell.py`` is loaded by path (it needs numpy only).

The npz holds, per golden case NAME: ``NAME/xyz`` float32 [F, N, 3], ``NAME/boxvectors`` float64 [3, 3, F], ``NAME/starts``, ``NAME/centersel``
(empty: none), ``NAME/center`` -- the inputs as tests/wrap_cell_cases.py generated them here -- and ``NAME/rectangular``, ``NAME/compact``,
``NAME/triclinic`` float32 [F, N, 3]: wrap_compact_unitcell (mode 0, mode 1) and wrap_triclinic_unitcell of the reference.  And for the box
vectors: ``bv/lengths`` [3, K], ``bv/angles`` [3, K] and ``bv/vectors`` float64 [3, 3, K], lengths_and_angles_to_box_vectors of the
reference on the cases' boxes and on angles of 90 and near 90 that exercise its snap to zero.
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import wrap_cell_cases as C  # noqa: E402


def main():
    sys.path.insert(0, os.environ["MOLECULEKIT_REF_WRAPPING"])
    import wrapping  # the compiled reference

    spec = importlib.util.spec_from_file_location("ref_unitcell", os.path.join(os.environ["MOLECULEKIT_REF"], "moleculekit", "unitcell.py"))
    unitcell = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(unitcell)

    out = {}
    for name in C.GOLDEN:
        c = C.cases()[name]
        sel = np.zeros(0, np.uint32) if c.centersel is None else np.ascontiguousarray(c.centersel, np.uint32)
        cen = np.zeros(3, np.float32) if c.center is None else np.ascontiguousarray(c.center, np.float32)
        groups = np.ascontiguousarray(c.starts, np.uint32)
        bv = np.ascontiguousarray(c.boxvectors, np.float64)
        out[f"{name}/xyz"], out[f"{name}/boxvectors"], out[f"{name}/starts"] = c.xyz, bv, groups
        out[f"{name}/centersel"], out[f"{name}/center"] = sel, cen
        for mode in C.MODES:
            coords = np.ascontiguousarray(np.transpose(c.xyz, (1, 2, 0)))          # [N, 3, F], wrapped in place
            if mode == "triclinic":
                wrapping.wrap_triclinic_unitcell(groups, coords, bv, sel, cen)
            else:
                wrapping.wrap_compact_unitcell(groups, coords, bv, sel, cen, 1 if mode == "compact" else 0)
            out[f"{name}/{mode}"] = np.ascontiguousarray(np.transpose(coords, (2, 0, 1)))

    lengths, angles = [], []
    for L, A in C.BOXES.values():
        lengths.append(L)
        angles.append(A)
    for L, A in (((30.0, 40.0, 50.0), (90.0, 90.0, 90.0)), ((30.0, 40.0, 50.0), (90.00001, 89.99999, 90.0)),
                 ((30.0, 40.0, 50.0), (90.0001, 89.9999, 90.001)), ((12.5, 12.5, 12.5), (89.999999, 90.0, 60.0)),
                 ((81.3, 77.7, 93.1), (61.2, 118.4, 91.0)), ((1e-7, 5.0, 6.0), (90.0, 90.0, 90.0)),
                 ((np.float32(94.93), np.float32(95.56), np.float32(178.05)), (np.float32(60.0), np.float32(90.0), np.float32(109.4712)))):
        lengths.append(L)
        angles.append(A)
    L, A = np.array(lengths, np.float64).T, np.array(angles, np.float64).T          # [3, K]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a, b, c = unitcell.lengths_and_angles_to_box_vectors(L[0], L[1], L[2], A[0], A[1], A[2])
    out["bv/lengths"], out["bv/angles"] = L, A
    out["bv/vectors"] = np.ascontiguousarray(np.transpose(np.stack((a, b, c), axis=1), (1, 2, 0)), dtype=np.float64)   # as Molecule.boxvectors
    np.savez_compressed(C.GOLDEN_FILE, **out)
    print(C.GOLDEN_FILE, os.path.getsize(C.GOLDEN_FILE), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
