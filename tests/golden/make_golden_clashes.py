"""tests/golden/make_golden_clashes.py -- writes tests/golden/clash_cases.npz: what the REFERENCE returns on the golden cases of
tests/clashes_cases.py, as data.  Not run by the suite; nothing of the reference is in this file or in the npz but its results.
Written with numpy 2.2.6 (the reference's float32 arithmetic depends on numpy 2's scalar promotion and on its einsum).

It needs the reference's ``find_clashes`` with its compiled kd-tree and its bond guesser with its compiled pair loop, which takes Cython
and a C++ compiler and is done once, in a scratch directory OUTSIDE this repository (nothing compiled is ever committed) -- a stub
package that holds nothing but these (the bond guesser as in make_golden_bonds.py):

    mkdir -p /tmp/refclash/moleculekit/kdtree && cd /tmp/refclash/moleculekit
    : > __init__.py
    cp $MOLECULEKIT_REF/moleculekit/distance.py $MOLECULEKIT_REF/moleculekit/periodictable.py $MOLECULEKIT_REF/moleculekit/bondguesser.py .
    cp $MOLECULEKIT_REF/moleculekit/bondguesser_utils/bondguesser_utils.pyx .
    cp -r $MOLECULEKIT_REF/moleculekit/kdtree/. kdtree/
    INC="$(python3-config --includes) -I$(python -c 'import numpy; print(numpy.get_include())')"
    cython -3 --cplus bondguesser_utils.pyx
    g++ -O2 -fPIC -shared -fwrapv -fno-strict-aliasing $INC bondguesser_utils.cpp -o bondguesser_utils$(python3-config --extension-suffix)
    cd kdtree && cython -3 --cplus _ckdtree.pyx
    g++ -O2 -std=c++17 -fPIC -shared -fwrapv -fno-strict-aliasing $INC -Isrc _ckdtree.cpp src/build.cxx src/count_neighbors.cxx src/query.cxx \\
        src/query_ball_point.cxx src/query_ball_tree.cxx src/query_pairs.cxx src/sparse_distances.cxx -o _ckdtree$(python3-config --extension-suffix)

    MOLECULEKIT_REF_CLASHES=/tmp/refclash python tests/golden/make_golden_clashes.py

``find_clashes`` takes a Molecule; the one here is a stand-in of this project's with the two methods the function calls, restated from
the reference's Molecule: ``atomselect`` for None, boolean masks and index arrays, and ``_getBonds`` -- the file bonds stacked on the
reference guesser's bonds.

The npz holds, per golden case NAME, the inputs as they went to the reference -- ``NAME/coords`` float32 [N, 3], ``NAME/element``,
``NAME/name``, ``NAME/bonds`` uint32 [nb, 2] (or ``NAME/inputs_of``: the case whose four arrays they are), ``NAME/sel1`` / ``NAME/sel2``
(absent: None), ``NAME/overlap`` float64, ``NAME/flags`` uint8 [3] = exclude_bonded, exclude_14, guess_bonds -- the bond list the
reference built its exclusions from, ``NAME/bonds_used`` (where it guessed; otherwise it is ``bonds``) -- and what it returned:
``NAME/pairs`` int64 [n, 2], ``NAME/distances`` float32 [n], ``NAME/overlaps`` float32 [n].

The reference sorts by overlap with an unstable sort, so the order of EQUAL overlaps is not defined; they are put into (a, b) order
before saving.  Asserted before anything is written: that only rows of equal overlap moved; the dtypes and shapes; that every case is
the case it is meant to be (tests/clashes_cases.py: check, on the restatement); that a negative kd-tree radius searches like its
absolute value (the cutoff <= 0 cases rest on it).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import clashes_cases as C  # noqa: E402
import clashes_restatement as R  # noqa: E402


class Mol:
    """the stand-in Molecule"""

    def __init__(self, c, guesser):
        self.coords = c["coords"][:, :, None].copy()
        self.numAtoms, self.frame, self.numFrames = len(c["coords"]), 0, 1
        self.element, self.name, self.bonds = c["element"], c["name"], c["bonds"].copy()
        self._guesser = guesser
        self.bonds_used = None

    def atomselect(self, sel):
        if sel is None:
            return np.ones(self.numAtoms, dtype=bool)
        mask = np.atleast_1d(sel)
        if mask.dtype != bool:
            new_mask = np.zeros(self.numAtoms, dtype=bool)
            new_mask[mask] = True
            mask = new_mask
        return mask

    def _getBonds(self, fileBonds=True, guessBonds=True):
        bonds = np.empty((0, 2), dtype=np.uint32)
        if fileBonds:
            bonds = np.vstack((bonds, self.bonds))
        if guessBonds:
            bonds = np.vstack((bonds, self._guesser(self)))
        self.bonds_used = bonds.astype(np.uint32)
        return self.bonds_used


def main():
    sys.path.insert(0, os.environ["MOLECULEKIT_REF_CLASHES"])
    import moleculekit.bondguesser as refbonds  # the stub package
    import moleculekit.distance as ref
    from moleculekit.kdtree import cKDTree

    C.check()
    pts = np.random.default_rng(0).random((80, 3))
    tree = cKDTree(pts)
    assert np.array_equal(tree.query_pairs(-0.3, output_type="ndarray"), tree.query_pairs(0.3, output_type="ndarray")) and len(tree.query_pairs(0.3))
    out = {}
    for name in C.GOLDEN:
        c = C.case(name)
        mol = Mol(c, refbonds.guess_bonds)
        pairs, distances, overlaps = ref.find_clashes(mol, **C.kwargs(c))
        assert pairs.dtype == np.int64 and pairs.shape == (len(distances), 2) and distances.dtype == np.float32 and overlaps.dtype == np.float32
        assert distances.shape == overlaps.shape == (len(pairs),)
        cp, cd, co = R.canonical(pairs, distances, overlaps)
        assert np.array_equal(co, overlaps), f"{name}: canonicalising moved rows of different overlap"
        assert sorted(map(tuple, np.column_stack([pairs, distances.view(np.int32), overlaps.view(np.int32)]).tolist())) == \
            sorted(map(tuple, np.column_stack([cp, cd.view(np.int32), co.view(np.int32)]).tolist())), f"{name}: canonicalising changed the rows"
        base = C.SAME_INPUTS.get(name)
        if base is None:
            out[f"{name}/coords"], out[f"{name}/element"], out[f"{name}/name"], out[f"{name}/bonds"] = c["coords"], c["element"], c["name"], c["bonds"]
        else:
            b = C.case(base)
            assert all(np.array_equal(c[k], b[k]) for k in ("coords", "element", "name", "bonds"))
            out[f"{name}/inputs_of"] = np.array(base)
        for k in ("sel1", "sel2"):
            if c[k] is not None:
                out[f"{name}/{k}"] = np.asarray(c[k])
        out[f"{name}/overlap"] = np.float64(c["overlap"])
        out[f"{name}/flags"] = np.array([c["exclude_bonded"], c["exclude_14"], c["guess_bonds"]], np.uint8)
        if c["guess_bonds"] and mol.bonds_used is not None:
            if base is None:
                out[f"{name}/bonds_used"] = mol.bonds_used
            else:
                assert np.array_equal(out[f"{base}/bonds_used"], mol.bonds_used)
        out[f"{name}/pairs"], out[f"{name}/distances"], out[f"{name}/overlaps"] = cp, cd, co
        rp, rd, ro, _ = C.restated(name)
        same = np.array_equal(cp, rp) and np.array_equal(cd, rd) and np.array_equal(co, ro)
        moved = int((pairs != cp).any(axis=1).sum())
        print(f"{name}: {len(cp)} rows, {moved} moved among equal overlaps, restatement {'equal' if same else 'DIFFERENT'}")
    path = os.path.join(HERE, "clash_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
