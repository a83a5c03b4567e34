"""tests/golden/make_golden_within.py -- writes tests/golden/within_cases.npz: what the compiled REFERENCE's
``atomselect_utils.within_distance`` leaves in its results array on the golden cases of tests/within_cases.py, as data.  Not run by the
suite; nothing of the reference is in this file or in the npz but its results.

It needs the reference's compiled loop, which takes Cython and a C++ compiler and is done once, in a scratch directory OUTSIDE this
repository (nothing compiled is ever committed), with the reference's own flags (setup.py: C++, -O3):

    mkdir -p /tmp/refwithin && cd /tmp/refwithin
    cp $MOLECULEKIT_REF/moleculekit/atomselect_utils/atomselect_utils.pyx .
    cython -3 --cplus atomselect_utils.pyx
    INC="$(python3-config --includes) -I$(python -c 'import numpy; print(numpy.get_include())')"
    g++ -O3 -fPIC -shared -fwrapv -fno-strict-aliasing $INC atomselect_utils.cpp -o atomselect_utils$(python3-config --extension-suffix)

    MOLECULEKIT_REF_WITHIN=/tmp/refwithin python tests/golden/make_golden_within.py

The npz holds, per golden case NAME, the inputs as they went to the reference -- ``NAME/coords`` float32 [F, N, 3], ``NAME/sel1`` and
``NAME/sel2`` uint32, ``NAME/cutoff`` float64 (the Python float; the reference's C ``float`` argument rounds it), ``NAME/mn`` and
``NAME/mx`` float32 [F, 3] (the gate bounds), ``NAME/preset`` bool [F, n1] (the results array on entry; absent: all False) -- and
``NAME/results`` bool [F, n1]: the results array after the call.  A case of several frames calls the reference once per frame.

Asserted before anything is written: that every case is the case it is meant to be (tests/within_cases.py: check, on the restatement),
and that the numpy restatement (tests/within_restatement.py) equals the compiled reference on every case.  With ``--time`` it also
prints the compiled reference's time on the first two shapes of tools/bench_within.py (context for DESIGN.md section 18).
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import within_cases as C  # noqa: E402


def reference_results(ref, c):
    F = c["coords"].shape[0]
    out = np.zeros((F, len(c["sel1"])), bool) if c["preset"] is None else c["preset"].copy()
    for f in range(F):
        ref.within_distance(np.ascontiguousarray(c["coords"][f]), c["cutoff"], c["sel1"], c["sel2"], c["mn"][f].copy(), c["mx"][f].copy(), out[f])
    return out


def timings(ref):
    rng = np.random.default_rng(0)
    d = np.load(os.path.join(HERE, "channels_3ptb.npz"))
    coords = d["coords"].astype(np.float32)
    lig = np.flatnonzero(d["resname"] == "BEN").astype(np.uint32)
    shapes = [("3PTB around its ligand", coords, np.arange(len(coords), dtype=np.uint32), lig, 5.0)]
    side = (103000 / 0.1) ** (1 / 3)                                  # 0.1 atoms per cubic angstrom
    big = (rng.random((103000, 3)) * side).astype(np.float32)
    centre = np.argsort(np.linalg.norm(big - side / 2, axis=1))[:3000].astype(np.uint32)
    shapes.append(("100 000 atoms around a 3 000-atom solute", big, np.arange(len(big), dtype=np.uint32), centre, 5.0))
    for name, xyz, s1, s2, cut in shapes:
        best = []
        for _ in range(5):
            out = np.zeros(len(s1), bool)
            t0 = time.perf_counter()
            ref.within_distance(xyz, cut, s1, s2, xyz[s2].min(axis=0), xyz[s2].max(axis=0), out)
            best.append(time.perf_counter() - t0)
        print(f"compiled reference, {name}: median {np.median(best) * 1e3:.2f} ms of 5 ({int(out.sum())} within)")


def main():
    sys.path.insert(0, os.environ["MOLECULEKIT_REF_WITHIN"])
    import atomselect_utils as ref  # the compiled reference, alone

    C.check()
    out = {}
    for name in C.GOLDEN:
        c = C.case(name)
        got = reference_results(ref, c)
        assert got.dtype == bool and got.shape == (c["coords"].shape[0], len(c["sel1"]))
        same = np.array_equal(got, C.restated(name))
        print(f"{name}: {got.shape[0]} x {got.shape[1]} results, {int(got.sum())} True, restatement {'equal' if same else 'DIFFERENT'}")
        assert same, f"{name}: the restatement differs from the compiled reference"
        for k in ("coords", "sel1", "sel2", "mn", "mx"):
            out[f"{name}/{k}"] = c[k]
        out[f"{name}/cutoff"] = np.float64(c["cutoff"])
        if c["preset"] is not None:
            out[f"{name}/preset"] = c["preset"]
        out[f"{name}/results"] = got
    path = os.path.join(HERE, "within_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    if "--time" in sys.argv:
        timings(ref)


if __name__ == "__main__":
    main()
