"""tests/golden/make_golden_rings.py -- writes tests/golden/ring_cases.npz: what the REFERENCE computes on the golden subset of
tests/rings_cases.py, as data.  Not run by the suite; nothing of the reference is in this file or in the npz but its results.

It needs the reference's three ring modules compiled, which takes Cython and a C++ compiler and is done once, in a scratch directory
OUTSIDE this repository (nothing compiled is ever committed):

    mkdir /tmp/refrings && cd /tmp/refrings
    for m in pipi cationpi sigmahole; do
        cp $MOLECULEKIT_REF/moleculekit/interactions/$m/$m.pyx .
        cython -3 --cplus $m.pyx
        g++ -O2 -fPIC -shared -fwrapv -fno-strict-aliasing $(python3-config --includes) \\
            -I$(python -c "import numpy; print(numpy.get_include())") $m.cpp -o $m$(python3-config --extension-suffix)
    done

    MOLECULEKIT_REF_RINGS=/tmp/refrings python tests/golden/make_golden_rings.py

``MOLECULEKIT_REF_RINGS``: the directory that holds the three compiled modules.

The npz holds, per golden case NAME: the inputs as tests/rings_cases.py generated them here and as they went to the reference's
``calculate`` -- ``NAME/kind``, ``NAME/coords`` float32 [N, 3, F], ``NAME/box`` float32 [3, F], ``NAME/ring_atoms``, ``NAME/starts1``,
``NAME/second`` (pi-pi: the second list's offsets; cation-pi: the cations; sigma-hole: the halide rows), ``NAME/thr`` -- and what it
returned, frame after frame: ``NAME/offsets`` int64 [F + 1], ``NAME/pairs`` uint32 [n, 2], ``NAME/distang`` float32 [n, 2].

Two things are asserted on the reference's own results before anything is written: no float32 angle it reported lies within 1e-4
degrees of a threshold in use (the comparisons of the suite rest on that margin; the cases module asserts it on the float64 angles of
every tested pair), and the stacked-copy case has frames in which the pair is reported AND frames in which it is dropped.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import rings_cases as C  # noqa: E402


def main():
    sys.path.insert(0, os.environ["MOLECULEKIT_REF_RINGS"])
    import cationpi  # the compiled reference
    import pipi
    import sigmahole

    C.check_margins()
    out = {}
    for name in C.GOLDEN:
        c = C.case(name)
        atoms, s1, second = C.flatten(c)
        coords, box, thr = c["coords"], c["box"], [float(t) for t in c["thr"]]
        if c["kind"] == C.PIPI:
            res, da = pipi.calculate(atoms, s1, second, coords, box, dist_threshold1=thr[0], angle_threshold1_max=thr[1], dist_threshold2=thr[2],
                                     angle_threshold2_min=thr[3])
            in_use = (thr[1], thr[3])
        elif c["kind"] == C.CATIONPI:
            res, da = cationpi.calculate(atoms, s1, second, coords, box, dist_threshold=thr[0], angle_threshold_min=thr[1])
            in_use = (thr[1],)
        else:
            res, da = sigmahole.calculate(atoms, s1, second, coords, box, dist_threshold=thr[0], angle_threshold_min=thr[1])
            in_use = (thr[1],)
        F = coords.shape[2]
        offs = np.zeros(F + 1, np.int64)
        for f in range(F):
            offs[f + 1] = offs[f] + len(res[f]) // 2
        pairs = np.array([v for f in range(F) for v in res[f]], dtype=np.int64).astype(np.uint32).reshape(-1, 2)
        distang = np.array([v for f in range(F) for v in da[f]], dtype=np.float32).reshape(-1, 2)
        assert len(pairs) == len(distang) == offs[-1]
        if len(distang):
            margin = min(float(np.min(np.abs(distang[:, 1].astype(np.float64) - float(np.float32(t))))) for t in in_use)
            assert margin >= C.MARGIN_DEG, f"{name}: a reported angle lies {margin:.3g} degrees from a threshold"
        if name == "pp_stacked_copy":
            per_frame = np.diff(offs)
            assert per_frame.max() == 1 and per_frame.min() == 0, "the stacked copy must be reported in some frames and dropped in others"
            print(f"{name}: reported in {int(per_frame.sum())} of {F} frames")
        out[f"{name}/kind"] = np.int32(c["kind"])
        out[f"{name}/coords"], out[f"{name}/box"] = coords, box
        out[f"{name}/ring_atoms"], out[f"{name}/starts1"], out[f"{name}/second"] = atoms, s1, second
        out[f"{name}/thr"] = np.asarray(thr, np.float32)
        out[f"{name}/offsets"], out[f"{name}/pairs"], out[f"{name}/distang"] = offs, pairs, distang
        print(f"{name}: {len(pairs)} pairs")
    path = os.path.join(HERE, "ring_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
