"""tests/golden/make_golden_hbonds.py -- writes tests/golden/hbond_cases.npz: what the REFERENCE computes on the golden subset of
tests/hbonds_cases.py, as data.  Not run by the suite; nothing of the reference is in this file or in the npz but its results.

It needs the reference's hydrogen-bond module compiled, which takes Cython and a C++ compiler and is done once, in a scratch directory
OUTSIDE this repository (nothing compiled is ever committed), as tests/golden/make_golden_rings.py describes for its modules:

    mkdir /tmp/refhb && cd /tmp/refhb
    cp $MOLECULEKIT_REF/moleculekit/interactions/hbonds/hbonds.pyx .
    cython -3 --cplus hbonds.pyx
    g++ -O2 -fPIC -shared -fwrapv -fno-strict-aliasing $(python3-config --includes) \\
        -I$(python -c "import numpy; print(numpy.get_include())") hbonds.cpp -o hbonds$(python3-config --extension-suffix)

    MOLECULEKIT_REF_HBONDS=/tmp/refhb python tests/golden/make_golden_hbonds.py

``MOLECULEKIT_REF_HBONDS``: the directory that holds the compiled module.

The npz holds, per golden case NAME, the inputs as tests/hbonds_cases.py generated them here and as they went to the reference's
``calculate`` -- ``NAME/coords`` float32 [N, 3, F], ``NAME/box`` float32 [3, F], ``NAME/donors`` uint32 [nd, 2] ([nd, 1] with
ignore_hs), ``NAME/acceptors`` uint32 [na], ``NAME/sel1`` / ``NAME/sel2`` uint32 [N], ``NAME/params`` float64 (dist_threshold,
angle_threshold, intra, ignore_hs) -- and what it returned, frame after frame: ``NAME/offsets`` int64 [F + 1], ``NAME/triples`` int32
[n, 3] (heavy atom, hydrogen or -1, acceptor).

Asserted on the reference's own results before anything is written: the margin condition of the cases module (no float64 angle of a
tested pair within 1e-4 degrees of the threshold in use; the two exactly collinear threshold-edge cases are exempt), and that the
reference reports at least one pair AND drops at least one allowed pair in every case of ``hbonds_cases.BOTH``.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import hbonds_cases as C  # noqa: E402
from hbonds_restatement import allowed_pairs  # noqa: E402


def main():
    sys.path.insert(0, os.environ["MOLECULEKIT_REF_HBONDS"])
    import hbonds  # the compiled reference

    C.check_margins()
    out = {}
    for name in C.GOLDEN:
        c = C.case(name)
        res = hbonds.calculate(*(c[k] for k in C.ARGS), dist_threshold=c["dist_threshold"], angle_threshold=c["angle_threshold"],
                               intra=c["intra"], ignore_hs=c["ignore_hs"])
        F = c["coords"].shape[2]
        offs = np.zeros(F + 1, np.int64)
        for f in range(F):
            assert len(res[f]) % 3 == 0
            offs[f + 1] = offs[f] + len(res[f]) // 3
        triples = np.array([v for f in range(F) for v in res[f]], dtype=np.int64).astype(np.int32).reshape(-1, 3)
        assert len(triples) == offs[-1]
        allowed = int(allowed_pairs(c["donors"], c["acceptors"], c["sel1"], c["sel2"], c["intra"]).sum()) * F
        if name in C.BOTH:
            assert 0 < len(triples) < allowed, f"{name}: the reference reports {len(triples)} of {allowed} allowed pairs; it must report and drop"
        for k in C.ARGS:
            out[f"{name}/{k}"] = c[k]
        out[f"{name}/params"] = np.array([c["dist_threshold"], c["angle_threshold"], c["intra"], c["ignore_hs"]], np.float64)
        out[f"{name}/offsets"], out[f"{name}/triples"] = offs, triples
        print(f"{name}: {len(triples)} of {allowed} allowed pairs reported")
    path = os.path.join(HERE, "hbond_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
