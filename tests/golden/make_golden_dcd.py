"""tests/golden/make_golden_dcd.py -- records what the reference's DCD reader and writer do with the cases of tests/dcd_cases.py, into
tests/golden/dcd_cases.npz.  Run once, by hand, where the reference (moleculekit) source tree is at hand; the tests only read the npz.

The reference's reader is a compiled module.  Build it in a scratch directory OUTSIDE this repository (nothing of it is committed):

    cp <moleculekit>/fileformats/dcd/dcd.pyx <moleculekit>/fileformats/dcd/dcdlib.pxd .
    cython -3 dcd.pyx
    gcc -O2 -fno-strict-aliasing -shared -fPIC dcd.c <moleculekit>/fileformats/dcd/src/dcdplugin.c -I<moleculekit>/fileformats/dcd \
        -I<moleculekit>/fileformats/dcd/include $(python3-config --includes) -I$(python -c "import numpy; print(numpy.get_include())") \
        -o dcd$(python3-config --extension-suffix)
    # (-fno-strict-aliasing: the plugin byte-swaps a float through an int pointer; an optimiser that assumes strict aliasing drops that
    #  swap and an opposite-endian header's DELTA comes out unswapped)

then, with that directory and the moleculekit source tree on PYTHONPATH (the tree supplies moleculekit.fileformats.utils, whose
ensure_type / cast_indices dcd.pyx imports, and readers.DCDread; the compiled module is registered as moleculekit.dcd below):

    PYTHONPATH=<scratch>:<moleculekit tree> python tests/golden/make_golden_dcd.py

Per case the npz holds: the file's bytes (synthesised by tests/dcd_cases.py, or written by the reference's DCDTrajectoryFile.write),
read_header(), the frame count, and for each (stride, atom_indices, frame) of dcd_cases.arg_sets what load_dcd returns and the step /
time / box fields of readers.DCDread's Trajectory.  For the written cases also the writer's inputs.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from tests import dcd_cases  # noqa: E402


def main():
    import dcd as refdcd                                   # the compiled reference module (see above)
    sys.modules["moleculekit.dcd"] = refdcd
    import moleculekit.readers as readers

    captured = {}
    readers.MolFactory.construct = staticmethod(lambda mol, traj, filename, frame: captured.__setitem__("traj", traj))
    out, names = {}, []
    tmp = tempfile.mkdtemp()

    def record(name, blob):
        path = os.path.join(tmp, name + ".dcd")
        with open(path, "wb") as fh:
            fh.write(blob)
        names.append(name)
        out[name + "/bytes"] = np.frombuffer(blob, np.uint8)
        with refdcd.DCDTrajectoryFile(path) as f:
            out[name + "/header"] = np.array(f.read_header(), np.float64)
            nframes = len(f)
            natoms = f.read(n_frames=1)[0].shape[1]
        out[name + "/nframes"] = np.int64(nframes)
        for i, (stride, atoms, frame) in enumerate(dcd_cases.arg_sets(natoms, nframes)):
            k = "%s/%s/" % (name, dcd_cases.arg_key(i))
            xyz, lengths, angles = refdcd.load_dcd(path, stride=stride, atom_indices=atoms, frame=frame)
            out[k + "xyz"] = xyz
            if lengths is not None:
                out[k + "lengths"], out[k + "angles"] = lengths, angles
            readers.DCDread(path, frame=frame, stride=stride, atom_indices=atoms)
            t = captured["traj"]
            assert np.array_equal(np.transpose(xyz, (1, 2, 0)).view(np.uint32), np.asarray(t.coords).view(np.uint32))
            out[k + "step"], out[k + "time"] = np.asarray(t.step), np.asarray(t.time)
        return path

    for name, c in dcd_cases.synthesised_cases().items():
        path = record(name, c["bytes"])
        got = refdcd.load_dcd(path)[0]
        assert np.array_equal(got.view(np.uint32), c["xyz"].view(np.uint32)), name     # the reference returns what was written
    for name, c in dcd_cases.written_cases().items():
        path = os.path.join(tmp, name + ".w.dcd")
        with refdcd.DCDTrajectoryFile(path, "w") as f:
            f.write(c["xyz"], cell_lengths=c["lengths"], cell_angles=c["angles"], istart=c["istart"], nsavc=c["nsavc"], delta=c["delta"])
        record(name, open(path, "rb").read())
        out[name + "/in_xyz"] = c["xyz"]
        if c["lengths"] is not None:
            out[name + "/in_lengths"], out[name + "/in_angles"] = c["lengths"], c["angles"]
        out[name + "/in_header"] = np.array([c["istart"], c["nsavc"], c["delta"]], np.float64)
    out["names"] = np.array(names)
    target = os.path.join(HERE, "dcd_cases.npz")
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
