"""CPU tier of the DCD path (moleculekit_amd/dcd.py; csrc/dcd_reader.h, csrc/dcd_kernels.h): the host parser and read loop through
libmkamd.so against what the reference's reader returns (tests/golden/dcd_cases.npz: the same float32 bits), the two device kernels
compiled for the host on tests/emu/emu_device.h against the same goldens and the reference-written files, the writer's file bytes,
damaged headers in a stand-alone program under AddressSanitizer and UBSan, and the host side of the Python API."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import dcd_cases
from tests import emu_dcd_build as emu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(GOLDEN, "dcd_cases.npz"))
NAMES = [str(n) for n in G["names"]]
WRITTEN = [n for n in NAMES if n.startswith("w_")]
OBLIQUE = {"cell_cos_oblique", "w_n63_f5"}            # angles through asin / sin of something other than 0: within one ulp (libm)
REMARK = slice(180, 260)                              # the creation-time remark of the writer's header


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("dcd")
    out = {}
    for n in NAMES:
        out[n] = str(d / (n + ".dcd"))
        with open(out[n], "wb") as fh:
            fh.write(G[n + "/bytes"].tobytes())
    return out


def ulp_close(a, b, dtype):
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    return bool(np.all(np.abs(a - b) <= np.spacing(np.abs(b))))


def check_cells(name, key, lengths, angles):
    if key + "lengths" not in G:
        assert lengths is None and angles is None
        return
    assert np.array_equal(bits(lengths), bits(G[key + "lengths"]))
    if name in OBLIQUE:
        assert ulp_close(angles, G[key + "angles"], np.float32)
    else:
        assert np.array_equal(bits(angles), bits(G[key + "angles"]))


@pytest.mark.parametrize("name", NAMES)
def test_host_read_equals_the_reference(files, name):
    from moleculekit_amd import dcd
    h = dcd.info(files[name])
    assert h["n_frames"] == int(G[name + "/nframes"])
    assert np.array_equal(np.array(dcd.read_header(files[name]), np.float64), G[name + "/header"])
    for i, (stride, atoms, frame) in enumerate(dcd_cases.arg_sets(h["n_atoms"], h["n_frames"])):
        key = "%s/%s/" % (name, dcd_cases.arg_key(i))
        xyz, lengths, angles = dcd.load_dcd(files[name], stride=stride, atom_indices=atoms, frame=frame)
        assert xyz.dtype == np.float32 and xyz.shape == G[key + "xyz"].shape
        assert np.array_equal(bits(xyz), bits(G[key + "xyz"]))
        check_cells(name, key, lengths, angles)
        t = dcd.DCDread(files[name], frame=frame, stride=stride, atom_indices=atoms)
        assert np.array_equal(bits(t.coords), bits(np.transpose(G[key + "xyz"], (1, 2, 0))))
        assert t.step.dtype == G[key + "step"].dtype and np.array_equal(t.step, G[key + "step"])      # (strided twice, like the reference)
        assert t.time.dtype == G[key + "time"].dtype and np.array_equal(t.time, G[key + "time"])
        assert (t.box is None) == (key + "lengths" not in G)
        if t.box is not None:
            assert t.box.shape == (3, xyz.shape[0]) and t.boxangles.shape == (3, xyz.shape[0])


def test_the_truncated_file_has_one_frame_fewer(files):
    from moleculekit_amd import dcd
    assert dcd.info(files["truncated"])["n_frames"] == 3 and dcd.load_dcd(files["truncated"])[0].shape == (3, 9, 3)


def test_a_stride_past_the_end_gives_one_frame(files):
    from moleculekit_amd import dcd
    assert dcd.load_dcd(files["plain"], stride=7)[0].shape == (1, 9, 3)
    assert dcd.load_dcd(files["plain"], stride=7, frame=2)[0].shape == (1, 9, 3)                       # frame overrides stride


def test_atom_indices_must_be_unique_integers_in_range(files):
    from moleculekit_amd import dcd
    for bad in ([1, 1], [0.5, 1.0], [9], [-1]):
        with pytest.raises(ValueError):
            dcd.load_dcd(files["plain"], atom_indices=bad)
    with pytest.raises(TypeError):
        dcd.load_dcd(b"x.dcd")


def test_opposite_endian_4d_is_refused_with_its_reason(tmp_path):
    from moleculekit_amd import dcd
    p = str(tmp_path / "big4.dcd")
    with open(p, "wb") as fh:
        fh.write(dcd_cases.refused_big_four())
    with pytest.raises(ValueError, match="opposite-endian DCD file with a 4th dimension"):
        dcd.load_dcd(p)


# ---- the kernels on the host emulation ----
def selections(N):
    return [None, np.arange(N, dtype=np.int32)[::-1].copy(), np.arange(0, N, 3, dtype=np.int32), np.array([N // 2], np.int32)]


def frame_lists(F):
    return [np.arange(F), np.arange(F)[::-1].copy()] + ([np.array([3, 0, 3, 1])] if F >= 4 else [])


def emu_decode(path, frames, atoms, scale=1.0):
    from moleculekit_amd import dcd
    h = dcd.info(path)
    raw_all = np.fromfile(path, np.uint8)
    frame0 = None
    if h["n_fixed"]:
        desc, lo, hi, _ = dcd.chunk_desc(path, [0])
        ident = np.arange(h["n_atoms"], dtype=np.int32)
        frame0, st = emu.decode(raw_all[lo:hi], desc, ident, ident, h["n_atoms"])
        assert not st.any()
        frame0 = np.ascontiguousarray(frame0[0])
    desc, lo, hi, cell = dcd.chunk_desc(path, frames)
    sel, src = dcd.source_table(path, atoms, h["n_atoms"])
    xyz, st = emu.decode(raw_all[lo:hi], desc, sel, src, h["n_atoms"], frame0=frame0, scale=scale)
    assert not st.any()
    return xyz


@pytest.mark.parametrize("name", NAMES)
def test_emulated_decode_equals_the_reference(files, name):
    full = G[name + "/a0/xyz"]
    F, N = full.shape[:2]
    for atoms in selections(N):
        for fr in frame_lists(F):
            want = full[fr] if atoms is None else full[fr][:, atoms]
            got = emu_decode(files[name], fr, atoms)
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want))


def test_emulated_decode_scales_only_when_asked(files):
    full = G["w_n9_f4/a0/xyz"]
    got = emu_decode(files["w_n9_f4"], np.arange(4), None, scale=10.0)
    with np.errstate(invalid="ignore"):
        want = full * np.float32(10)
    finite = np.isfinite(full)
    assert np.array_equal(bits(got)[finite], bits(want)[finite]) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(bits(emu_decode(files["w_n9_f4"], np.arange(4), None, scale=1.0)), bits(full))   # NaN payloads, -0: untouched


def test_emulated_decode_guards_the_byte_count(files):
    """A descriptor that reaches past the bytes the kernel is told it has: status 1 for that frame, nothing of it stored."""
    from moleculekit_amd import dcd
    p = files["w_n65_f4_zero"]
    raw_all = np.fromfile(p, np.uint8)
    desc, lo, hi, _ = dcd.chunk_desc(p, np.arange(4))
    sel, src = dcd.source_table(p, None, 65)
    d = desc.copy().view(dcd.DESC_DTYPE).reshape(-1)
    limit = int(d["z_off"][2]) + 4 * 65 - 4                              # frame 2's z plane ends 4 bytes behind it; frame 3 lies beyond
    xyz, st = emu.decode(raw_all[lo:hi], desc, sel, src, 65, n_bytes=limit)
    assert st.tolist() == [0, 0, 1, 1]
    assert np.array_equal(bits(xyz[:2]), bits(G["w_n65_f4_zero/a0/xyz"][:2]))
    assert (xyz[2:].view(np.uint8) == emu.POISON).all()
    d["y_off"][1] += 2                                                   # a plane that is not 4-byte aligned
    assert emu.decode(raw_all[lo:hi], d.view(np.uint8).reshape(-1, 32), sel, src, 65)[1].tolist() == [0, 1, 0, 0]


def written_inputs(name):
    L = G[name + "/in_lengths"] if name + "/in_lengths" in G else None
    A = G[name + "/in_angles"] if name + "/in_angles" in G else None
    istart, nsavc, delta = G[name + "/in_header"]
    return G[name + "/in_xyz"], L, A, int(istart), int(nsavc), float(delta)


def check_cell_doubles(name, ours, theirs):
    """Frame images: every byte equal, but the cosines of oblique cells within one float64 ulp."""
    if name not in OBLIQUE:
        assert np.array_equal(ours, theirs)
        return
    xyz = G[name + "/in_xyz"]
    F, N = xyz.shape[:2]
    a, b = ours.reshape(F, -1), theirs.reshape(F, -1)
    assert a.shape == b.shape and np.array_equal(a[:, 52:], b[:, 52:]) and np.array_equal(a[:, :4], b[:, :4])
    assert ulp_close(a[:, 4:52].copy().view(np.float64), b[:, 4:52].copy().view(np.float64), np.float64)


@pytest.mark.parametrize("name", WRITTEN)
def test_emulated_encode_and_header_equal_the_reference_written_file(name):
    from moleculekit_amd import dcd
    xyz, L, A, istart, nsavc, delta = written_inputs(name)
    theirs = G[name + "/bytes"]
    image = emu.encode(xyz, dcd.cell_records(L, A, len(xyz)))
    assert len(image) == len(theirs) - dcd.HEADER_BYTES                 # (poisoned first and exactly as long: every byte was written)
    check_cell_doubles(name, image, theirs[dcd.HEADER_BYTES:])
    head = np.frombuffer(dcd.file_header(xyz.shape[1], len(xyz), istart, nsavc, delta, L is not None), np.uint8)
    keep = np.ones(dcd.HEADER_BYTES, bool)
    keep[REMARK] = False
    assert np.array_equal(head[keep], theirs[:dcd.HEADER_BYTES][keep])
    remark = head[REMARK].tobytes()
    assert remark.startswith(b"REMARKS Created ") and theirs[REMARK].tobytes().startswith(b"REMARKS Created ")
    assert remark.rstrip(b"\0") == remark[:len(remark.rstrip(b"\0"))] and b"\0" not in remark.rstrip(b"\0")   # zero-padded behind the text


def test_zero_cell_is_written_with_unit_cosines():
    from moleculekit_amd import dcd
    rec = dcd.cell_records(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32), 2)
    assert rec.tolist() == [[0.0, 1.0, 0.0, 1.0, 1.0, 0.0]] * 2
    assert dcd.cell_records(None, None, 2) is None
    with pytest.raises(ValueError):
        dcd.cell_records(np.zeros((2, 3)), None, 2)


# ---- damaged headers, in a sanitized program of its own ----
def damage_file(tmp_path, spec, patches):
    rng = np.random.default_rng(5)
    N, F = spec["N"], spec["F"]
    cell = dcd_cases.cos_cell((30, 40, 50), (90, 90, 90), F) if spec.get("cell") else None
    blob = bytearray(dcd_cases.synth_dcd(dcd_cases.coords(rng, F, N), cell=cell, fixed=spec.get("fixed")))
    for off, val in patches:
        blob[off:off + 4] = int(val).to_bytes(4, "little", signed=True)
    return bytes(blob)


def test_damaged_headers_are_refused_under_sanitizers(tmp_path):
    from moleculekit_amd import dcd
    spec = json.load(open(os.path.join(GOLDEN, "dcd_damage_cases.json")))
    exe = emu.build_main()
    paths = []
    for c in spec["cases"]:
        paths.append(str(tmp_path / (c["name"] + ".dcd")))
        with open(paths[-1], "wb") as fh:
            fh.write(damage_file(tmp_path, spec["bases"][c["base"]], c["patches"]))
    r = subprocess.run([exe, "file"] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(paths)
    for c, line, p in zip(spec["cases"], lines, paths):
        assert " status=1 " in line and c["message"] in line, (c["name"], line)
        with pytest.raises(ValueError, match=c["message"].replace(".", r"\.")):        # the same through libmkamd.so
            dcd.load_dcd(p)
    for base in spec["bases"].values():                                               # the undamaged bases read clean
        good = str(tmp_path / "good.dcd")
        with open(good, "wb") as fh:
            fh.write(damage_file(tmp_path, base, []))
        r = subprocess.run([exe, "file", good], capture_output=True, text=True)
        assert r.returncode == 0 and " status=0 frames=3 " in r.stdout, r.stdout + r.stderr[-2000:]


@pytest.mark.parametrize("base", ["plain", "fixed", "cell"])
def test_every_truncation_is_refused_or_shorter_under_sanitizers(tmp_path, base):
    spec = json.load(open(os.path.join(GOLDEN, "dcd_damage_cases.json")))["bases"][base]
    blob = damage_file(tmp_path, spec, [])
    p = str(tmp_path / "whole.dcd")
    with open(p, "wb") as fh:
        fh.write(blob)
    r = subprocess.run([emu.build_main(), "truncate", p], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(blob) + 1
    N, F, nfix = spec["N"], spec["F"], len(spec.get("fixed", []))
    extra = 56 if spec.get("cell") else 0
    first_off = 276 + ((N - nfix) * 4 + 8 if nfix else 0)
    first, later = extra + 3 * (4 * N + 8), extra + 3 * (4 * (N - nfix) + 8)
    for n, line in enumerate(lines):
        want = 0 if n < first_off + first else 1 + (n - first_off - first) // later
        assert line == "len=%d status=%d frames=%d" % (n, 0 if want else 1, want), line
    assert lines[-1].endswith("frames=%d" % F)


# ---- the Python side that needs no GPU ----
class Mol:
    def __init__(self, F=3, N=4, **kw):
        self.coords = np.zeros((N, 3, F), np.float32)
        self.box = np.zeros((3, F), np.float32)
        self.boxangles = np.zeros((3, F), np.float32)
        self.__dict__.update(kw)


def test_dcdwrite_arithmetic_on_duck_typed_molecules():
    from moleculekit_amd import dcd
    m = Mol(step=np.array([1000, 1250, 1500]), fstep=0.0001)
    _, box, ang, istart, nsavc, delta = dcd._dcdwrite_arrays(m)
    assert (istart, nsavc) == (1000, 250) and delta == 0.0001 * 1000 / 250 / 0.04888821
    assert box.shape == (3, 3) and not box.any() and not ang.any()
    big = Mol(step=np.array([2 ** 33, 2 ** 33 + 100, 2 ** 33 + 200]), fstep=0.0001)            # does not fit an int32: renumbered
    _, _, _, istart, nsavc, delta = dcd._dcdwrite_arrays(big)
    assert (istart, nsavc) == (2 ** 33 // 100, 1) and delta == 0.0001 * 1000 / 100 / 0.04888821 * 100
    huge = Mol(step=np.array([2 ** 62, 2 ** 62 + 2, 2 ** 62 + 4]), fstep=0.0001)               # still too large: start from 1
    assert dcd._dcdwrite_arrays(huge)[3:5] == (1, 1)
    assert dcd._dcdwrite_arrays(Mol(step=np.array([5, 10, 15])))[3:] == (0, 1, 1.0)            # no fstep
    assert dcd._dcdwrite_arrays(Mol(step=np.array([5]), fstep=0.1))[3:] == (0, 1, 1.0)         # one frame: no second step
    boxed = Mol(step=np.array([0, 1, 2]), fstep=0.1)
    boxed.box = np.full((3, 3), 50, np.float32)
    boxed.boxangles = np.full((3, 3), 90, np.float32)
    _, box, ang, _, _, _ = dcd._dcdwrite_arrays(boxed)
    assert box.shape == (3, 3) and (box == 50).all() and (ang == 90).all()
    with pytest.raises(OverflowError):
        dcd.file_header(4, 3, istart=2 ** 31)


@pytest.fixture
def stub_moleculekit(monkeypatch):
    pkg, readers, writers = types.ModuleType("moleculekit"), types.ModuleType("moleculekit.readers"), types.ModuleType("moleculekit.writers")

    def DCDread(filename, frame=None, topoloc=None, stride=None, atom_indices=None):
        return ("reference read", filename)

    def DCDwrite(mol, filename):
        return ("reference write", filename)

    class Trajectory:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    class MolFactory:
        @staticmethod
        def construct(topo, traj, filename, frame):
            return ("constructed", traj, filename, frame)

    readers.DCDread, readers._TRAJECTORY_READERS = DCDread, {"xtc": lambda *a, **k: None, "dcd": DCDread}
    readers.Trajectory, readers.MolFactory = Trajectory, MolFactory
    writers.DCDwrite, writers._WRITERS = DCDwrite, {"pdb": lambda mol, filename: None, "dcd": DCDwrite}
    pkg.readers, pkg.writers = readers, writers
    for name, mod in (("moleculekit", pkg), ("moleculekit.readers", readers), ("moleculekit.writers", writers)):
        monkeypatch.setitem(sys.modules, name, mod)
    return readers, writers


def test_install_swaps_reader_and_writer_and_uninstall_restores(stub_moleculekit, monkeypatch, files):
    from moleculekit_amd import dcd
    rd, wr = stub_moleculekit
    calls = []
    monkeypatch.setattr(dcd, "DCDwrite", lambda mol, filename, ctx=None: calls.append((mol, filename)))
    read0, write0, xtc0, pdb0 = rd.DCDread, wr.DCDwrite, rd._TRAJECTORY_READERS["xtc"], wr._WRITERS["pdb"]
    assert dcd.install() == (read0, write0)
    assert dcd.install() == (read0, write0)                              # idempotent
    assert rd.DCDread is not read0 and rd._TRAJECTORY_READERS["dcd"] is rd.DCDread and rd._TRAJECTORY_READERS["xtc"] is xtc0
    assert wr.DCDwrite is not write0 and wr._WRITERS["dcd"] is wr.DCDwrite and wr._WRITERS["pdb"] is pdb0
    tag, traj, filename, frame = rd._TRAJECTORY_READERS["dcd"](files["w_n9_f4"], frame=2)      # as Molecule.read calls it
    assert tag == "constructed" and filename == files["w_n9_f4"] and frame == 2
    assert np.array_equal(bits(traj.coords), bits(np.transpose(G["w_n9_f4/a0/xyz"][2:3], (1, 2, 0)))) and traj.step.tolist() == [1000]
    wr._WRITERS["dcd"]("mol", "a.dcd")
    assert calls == [("mol", "a.dcd")]
    dcd.uninstall()
    assert rd.DCDread is read0 and rd._TRAJECTORY_READERS["dcd"] is read0 and wr.DCDwrite is write0 and wr._WRITERS["dcd"] is write0
    assert rd.DCDread("x.dcd") == ("reference read", "x.dcd")
    dcd.uninstall()                                                      # a second time: nothing to undo
    assert wr.DCDwrite is write0
