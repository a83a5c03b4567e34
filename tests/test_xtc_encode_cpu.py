"""CPU tier of the device XTC writer (csrc/xtc_encode.h): its kernels, launched by the product's own launch plan, on the host SIMT
emulation (tests/emu/emu_xtc_encode.cpp).  The bar is the reference writer's file, byte for byte: the committed
tests/golden/xtc_reference/<name>.xtc for the named cases, the reference codec itself (built on demand from the reference tree) for a
random sweep.  A frame outside what the device path takes gets status 2 and no bytes; nothing else may differ.

Also here: the committed inputs of the GPU tier against their generator, what the walk reached, hostile values, the same kernels in a
program of its own under AddressSanitizer and UBSan, and the host side of the Python API (``XTCwrite``'s defaults, ``install()``)."""
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import emu_xtc_encode_build as emu
from tests import xtc_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIX = os.path.join(GOLDEN, "xtc_reference")
sys.path.insert(0, GOLDEN)
from make_golden_xtc_reference import fixture_cases  # noqa: E402

WHOLE = ["water", "water_one_frame", "chain_001", "chain_005_neg", "close_far", "flag_free", "precisions", "per_axis_x", "triple64",
         "atoms1", "atoms2", "atoms3", "atoms9", "atoms10", "atoms11"]
REFUSED = ["triple65", "zigzag"]
PARTIAL = {"smallidx_ends": [0, 0, 0, 0, 2]}        # frame 4: header index 64
_CASES, _OUT = {}, {}


def case(name):
    if not _CASES:
        _CASES.update((c.name, c) for c in fixture_cases())
    return _CASES[name]


def encoded(name):
    """The emulated kernels' output for a named case (computed once, shared, left unchanged)."""
    if name not in _OUT:
        c = case(name)
        _OUT[name] = emu.encode(c.coords, c.box, precision=c.precision)
    return _OUT[name]


def fixture_bytes(name):
    with open(os.path.join(FIX, name + ".xtc"), "rb") as f:
        return f.read()


def split_records(buf):
    """A file's records and what their headers say about the device path: [(bytes, refused by the header rule)]."""
    out, p = [], 0
    while p < len(buf):
        magic, n = struct.unpack(">ii", buf[p:p + 8])
        assert magic == 1995
        if n <= 9:
            q, refused = p + 56 + 12 * n, False
        else:
            lo = struct.unpack(">iii", buf[p + 60:p + 72])
            hi = struct.unpack(">iii", buf[p + 72:p + 84])
            smallidx, nbytes = struct.unpack(">ii", buf[p + 84:p + 92])
            size = [h - l + 1 for l, h in zip(lo, hi)]
            triple = 0 if max(size) > 0xffffff else (size[0] * size[1] * size[2]).bit_length()
            refused = triple > 64 or smallidx + 8 > 64
            q = p + 92 + (nbytes + 3) // 4 * 4
        out.append((buf[p:q], refused))
        p = q
    return out


def test_all_named_cases_are_listed():
    assert sorted(WHOLE + REFUSED + list(PARTIAL)) == sorted(c.name for c in fixture_cases())


@pytest.mark.parametrize("name", WHOLE)
def test_named_case_gives_the_reference_writers_bytes(name):
    out = encoded(name)
    assert out["status"].tolist() == [0] * len(out["status"])
    got, want = emu.records(out), fixture_bytes(name)
    assert len(got) == len(want) and got == want
    recs = split_records(want)
    assert out["offsets"].tolist() == np.concatenate([[0], np.cumsum([len(r) for r, _ in recs])]).tolist()
    assert not any(refused for _, refused in recs)


@pytest.mark.parametrize("name", REFUSED)
def test_refused_case_has_status_2_everywhere_and_an_untouched_image(name):
    out = encoded(name)
    assert out["status"].tolist() == [2] * len(out["status"])
    assert out["offsets"].tolist() == [0] * (len(out["status"]) + 1)
    assert emu.records(out) == b""                                    # (records() checks the poison behind offsets[-1] = 0)
    assert all(refused for _, refused in split_records(fixture_bytes(name)))


def test_smallidx_ends_first_four_records_are_a_prefix_of_the_file():
    out = encoded("smallidx_ends")
    assert out["status"].tolist() == PARTIAL["smallidx_ends"]
    recs = split_records(fixture_bytes("smallidx_ends"))
    assert [refused for _, refused in recs] == [False, False, False, False, True]
    assert struct.unpack(">i", recs[4][0][84:88])[0] == 64
    got = emu.records(out)
    assert got == b"".join(r for r, _ in recs[:4]) and fixture_bytes("smallidx_ends").startswith(got)
    assert out["offsets"][4] == out["offsets"][5] == len(got)


def test_committed_inputs_are_the_generators_arrays():
    """tests/golden/xtc_encode_inputs.npz (the GPU tier's inputs) holds what ``fixture_cases()`` generates, bit for bit -- so the bytes
    checked above are the bytes the GPU tier asks for."""
    with np.load(os.path.join(GOLDEN, "xtc_encode_inputs.npz")) as z:
        names = sorted({k.split("__")[0] for k in z.files})
        assert names == sorted(c.name for c in fixture_cases())
        for c in fixture_cases():
            F = c.coords.shape[0]
            assert z[c.name + "__coords"].dtype == np.float32 and z[c.name + "__coords"].tobytes() == np.ascontiguousarray(c.coords, np.float32).tobytes()
            assert z[c.name + "__box"].tobytes() == np.ascontiguousarray(c.box, np.float32).tobytes()
            assert z[c.name + "__precision"].tobytes() == np.broadcast_to(np.asarray(c.precision, np.float32), (F,)).tobytes()


def test_reach_of_the_named_cases():
    """From the plan kernel's group records: groups of 8 small atoms, a swap, ``smallidx`` 9 and steps up and down, flagged and
    unflagged groups, a walk across more than one LDS window."""
    total = dict(max_small=0, swaps=0, idx_lo=99, idx_hi=0, up=0, down=0, flagged=0, unflagged=0, windows=0)
    for name in WHOLE + list(PARTIAL):
        r = emu.reach(encoded(name))
        for k in ("max_small", "idx_hi", "windows"):
            total[k] = max(total[k], r[k])
        total["idx_lo"] = min(total["idx_lo"], r["idx_lo"])
        for k in ("swaps", "up", "down", "flagged", "unflagged"):
            total[k] += r[k]
    print(total)
    assert total["max_small"] == 8 and total["swaps"] > 0 and total["idx_lo"] == 9
    assert total["up"] > 0 and total["down"] > 0 and total["flagged"] > 0 and total["unflagged"] > 0
    assert total["windows"] > 1


def test_group_records_tile_the_stream():
    """Every group starts where the one before ends, and the last one ends at the stream's bit count."""
    out = encoded("water")
    for f in range(len(out["status"])):
        p = out["plan"][f]
        n = int(p["ngroups"])
        g = out["groups"][f, :n].astype(np.int64)
        meta = g[:, 2]
        sidx, ns, fv = meta & 0xff, (meta >> 8) & 15, (meta >> 16) & 0xff
        full = int(p["bitsize"]) or int(p["fieldbits"].sum())
        ends = g[:, 0] + full + np.where(fv == 0xff, 1, 6) + ns * sidx
        assert g[0, 0] == 0 and np.array_equal(ends[:-1], g[1:, 0]) and ends[-1] == p["nbits"]
        assert np.array_equal(g[1:, 1], g[:-1, 1] + 1 + ns[:-1]) and g[-1, 1] + 1 + ns[-1] == out["groups"].shape[1]


HOSTILE = {"nan": np.nan, "plus_inf": np.inf, "minus_inf": -np.inf, "1e30": 1e30}


def hostile_frames(kind):
    """Three frames of 30 water atoms; the middle one made hostile."""
    c = xtc_cases.water(np.random.default_rng(77), nmol=10, F=3)
    x = c.coords.copy()
    if kind == "span":                                               # +-2.1e9 quanta: each value fits an int, the range does not
        x[1, 3, 0], x[1, 7, 0] = 2.1e6, -2.1e6
    else:
        x[1, 5, 1] = HOSTILE[kind]
    return x, c.box


@pytest.mark.parametrize("kind", sorted(HOSTILE) + ["span"])
def test_hostile_values_are_refused_and_leave_the_other_frames_alone(kind):
    x, box = hostile_frames(kind)
    t, s = np.array([0.5, 1.5, 2.5], np.float32), np.array([10, 20, 30], np.int32)
    out = emu.encode(x, box, time=t, step=s)
    assert out["status"].tolist() == [0, 2, 0]
    clean = emu.encode(x[[0, 2]], box[[0, 2]], time=t[[0, 2]], step=s[[0, 2]])
    assert clean["status"].tolist() == [0, 0]
    assert emu.records(out) == emu.records(clean) and len(emu.records(clean)) > 2 * 92
    assert out["offsets"].tolist() == [0, clean["offsets"][1], clean["offsets"][1], clean["offsets"][2]]


def test_precision_of_zero_or_less_is_written_as_1000():
    c = case("water_one_frame")
    for p in (0.0, -5.0):
        out = emu.encode(c.coords, c.box, precision=p)
        assert out["status"].tolist() == [0] and emu.records(out) == fixture_bytes("water_one_frame")


def test_input_scale_is_one_float32_product():
    """Angstrom input: ``x * in_scale`` on the device is the float32 product the reference's ``XTCwrite`` forms on the host."""
    c = case("close_far")
    ang = (c.coords * np.float32(10.0)).astype(np.float32)
    nm = (ang * np.float32(0.1)).astype(np.float32)
    assert not np.array_equal(nm, c.coords)                          # (the round trip is not the identity: the product matters)
    a, b = emu.encode(ang, c.box, in_scale=np.float32(0.1)), emu.encode(nm, c.box)
    assert a["status"].tolist() == [0, 0] and emu.records(a) == emu.records(b)
    few = case("atoms3")                                             # plain floats: the scaled values themselves
    ang = (few.coords * np.float32(10.0)).astype(np.float32)
    assert emu.records(emu.encode(ang, few.box, in_scale=np.float32(0.1))) == emu.records(emu.encode((ang * np.float32(0.1)).astype(np.float32), few.box))


def test_frames_of_two_million_atoms_are_refused_whole():
    N = 1 << 21
    out = emu.encode(np.zeros((2, N, 3), np.float32))
    assert out["status"].tolist() == [2, 2] and out["offsets"].tolist() == [0, 0, 0] and emu.records(out) == b""


def write_case_file(path, coords, box, time, step, precision, status, image, in_scale=1.0):
    F, N = coords.shape[:2]
    with open(path, "wb") as f:
        f.write(struct.pack("<qqf", F, N, in_scale))
        for a, dt in ((emu.per_frame(precision, F, np.float32), "<f4"), (box, "<f4"), (time, "<f4"), (step, "<i4"), (coords, "<f4"), (status, "<i4")):
            f.write(np.ascontiguousarray(a).astype(dt).tobytes())
        f.write(struct.pack("<q", len(image)) + image)


def test_kernels_under_address_and_ub_sanitizers(tmp_path):
    """The same emulated kernels in a program of its own built with -fsanitize=address,undefined, on the named cases and the hostile
    inputs, every buffer a heap block of exactly the promised size (tests/emu/xtc_encode_main.cpp).  Nothing is preloaded."""
    exe = emu.build_main()
    files = []
    for c in fixture_cases():
        F = c.coords.shape[0]
        status = PARTIAL.get(c.name, [2 if c.name in REFUSED else 0] * F)
        recs = split_records(fixture_bytes(c.name))
        image = b"".join(r for (r, _), st in zip(recs, status) if st == 0)
        files.append(str(tmp_path / (c.name + ".bin")))
        write_case_file(files[-1], c.coords, c.box, np.arange(F), np.arange(F), c.precision, status, image)
    for kind in sorted(HOSTILE) + ["span"]:
        x, box = hostile_frames(kind)
        image = emu.records(emu.encode(x[[0, 2]], box[[0, 2]], time=[0, 2], step=[0, 2]))
        files.append(str(tmp_path / ("hostile_" + kind + ".bin")))
        write_case_file(files[-1], x, box, np.arange(3), np.arange(3), 1000.0, [0, 2, 0], image)
    env = dict(os.environ)                                          # as inherited, but for the sanitizers' own options
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert '"failed": 0' in r.stdout and '"cases": %d' % len(files) in r.stdout


def test_random_sweep_against_the_reference_writer(tmp_path):
    """200 small files of ``xtc_cases.random_case``: every frame either equals the reference's record or has status 2, and status 2
    occurs exactly where the reference-written header says so (a triple of more than 64 bits, or ``smallidx + 8 > 64``)."""
    from oracle import xtcref
    if not xtcref.available():
        pytest.skip("neither the reference tree nor oracle/_ref/libxtcref.so is there")
    rng = np.random.default_rng(2024)
    whole = frames = frames_ok = 0
    for i in range(200):
        c = xtc_cases.random_case(rng, i)
        fn = xtc_cases.write(c, tmp_path / "sweep.xtc")
        with open(fn, "rb") as f:
            recs = split_records(f.read())
        out = emu.encode(c.coords, c.box, precision=c.precision)
        assert len(recs) == len(out["status"]), c.name
        assert out["status"].tolist() == [2 if refused else 0 for _, refused in recs], c.name
        assert emu.records(out) == b"".join(r for r, refused in recs if not refused), c.name
        frames += len(recs)
        frames_ok += sum(not refused for _, refused in recs)
        whole += not any(refused for _, refused in recs)
    print(f"{whole} of 200 files and {frames_ok} of {frames} frames encoded")
    assert whole >= 170


# ---- the Python API on the host ----
def test_xtcwrite_arrays_follow_the_reference_rules():
    from moleculekit_amd import xtc
    rng = np.random.default_rng(5)
    coords = rng.normal(size=(12, 3, 4)).astype(np.float32)
    # a molecule without box, step or time: zeros everywhere
    c, box, time, step = xtc._xtcwrite_arrays(types.SimpleNamespace(coords=coords, numFrames=4))
    assert c is coords or np.array_equal(c, coords)
    assert box.shape == (3, 3, 4) and box.dtype == np.float32 and not box.any()
    assert time.dtype == np.float32 and time.tolist() == [0, 0, 0, 0] and step.dtype == np.uint32 and step.tolist() == [0, 0, 0, 0]
    # one frame's box vectors in Angstrom are repeated for every frame, in nm (a float32 product); fs -> ps
    bv = np.diag([30.0, 40.0, 50.0]).astype(np.float32).reshape(3, 3, 1)
    mol = types.SimpleNamespace(coords=coords, numFrames=4, box=np.zeros((3, 1)), boxvectors=bv, step=np.array([100, 200, 300, 400]),
                                time=np.array([2000.0, 4000.0, 6000.0, 8000.0]), fstep=0.002)
    c, box, time, step = xtc._xtcwrite_arrays(mol)
    assert box.shape == (3, 3, 4) and all(np.array_equal(box[:, :, f], (bv[:, :, 0] * 0.1).astype(np.float32)) for f in range(4))
    assert box.dtype == np.float32 and box[0, 0, 0] == np.float32(30.0) * np.float32(0.1)
    assert time.tolist() == [2.0, 4.0, 6.0, 8.0] and step.tolist() == [100, 200, 300, 400]
    # steps beyond 32 bits are renumbered from 1
    mol.step = np.array([1, 2, 3, 2 ** 33], dtype=np.int64)
    assert xtc._xtcwrite_arrays(mol)[3].tolist() == [1, 2, 3, 4]
    # times float32 cannot hold are rebuilt from fstep and the step stride: (time - (step0 - stride) * (fstep / stride / 1e-6)) / 1e3
    mol.step = np.array([100, 200, 300, 400])
    mol.time = np.array([1e3, 2e3, 3e3, 123456789012.0])
    want = ((mol.time - (100 - 100) * ((0.002 / 100) / 1e-6)) / 1e3).astype(np.float32)
    assert np.array_equal(xtc._xtcwrite_arrays(mol)[2], want)
    mol.step = np.array([7, 7, 7, 7])
    with pytest.raises(AssertionError):
        xtc._xtcwrite_arrays(mol)


def test_step_bits_are_the_unsigned_values():
    from moleculekit_amd import xtc
    assert xtc._step_i32(np.array([0, 5, 2 ** 31, 2 ** 32 - 1], np.uint32)).tolist() == [0, 5, -2 ** 31, -1]
    assert xtc._index_side_file(os.path.join("a", "b", "t.xtc")) == os.path.join("a", "b", ".t.xtc")


@pytest.fixture
def stub_writers(monkeypatch):
    pkg, writers = types.ModuleType("moleculekit"), types.ModuleType("moleculekit.writers")

    def XTCwrite(mol, filename):
        return ("reference", filename)

    writers.XTCwrite = XTCwrite
    writers._WRITERS = {"pdb": lambda mol, filename: None, "xtc": XTCwrite}
    pkg.writers = writers
    monkeypatch.setitem(sys.modules, "moleculekit", pkg)
    monkeypatch.setitem(sys.modules, "moleculekit.writers", writers)
    return writers


def test_install_swaps_the_writer_and_uninstall_restores(stub_writers, monkeypatch):
    from moleculekit_amd import xtc
    calls = []
    monkeypatch.setattr(xtc, "XTCwrite", lambda mol, filename, ctx=None: calls.append((mol, filename)))
    w = stub_writers
    original, pdb = w.XTCwrite, w._WRITERS["pdb"]
    assert xtc.install() is original
    assert xtc.install() is original                                   # idempotent
    assert w.XTCwrite is not original and w._WRITERS["xtc"] is w.XTCwrite and w._WRITERS["pdb"] is pdb
    w._WRITERS["xtc"]("mol", "a.xtc")                                  # as Molecule.write calls it
    w.XTCwrite("mol2", "b.xtc")
    assert calls == [("mol", "a.xtc"), ("mol2", "b.xtc")]
    xtc.uninstall()
    assert w.XTCwrite is original and w._WRITERS["xtc"] is original and w._WRITERS["pdb"] is pdb
    assert w.XTCwrite("mol", "c.xtc") == ("reference", "c.xtc")
    xtc.uninstall()                                                    # a second time: nothing to undo
    assert w.XTCwrite is original
