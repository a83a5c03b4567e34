"""CPU tier: the run cursor of the candidate traversal and the cover fold once per channel (round 9) on the
host emulation of the product's kernels.

1. The mapping alone: tables of 64 run lengths walked chunk by chunk through the product's cand_issue (tests/emu/emu_cand_cursor.cpp);
   (valid, record, code) of every lane of every chunk against the concatenated runs indexed by the candidate number, for a whole
   traversal (stride 1) and for a team's dealing (stride 4, first chunk 0..3), one chunk at a time and four issued together.  A
   team's wave keeps the per-chunk search of the runs: the strided walks run both, the search and the cursor.
2. The kernel, fold and cursor together: the comparisons of tests/test_emu_cover_fold.py with the plain call, bit for bit, on tiles whose
   channels hold only covered classes, on tiles where a 1.1 A atom (the uncovered class) sits in every channel below 7, and with both
   kinds of channel in one tile."""
import numpy as np
import pytest

from tests import emu_build as E
from tests import emu_cand_cursor_build as CC
from tests import emu_cover_fold_build as EC
from tests.synth import synth_sigmas
from tests.test_emu_cover_fold import NV, ragged

OFF = CC.SURV_OFF_BITS


def table(**runs):
    t = np.zeros(64, np.int64)
    for k, v in runs.items():
        t[int(k[1:])] = v
    return t


def _tables():
    rng = np.random.default_rng(9)
    T = {}
    T["all_empty"] = np.zeros(64, np.int64)
    T["single_run_lane0"] = table(l0=300)
    T["single_run_lane37"] = table(l37=65)
    T["single_run_of_one"] = table(l63=1)
    T["zeros_front_middle_end"] = np.concatenate([np.zeros(7), [110, 95], np.zeros(20), [1, 130, 64], np.zeros(5), [63, 65], np.zeros(25)]).astype(np.int64)
    T["edge_lengths"] = table(l0=1, l1=63, l2=64, l3=65, l4=128, l5=1, l6=1, l7=1, l8=64, l9=64)
    T["not_codable"] = table(l2=1, l3=1025, l5=63, l9=1025, l10=64, l40=128, l63=1)          # 1 025 > 1 << SURV_OFF_BITS
    T["nine_columns"] = table(l0=110, l1=97, l2=121, l3=108, l4=0, l5=113, l6=102, l7=117, l8=109)
    full = rng.integers(0, 40, 64); full[63] = 17                                              # 63 cell runs + lane 63's spill run
    full[:63][full[:63] == 0] = 1
    T["63_runs_and_the_spill_run"] = full
    T["63_runs_of_one_and_the_spill_run"] = np.ones(64, np.int64)
    T["short_runs_with_gaps"] = np.where(rng.random(64) < 0.5, rng.integers(1, 4, 64), 0)     # several runs inside one chunk
    T["spill_run_alone_behind_empties"] = table(l63=200)
    return T


TABLES = _tables()


def layout(length, seed=1):
    """the runs laid out in a record buffer in shuffled order with gaps -> (r0 [64], the class words of the records)"""
    rng = np.random.default_rng(seed)
    r0 = np.zeros(64, np.int64)
    pos = 3
    for j in rng.permutation(64):
        r0[j] = pos
        pos += int(length[j]) + int(rng.integers(0, 5))
    r = np.arange(pos + 64, dtype=np.uint64)
    return r0, ((r * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xffffffff)).astype(np.uint32)


def restated(r0, length):
    """the concatenated runs: candidate number n -> (record index, run, offset inside the run)"""
    rec = np.concatenate([r0[j] + np.arange(length[j]) for j in range(64)] + [np.zeros(0, np.int64)])
    run = np.concatenate([np.full(length[j], j) for j in range(64)] + [np.zeros(0, np.int64)])
    off = np.concatenate([np.arange(length[j]) for j in range(64)] + [np.zeros(0, np.int64)])
    return rec.astype(np.int64), run.astype(np.int64), off.astype(np.int64)


WALKS = [(0, 1, 1), (0, 1, 4)] + [(f, 4, b) for f in range(4) for b in (1, 4)]


@pytest.mark.parametrize("name", sorted(TABLES))
def test_every_lane_of_every_chunk_gets_the_record_of_its_candidate_number(name):
    length = TABLES[name].astype(np.int64)
    r0, cls = layout(length)
    rec, run, off = restated(r0, length)
    N = int(length.sum())
    T = (N + 63) // 64
    codable = bool((length <= (1 << OFF)).all())
    n = np.arange(T * 64).reshape(T, 64)
    want_valid = n < N
    nn = np.minimum(n, max(N - 1, 0))
    # (a strided walk: the per-chunk search, which is what a team's wave runs, and the cursor, which has to be right there too)
    for first, stride, batch, search in [w + (s,) for w in WALKS for s in ((False,) if w[1] == 1 else (True, False))]:
        valid, r, code, ids, visited, gN, gT, gcod = CC.walk(r0, length, cls, first=first, stride=stride, batch=batch, search=search)
        assert (gN, gT, gcod) == (N, T, codable), (name, first, stride, batch)
        mine = np.zeros(T, bool); mine[first::stride] = True
        assert np.array_equal(visited, mine), (name, first, stride, batch)
        if N == 0:
            continue
        v, wv = valid[mine], want_valid[mine]
        assert np.array_equal(v, wv), (name, first, stride, batch)
        assert np.array_equal(r[mine][wv], rec[nn[mine]][wv]), (name, first, stride, batch)
        # the code: the run's own index above the offset; a sum in the kernel, the same word as `|` while the offset fits
        want_code = (run[nn] << OFF) | off[nn] if search else (run[nn] << OFF) + off[nn]
        assert np.array_equal(code[mine][wv], want_code[mine][wv].astype(np.uint32)), (name, first, stride, batch)
        if codable:
            assert np.array_equal(want_code, (run[nn] << OFF) | off[nn]) and int(want_code.max()) < 1 << 16
        # the loads went to that record (a valid lane's class word), and nowhere for a lane past the end
        assert np.array_equal(ids[mine][wv], cls[rec[nn[mine]][wv]]) and not ids[mine][~wv].any()


def test_random_tables():
    rng = np.random.default_rng(2)
    for i in range(12):
        length = np.where(rng.random(64) < rng.random(), rng.integers(1, [3, 70, 200][i % 3], 64), 0).astype(np.int64)
        r0, cls = layout(length, seed=10 + i)
        rec, run, off = restated(r0, length)
        N = int(length.sum()); T = (N + 63) // 64
        if N == 0:
            continue
        n = np.minimum(np.arange(T * 64).reshape(T, 64), N - 1)
        ok = np.arange(T * 64).reshape(T, 64) < N
        for first, stride, batch, search in ((0, 1, 4, False), (i % 4, 4, 4, False), (i % 4, 4, 4, True)):
            valid, r, code, ids, visited, *_ = CC.walk(r0, length, cls, first=first, stride=stride, batch=batch, search=search)
            m = np.zeros(T, bool); m[first::stride] = True
            assert np.array_equal(valid[m], ok[m]) and np.array_equal(r[m][ok[m]], rec[n[m]][ok[m]])
            assert np.array_equal(code[m][ok[m]], ((run[n] << OFF) | off[n])[m][ok[m]].astype(np.uint32))


# ---- the kernel: fold and cursor together ----------------------------------------------------------------------------------------
def _three(xyz, offs, sig, origins, nv=NV, **kw):
    plain, e0 = E.voxelize_lattice(xyz, offs, sig, origins, nv, 1.0, prepass_mode=0, tile_team=0, tile_items=0, direct=0,
                                   **{k: v for k, v in kw.items() if k in ("tile_k", "lds_tier")})
    on = EC.voxelize(xyz, offs, sig, origins, nv, **kw)
    off = EC.voxelize(xyz, offs, sig, origins, nv, cover_fold=-1, **kw)
    assert e0 == 0 and on["err"] == 0 and off["err"] == 0
    return plain, on, off


def _hyd_bit(h):
    return EC.class_bit(h["table"], np.float32(1.1))


@pytest.mark.parametrize("K", [4, 8])
def test_channels_of_covered_classes_only_fold_once_behind_their_last_class(K):
    """no hydrogens: every class of the table is covered, every channel below 7 of every tile folds once and nothing follows the fold"""
    xyz, offs, sig, origins = ragged()
    sig[sig == np.float32(1.1)] = 0.0
    plain, on, off = _three(xyz, offs, sig, origins, tile_k=K)
    assert int(on["masks"][0]) == 0xfffe
    assert np.array_equal(plain, on["out"]) and np.array_equal(plain, off["out"]) and plain[..., :7].max() > 0.5 and plain[..., 7].max() > 0.5
    mut = EC.voxelize(xyz, offs, sig, origins, NV, tile_k=K, mutant=True)            # (the fold is what carries channel 7 here)
    assert not np.array_equal(mut["out"], plain) and np.array_equal(mut["out"][..., :7], plain[..., :7])


@pytest.mark.parametrize("K", [4, 8])
def test_a_hydrogen_in_every_channel_below_7_of_every_tile(K):
    """the uncovered class (1.1 A) in every channel 0..6 around every tile: no channel is all covered; the covered classes still
    fold, the hydrogens behind them do not, and channel 7 must not see them"""
    xyz, offs, sig, origins = ragged()
    rng = np.random.default_rng(4)
    a0, a1 = int(offs[0]), int(offs[1])
    hyd = np.nonzero(sig[a0:a1].max(axis=1) == np.float32(1.1))[0] + a0
    assert len(hyd) > 100
    sig[hyd, :7] = 1.1                                                               # every hydrogen of item 0 in all seven channels
    xyz[hyd] = rng.uniform([-8, -8, -4], [8, 8, 4], size=(len(hyd), 3)).astype(np.float32)      # ... inside item 0's grid: > 1 per 8 A^3 tile
    plain, on, off = _three(xyz, offs, sig, origins, tile_k=K)
    h = on
    assert not int(h["masks"][0]) & _hyd_bit(h) and bin(~int(h["masks"][0]) & 0xfffe).count("1") == 1
    g = plain[0].reshape(16, 16, 8, 8)
    for c in range(7):                                                               # a hydrogen's value in every tile of every channel
        tiles = g[..., c].reshape(16 // K, K, 2, 8, 1, 8).max(axis=(1, 3, 5))
        assert (tiles > 0.5).all(), c
    assert np.array_equal(plain, on["out"]) and np.array_equal(plain, off["out"])
    assert not np.array_equal(EC.voxelize(xyz, offs, sig, origins, NV, tile_k=K, mutant=True)["out"], plain)


@pytest.mark.parametrize("K", [4, 8])
def test_both_kinds_of_channel_in_one_tile(K):
    """channels 0..2 carry hydrogens beside the heavy classes, channels 3..6 heavy atoms only"""
    xyz, offs, sig, origins = ragged()
    hyd = sig.max(axis=1) == np.float32(1.1)
    sig[hyd, 3:7] = 0.0
    heavy = np.nonzero(~hyd & (sig[:, 7] > 0))[0]
    sig[heavy[::3], 4] = sig[heavy[::3], 7]                                          # (the thin channels get entries in every tile)
    sig[heavy[1::3], 6] = sig[heavy[1::3], 7]
    plain, on, off = _three(xyz, offs, sig, origins, tile_k=K)
    assert bin(~int(on["masks"][0]) & 0xfffe).count("1") == 1 and not int(on["masks"][0]) & _hyd_bit(on)
    assert np.array_equal(plain, on["out"]) and np.array_equal(plain, off["out"])
    assert plain[0, :, 0].max() > 0.5 and plain[0, :, 6].max() > 0.5
    assert not np.array_equal(EC.voxelize(xyz, offs, sig, origins, NV, tile_k=K, mutant=True)["out"], plain)


def test_a_team_and_the_dense_tier_with_the_cursor():
    """the team kernel (strided chunks: it keeps the per-chunk search, not the cursor), the DENSE instance, the direct layout and
    the general path (these three traverse with the cursor)"""
    xyz, offs, sig, origins = ragged()
    plain, _ = E.voxelize_lattice(xyz, offs, sig, origins, NV, 1.0, prepass_mode=0, tile_team=0, tile_items=0, direct=0)
    team = EC.voxelize(xyz, offs, sig, origins, NV, tile_team=1)
    assert team["err"] == 0 and np.array_equal(team["out"], plain)
    rng = np.random.default_rng(7)
    n = 3400
    s2 = np.ascontiguousarray(synth_sigmas(rng, n), np.float32)
    x2 = rng.uniform([-13, -13, -9], [13, 13, 9], size=(n, 3)).astype(np.float32)
    o2, g2 = np.array([0, n], np.int64), np.array([[-8.0, -8.0, -4.0]])
    p2, _ = E.voxelize_lattice(x2, o2, s2, g2, NV, 1.0, prepass_mode=0, tile_team=0, tile_items=0, direct=0, lds_tier=0)
    d2 = EC.voxelize(x2, o2, s2, g2, NV, lds_tier=0)
    assert d2["feedback"][0] > 0 and np.array_equal(d2["out"], p2)
    # the direct layout (up to 27 cell runs + the spill run) against the column layout (9 runs): another run table, the same bits
    for caps in (dict(), dict(cell_cap=4, spill_cap=4096)):                          # (4 slots per cell: most atoms go through the spill run)
        words = np.zeros(4, np.uint32)
        dd, e = E.voxelize_lattice(xyz, offs, sig, origins, NV, 1.0, prepass_mode=0, tile_team=0, tile_items=0, direct=1, repeat=2,
                                   direct_words=words, **caps)
        assert e == 0 and words[0] == 0 and (words[1] > 100) == bool(caps) and np.array_equal(dd, plain), (caps, words)
    gen, e = E.voxelize_lattice(xyz, offs, sig, origins, NV, 1.0, prepass_mode=0, tile_team=0, tile_items=0, direct=0, force_general=True)
    assert e == 0 and np.array_equal(gen, plain)
