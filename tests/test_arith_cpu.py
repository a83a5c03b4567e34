"""CPU tier: the arithmetic probe (moleculekit_amd/csrc/arith_probe.h) on the host emulation, over the cases of tests/arith_cases.py.

The emulation replaces the device primitives with the host's a / b, sqrtf and nearbyintf, so this tier cannot speak for the device
lowering -- tests/test_gpu_arith.py sends the same cases through ``Context.arith_probe`` with the same assertions.  What it proves
without a GPU: the vectors are what arith_cases.py says they are (every special, every exponent, both sides of every branch, inputs
that tell a fused multiply-add from two roundings), the numpy references agree with the product's source compiled for the host, and
the emulator's replacements are the correctly rounded operations the references assume.
"""
import os
import platform
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import arith_cases as AC  # noqa: E402
import rings_restatement as RR  # noqa: E402

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def probe():
    import emu_arith_build
    emu_arith_build.build()
    return emu_arith_build.probe


def test_every_operation_of_the_probe_has_cases_and_the_binding_names_them(probe):
    import emu_arith_build
    from moleculekit_amd._lib import ARITH_OPS
    assert sorted(AC.OPS) == sorted(ARITH_OPS) and len(ARITH_OPS) == emu_arith_build.n_ops()
    assert sorted(v[0] for v in ARITH_OPS.values()) == list(range(len(ARITH_OPS)))
    for name, (code, arity, in_dt, out_dt, cols) in ARITH_OPS.items():
        assert emu_arith_build.arity(code) == arity, name
        assert (name in AC.UNARY, name in AC.BINARY + AC.BINARY64, name in AC.TERNARY + AC.TERNARY64) == (arity == 1, arity == 2, arity == 3)
    grouped = [op for g in AC.GROUPS.values() for op in g] + ["acosf", "ring_angle"]
    assert sorted(grouped) == sorted(AC.OPS)
    # an unknown operation and a missing operand are refused, nothing is launched
    import ctypes
    x = np.zeros(3, F32)
    px = x.ctypes.data_as(ctypes.c_void_p)
    L = emu_arith_build.lib()
    assert L.emu_arith_probe(ctypes.c_int(len(ARITH_OPS)), ctypes.c_longlong(3), px, px, px, px) != 0 and b"unknown" in L.emu_arith_last_error()
    assert L.emu_arith_probe(ctypes.c_int(ARITH_OPS["fadd"][0]), ctypes.c_longlong(3), px, None, None, px) != 0 and b"NULL" in L.emu_arith_last_error()
    # ... and the sentinel is in place where nothing is written: an empty call
    assert probe("fadd", x[:0], x[:0]).size == 0


def test_the_vectors_are_what_they_claim():
    S = AC.bits32(AC.SPECIALS)
    for must in (0, 0x80000000, 1, 0x007fffff, 0x00800000, 0x0f7fffff, 0x0f800000, 0x0f800001, 0x3effffff, 0x3f000000, 0x3f000001,
                 0x3f7fffff, 0x3f800000, 0x3f800001, 0xbf800000, 0x22ffffff, 0x23000000, 0x23000001, 0xa3000000, 0x7f7fffff, 0x7f800000,
                 0xff800000, 0x7fc00000):
        assert must in S, hex(must)
    assert len(set(S.tolist())) == S.size == 34
    L = AC.bits32(AC.ladder32())
    assert L.size == 255 * 256 * 2 and set(((L >> 23) & 0xff).tolist()) == set(range(255)) and (L >> 31).sum() == L.size // 2
    L64 = AC.ladder64().view(np.uint64)
    assert set(((L64 >> np.uint64(52)) & np.uint64(0x7ff)).tolist()) == set(range(0, 2047, 16))
    for cols in (AC.unary32(), AC.binary32(), AC.ternary32(), AC.binary64(), AC.ternary64(), AC.fdiv_cases(), AC.round_cases(),
                 AC.round_quot_cases(), AC.wrap_decide_cases()):
        assert cols[0].size % 64 != 0 and not cols[0].flags.writeable
    # the cross products are complete
    a, b = AC.binary32()
    assert len(set(zip(AC.bits32(a[:34 * 34]).tolist(), AC.bits32(b[:34 * 34]).tolist()))) == 34 * 34
    a, b, c = AC.ternary32()
    assert len(set(zip(*(AC.bits32(x[:34 ** 3]).tolist() for x in (a, b, c))))) == 34 ** 3
    # the rounding edges
    r = AC.round_cases()[0]
    for v in (0.5, -0.5, 4096.5, -4096.5, 2.5, 0.49999997, -0.49999997, 2.0 ** 22 + 0.5, 2.0 ** 22 - 0.5, 2.0 ** 23 - 1, 2.0 ** 23, 2.0 ** 24, -0.4):
        assert F32(v) in r, v
    assert np.nextafter(F32(2.5), F32(3)) in r and np.nextafter(F32(2.5), F32(2)) in r
    # the division's edges: denormal quotients, overflow, ties
    a, b = AC.fdiv_cases()
    with np.errstate(all="ignore"):
        q = a / b
        exact = a.astype(F64) / b.astype(F64)
    tiny = np.isfinite(q) & (np.abs(q) < F32(2.0 ** -126)) & (q != 0)
    assert tiny.sum() > 10000 and (np.isinf(q) & np.isfinite(a) & (b != 0)).sum() > 10000
    for d in (1, 2, 10, 4096, 2 ** 24 - 1, 2 ** 24):
        assert F32(d) in b
    # a tie: the exact quotient (a power-of-two divisor: float64 holds it) lies halfway between two float32 neighbours
    lo = np.minimum(np.nextafter(q, F32(-np.inf)), q).astype(F64)
    pw2 = np.isin(np.abs(b), [2.0, 4.0, 8.0, 1024.0]) & np.isfinite(q)
    mid_dn = (q.astype(F64) + np.nextafter(q, F32(-np.inf)).astype(F64)) / 2
    mid_up = (q.astype(F64) + np.nextafter(q, F32(np.inf)).astype(F64)) / 2
    ties = pw2 & ((exact == mid_dn) | (exact == mid_up))
    assert ties.sum() > 10000, ties.sum()
    assert (AC.bits32(q[ties]) & 1 == 0).all()                         # ... and the reference went to the even neighbour


def test_the_root_layout_puts_both_sides_of_the_ballot_on_the_same_values():
    x, plain, mixed, n_runs = AC.sqrt_layout()
    assert x.size % 64 != 0 and AC.ordinary(x[plain]).all() and plain.size == 64 * n_runs
    odd = AC.SPECIALS[~AC.ordinary(AC.SPECIALS)]
    assert mixed.shape == (odd.size * 3, 64 * n_runs) and odd.size >= 20
    for row in mixed:
        runs = x[row].reshape(n_runs, 64)
        assert ((~AC.ordinary(runs)).sum(axis=1) == 1).all()           # every wave of a mixed run takes the long form
    assert (mixed % 64 == np.arange(64 * n_runs) % 64).all() and plain[0] % 64 == 0      # lanes are kept
    # denormals and numbers below 2^-96 reach the scaled branch, next to the ladder's
    assert (AC.bits32(x) < 0x00800000).sum() > 500 and ((AC.bits32(x) >= 0x00800000) & (AC.bits32(x) < 0x0f800000)).sum() > 5000


def test_roundf_reference_is_the_restatements_round_with_the_sign_of_zero():
    x = np.concatenate([AC.unary32()[0], AC.round_cases()[0]])
    mine, theirs = AC.c_roundf(x), RR._c_round(x)
    ok = ~np.isnan(theirs)
    assert np.array_equal(mine[ok], theirs[ok]) and np.isnan(mine[~ok]).all()              # equal as numbers (-0 == +0) ...
    apart = AC.bits32(mine[ok]) != AC.bits32(theirs[ok])
    assert (mine[ok][apart] == 0).all() and np.signbit(x[ok][apart]).all()                 # ... and apart only as -0 against +0
    assert AC.bits32(AC.c_roundf(F32([-0.4, 0.49999997, -0.49999997, 0.5, -0.5, 2.5, 8388607.5]))).tolist() == \
        AC.bits32(F32([-0.0, 0.0, -0.0, 1.0, -1.0, 3.0, 8388608.0])).tolist()


def test_multiply_add_inputs_tell_two_roundings_from_one():
    """at least 20 % of the uniform(-50, 50) triples give another result fused (measured: 26 % for both widths)"""
    a, b, c = AC.muladd_triples32()
    two = AC.reference("fmul_add", a, b, c)
    share32 = float((AC.bits32(two) != AC.bits32(AC.fused32(a, b, c))).mean())
    a, b, c = AC.muladd_triples64()
    two = AC.reference("dmul_add", a, b, c)
    share64 = float((two.view(np.uint64) != AC.fused64(a, b, c).view(np.uint64)).mean())
    print("fused differs: float32 %.3f of %d, float64 %.3f of %d" % (share32, a.size << 8, share64, a.size))
    assert AC.muladd_triples32()[0].size == 1 << 20 and a.size == 4096
    assert share32 >= 0.2 and share64 >= 0.2, (share32, share64)


def test_minimum_image_cases_reach_both_branches():
    """In every range with a normal box the share of cases that take the reciprocal shortcut lies in [0.2, 0.8]; where the reciprocal of
    a denormal box overflows (boxes below 2^-128) no case takes it."""
    mi = AC.min_image_cases()
    shares = {}
    for name in AC.MIN_IMAGE_RANGES:
        a, b = mi[name]
        took = AC.min_image_takes_shortcut(a, b)
        shares[name] = float(took.mean())
        if name == "denormal":
            with np.errstate(all="ignore"):
                overflow = np.isinf(F32(1) / b)
            assert overflow.sum() > 10000 and not took[overflow].any()
            shares["denormal, finite reciprocal"] = float(took[~overflow].mean())
        else:
            assert 0.2 <= shares[name] <= 0.8, shares
    print("shortcut shares:", shares)
    a, b = mi["2^126..max"]
    with np.errstate(all="ignore"):
        ib = F32(1) / b
    assert (np.abs(ib) < F32(2.0 ** -126)).all() and (ib != 0).all()                       # the reciprocal is a denormal there
    assert (mi["edges"][1] == 0).sum() > 1000 and (~np.isfinite(mi["edges"][0])).sum() > 1000


@pytest.mark.parametrize("group", list(AC.GROUPS))
def test_operations_match_their_references_on_the_emulation(probe, group):
    AC.check_group(probe, group)


def test_acosf_and_the_folded_angle_match_the_restatement_on_the_emulation(probe):
    AC.check_acos(probe)


def test_the_c_librarys_acosf_is_the_restatement_where_it_is_the_goldens_glibc(probe):
    """glibc 2.35 made the golden ring data; its acosf is fdlibm's, which the restatement (and ring_acosf) restate"""
    if platform.libc_ver() != ("glibc", "2.35"):
        pytest.skip("the host's C library is %s %s, not the goldens' glibc 2.35" % platform.libc_ver())
    import emu_arith_build
    bad = 0
    for (x,) in AC.acos_chunks():
        bad += AC.compare(emu_arith_build.libm_acosf(x), RR.acosf(x)).size
    assert bad == 0
