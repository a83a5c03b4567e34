"""tests/arith_cases.py -- TEST INFRASTRUCTURE: the vectors and the independent references of the arithmetic probe
(moleculekit_amd/csrc/arith_probe.h, ``Context.arith_probe``; on the host emulation ``emu_arith_build.probe``).

Every vector is seeded and built from bit patterns; every reference is plain numpy, where a float32 operation on float32 arrays rounds
once (IEEE division and square root included, denormals kept) -- nothing here calls the code under test.

  SPECIALS     +-0, +-smallest and +-largest denormal, +-smallest normal, the three patterns around 2^-96 (where mk_fsqrt_rn changes
               branch), +-0.5 and +-1 with both neighbours, +-2^-57 with both neighbours (acosf's tiny branch), +-largest finite, +-inf,
               a quiet NaN.  Binary and ternary operations get their full cross product.
  ladder32     every float32 exponent (0..254) x 256 seeded mantissas x both signs; binary operations pair it with a shuffled copy and
               with every special in both roles.  ladder64: the same over every 16th float64 exponent.
  per operation the edges listed at its function below.

``run(probe, op)`` sends the operation's vectors through ``probe`` in chunks and returns a ``Report``: elements, mismatches, and the
first mismatching input patterns.  Finite results and zeros are compared as bit patterns; where the reference is a NaN the result must
be a NaN (payload and sign are not claimed).
"""
from __future__ import annotations

import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np

import rings_restatement as RR

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64
SIGN = 0x80000000
CHUNK = (1 << 22) - 27              # elements per probe call: not a multiple of 64 (nor of the 256 threads of a block)

UNARY = ("fsqrt", "ring_sqrt", "roundf", "rint", "dround", "acosf", "ring_angle")
BINARY = ("fadd", "fsub", "fmul", "fdiv", "ring_div", "round_quot", "ring_round_quot", "min_image", "min_image_pk", "dih_wrap")
TERNARY = ("fmul_add", "wrap_decide")
BINARY64, TERNARY64 = ("ddiv",), ("dmul_add",)
OPS = UNARY + BINARY + TERNARY + BINARY64 + TERNARY64


def f32(bits):
    return np.ascontiguousarray(np.asarray(bits, dtype=np.int64).astype(U32)).view(F32)


def f64(bits):
    return np.ascontiguousarray(np.asarray(bits, dtype=U64)).view(F64)


def bits32(x):
    return np.ascontiguousarray(x, F32).view(U32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _special_bits():
    b = [0x00000000, SIGN, 0x00000001, SIGN | 1, 0x007fffff, SIGN | 0x007fffff, 0x00800000, SIGN | 0x00800000,
         0x0f7fffff, 0x0f800000, 0x0f800001]
    for p in (0x3f000000, 0x3f800000, 0x23000000):
        for s in (0, SIGN):
            b += [s | (p - 1), s | p, s | (p + 1)]
    b += [0x7f7fffff, SIGN | 0x7f7fffff, 0x7f800000, SIGN | 0x7f800000, 0x7fc00000]
    return b


SPECIALS = _frozen(f32(_special_bits()))
# float64: the float32 specials widened (exact) and the float64 patterns of the same kind
SPECIALS64 = _frozen(np.concatenate([
    SPECIALS.astype(F64),
    f64([0x1, 0x8000000000000001, 0x000fffffffffffff, 0x800fffffffffffff, 0x0010000000000000, 0x8010000000000000,
         0x3fdfffffffffffff, 0x3fe0000000000001, 0x3fefffffffffffff, 0x3ff0000000000001, 0xbfefffffffffffff, 0xbff0000000000001,
         0x7fefffffffffffff, 0xffefffffffffffff])]))


def ordinary(x):
    """mk_fsqrt_rn's own split: a float in [2^-96, inf)"""
    b = bits32(x)
    return (b >= 0x0f800000) & (b < 0x7f800000)


@functools.lru_cache(None)
def ladder32():
    rng = np.random.default_rng(1001)
    e = np.repeat(np.arange(255, dtype=U32), 256)
    pos = (e << U32(23)) | rng.integers(0, 1 << 23, size=e.size, dtype=U32)
    return _frozen(np.concatenate([pos, pos | U32(SIGN)]).view(F32))


@functools.lru_cache(None)
def ladder64():
    rng = np.random.default_rng(1002)
    e = np.repeat(np.arange(0, 2047, 16, dtype=U64), 256)
    pos = (e << U64(52)) | rng.integers(0, 1 << 52, size=e.size, dtype=U64)
    return _frozen(np.concatenate([pos, pos | U64(1 << 63)]).view(F64))


def _cross(*sets):
    g = np.meshgrid(*sets, indexing="ij")
    return tuple(np.ascontiguousarray(x.ravel()) for x in g)


def _odd(cols):
    """the same columns, a few elements longer if their length is a multiple of 64"""
    cols = tuple(cols)
    if cols[0].size % 64 == 0:
        cols = tuple(np.concatenate([c, c[:37]]) for c in cols)
    assert cols[0].size % 64 and all(c.size == cols[0].size for c in cols)
    return _frozen(*cols) if len(cols) > 1 else (_frozen(cols[0]),)


def _stack(*parts):
    """parts: tuples of equally long columns -> one tuple of columns"""
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(len(parts[0])))


@functools.lru_cache(None)
def unary32():
    return _odd((np.concatenate([SPECIALS, ladder32()]),))


@functools.lru_cache(None)
def binary32():
    """specials x specials; the ladder with a shuffled copy; the ladder with every special, in both roles"""
    rng = np.random.default_rng(1003)
    L = ladder32()
    la, sb = _cross(L, SPECIALS)
    return _odd(_stack(_cross(SPECIALS, SPECIALS), (L, rng.permutation(L)), (la, sb), (sb, la)))


@functools.lru_cache(None)
def ternary32():
    rng = np.random.default_rng(1004)
    L = ladder32()
    return _odd(_stack(_cross(SPECIALS, SPECIALS, SPECIALS), (L, rng.permutation(L), rng.permutation(L))))


@functools.lru_cache(None)
def binary64():
    rng = np.random.default_rng(1005)
    L = ladder64()
    la, sb = _cross(L, SPECIALS64)
    return _odd(_stack(_cross(SPECIALS64, SPECIALS64), (L, rng.permutation(L)), (la, sb), (sb, la)))


@functools.lru_cache(None)
def ternary64():
    rng = np.random.default_rng(1006)
    L = ladder64()
    return _odd(_stack(_cross(SPECIALS64, SPECIALS64, SPECIALS64), (L, rng.permutation(L), rng.permutation(L))))


# ------------------------------------------------------------------------------------------------
# the root: runs of 64 consecutive elements are the lanes of one wave
# ------------------------------------------------------------------------------------------------
SQRT_LANES = (0, 31, 63)


@functools.lru_cache(None)
def sqrt_layout():
    """-> (x, plain, mixed, n_runs): ``x`` the probe's input; ``plain`` [n_runs * 64] the indexes of runs of ordinary values only (every
    lane of their waves takes the short form); ``mixed`` [variants, n_runs * 64] the indexes of the same runs laid out again with lane
    0, 31 or 63 replaced by one non-ordinary special (the whole wave takes the long form) -- at a replaced lane the index points at
    the special.  Behind them the ladder sorted (ordinary runs among it) and shuffled (hardly a run without a negative number), the
    specials, and a last partial run."""
    rng = np.random.default_rng(1007)
    L = ladder32()
    ordv = L[ordinary(L)]
    n_runs = 16
    runs = np.concatenate([rng.choice(ordv, 48 * n_runs), f32(rng.integers(0x0f800000, 0x10800000, 8 * n_runs)),   # just above 2^-96
                           f32(rng.integers(0x7e800000, 0x7f800000, 8 * n_runs))])                                   # just below inf
    runs = rng.permutation(runs).astype(F32)
    assert ordinary(runs).all() and runs.size == 64 * n_runs
    odd = SPECIALS[~ordinary(SPECIALS)]
    parts, mixed = [runs], []
    pos = runs.size
    for s in odd:
        for lane in SQRT_LANES:
            v = runs.copy()
            v[lane::64] = s
            parts.append(v)
            mixed.append(np.arange(pos, pos + v.size))
            pos += v.size
    x = np.concatenate(parts + [L, rng.permutation(L), SPECIALS, runs[:37]])
    assert x.size % 64 and x.size < CHUNK
    return _frozen(x), np.arange(runs.size), np.array(mixed), n_runs


def sqrt_layout_disagreements(got):
    """ordinary values whose root differs between the run of ordinary values and the same run with a non-ordinary lane in it"""
    x, plain, mixed, _ = sqrt_layout()
    gb = bits32(got)
    keep = np.ones(plain.size, bool)
    bad = 0
    for lane in SQRT_LANES:
        rows = mixed[SQRT_LANES.index(lane)::len(SQRT_LANES)]
        keep[:] = True
        keep[lane::64] = False
        assert (bits32(x)[rows][:, keep] == bits32(x)[plain][keep]).all()
        bad += int((gb[rows][:, keep] != gb[plain][keep]).sum())
    return bad


# ------------------------------------------------------------------------------------------------
# the division
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def fdiv_cases():
    """Divisors 1..4096, 2^24 - 1, 2^24 (the running mean's n + 1), 10 and 2 under seeded numerators of every exponent and the specials;
    quotients that are denormal, that overflow, and that are round-to-even ties (an odd denormal pattern, or a normal number whose
    low bits stick out below 2^-149 by exactly a half, divided by a power of two: only a denormal quotient can be a tie).  0 / 0,
    x / 0 and inf / inf are in the specials' cross product."""
    rng = np.random.default_rng(1008)
    div = np.concatenate([np.arange(1, 4097), [2 ** 24 - 1, 2 ** 24]]).astype(F32)
    num = np.concatenate([SPECIALS, f32(rng.integers(0, 0x7f800000, 768)), -f32(rng.integers(0, 0x7f800000, 256))])
    parts = [_cross(num, div)]
    n = 1 << 16
    small = f32(rng.integers(1, 0x10000000, n) | (rng.integers(0, 2, n) << 31))              # below 2^-95
    big = f32(rng.integers(0x3f800000, 0x4b800000, n) | (rng.integers(0, 2, n) << 31))       # 1 .. 2^24
    huge = f32(rng.integers(0x73000000, 0x7f800000, n) | (rng.integers(0, 2, n) << 31))
    parts += [(small, big), (huge, small), (huge, f32(rng.integers(0x30000000, 0x3f800000, n)))]
    tie_num = f32(rng.integers(0, 0x02000000, n) | 1 | (rng.integers(0, 2, n) << 31))          # odd patterns: denormal .. 2^-123
    parts += [(tie_num, np.full(n, p, F32)) for p in (2.0, 4.0, 8.0, 1024.0, -2.0)]
    tie_num = f32((rng.integers(0, 0x02000000, n) | 3) | (rng.integers(0, 2, n) << 31))        # ... ties with an odd neighbour below
    parts += [(tie_num, np.full(n, 2.0, F32))]
    return _odd(_stack(*parts))


# ------------------------------------------------------------------------------------------------
# the roundings
# ------------------------------------------------------------------------------------------------
def c_round64(x):
    """C's round() of float64 values: half away from zero, the sign of the argument kept (round(-0.4) is -0)"""
    x = np.asarray(x, F64)
    with np.errstate(all="ignore"):
        return np.copysign(np.floor(np.abs(x) + 0.5), x)


def c_roundf(x):
    """C's roundf() of float32 values: rings_restatement._c_round, with the sign of the argument on a zero result (which that
    restatement, made for quotients it multiplies a box with, does not keep).  |x| + 0.5 is exact in float64 for every float32
    below 2^52 and rounds back to |x| above."""
    x = np.ascontiguousarray(x, F32)
    with np.errstate(all="ignore"):
        return np.copysign(RR._c_round(x), x)


@functools.lru_cache(None)
def round_cases():
    """k + 0.5 for |k| <= 4096 with both neighbours; +-0.49999997; 2^22 +- 0.5, 2^23 - 1, 2^23, 2^24; -0.4; all in both signs"""
    k = np.arange(-4096, 4097).astype(F64) + 0.5
    h = k.astype(F32)
    assert (h.astype(F64) == k).all()
    one = np.concatenate([h, np.nextafter(h, F32(np.inf)), np.nextafter(h, F32(-np.inf)),
                          f32([0x3effffff]), np.array([2.0 ** 22 - 0.5, 2.0 ** 22 + 0.5, 2.0 ** 23 - 1, 2.0 ** 23, 2.0 ** 24, 2.0 ** 23 - 0.5,
                                                       2.0 ** 23 + 1, 2.0 ** 24 - 1, 2.0 ** 24 + 2, 0.4, 0.6], F32)])
    assert one.dtype == F32 and F32(0.49999997) == f32([0x3effffff])[0]
    return _odd((np.concatenate([one, -one]),))


def _ulp_steps(a, steps):
    """[len(steps), n]: a moved by that many float32 patterns away from zero (negative: towards it)"""
    b = bits32(a).astype(np.int64)
    mag = (b & 0x7fffffff)[None, :] + np.asarray(steps, np.int64)[:, None]
    assert (mag >= 0).all() and (mag < 0x7f800000).all()
    return f32((mag | (b & SIGN)[None, :]).ravel()).reshape(len(steps), a.size)


STEPS = np.arange(-6, 7)


@functools.lru_cache(None)
def round_quot_cases():
    """a = (k + 0.5) b EXACTLY -- b a power of two, or a number with a short mantissa -- and the same a moved by +-1..6 patterns"""
    rng = np.random.default_rng(1009)
    pow2 = np.array([2.0 ** e for e in (-140, -126, -100, -30, -3, 0, 1, 5, 20, 60, 100)], F64)
    short = np.concatenate([np.arange(3, 1024, 2)[rng.integers(0, 510, 24)] * 2.0 ** rng.integers(-40, 40, 24),
                            [10.0, 30.0, 45.5, 66.875, 0.625]])
    b = np.concatenate([pow2, short, -short[:4]])
    k = np.concatenate([np.arange(-64, 65), [-4096, -1000.0, 511, 2047, 4096]]) + 0.5
    kk, bb = _cross(k, b)
    a64 = kk * bb
    a = a64.astype(F32)
    assert (a.astype(F64) == a64).all() and (bb.astype(F32).astype(F64) == bb).all()       # exact products
    a = a[np.abs(a64) >= 2.0 ** -140 * 8]                                                        # room for six patterns towards zero
    bb = bb[np.abs(a64) >= 2.0 ** -140 * 8]
    moved = _ulp_steps(a, STEPS)
    return _odd((moved.ravel(), np.tile(bb.astype(F32), len(STEPS))))


# ------------------------------------------------------------------------------------------------
# the minimum image with its reciprocal shortcut
# ------------------------------------------------------------------------------------------------
MIN_IMAGE_RANGES = ("10..100", "1e-38..1e-37", "denormal", "2^125..2^126", "2^126..max")


@functools.lru_cache(None)
def min_image_cases():
    """-> {range: (a, b)}: boxes b drawn from five ranges -- [10, 100], [1e-38, 1e-37], the denormals, [2^125, 2^126], [2^126, max) (there
    the reciprocal is a denormal) -- and separations a = +-(k + 0.5) b moved by -6..6 patterns, k in 0..2 for the first three ranges
    and 0 for the last two (a stays finite); under "edges": b = 0 and non-finite a."""
    rng = np.random.default_rng(1010)
    n = 4096
    boxes = {"10..100": rng.uniform(10, 100, n).astype(F32),
             "1e-38..1e-37": rng.uniform(1e-38, 1e-37, n).astype(F32),
             "denormal": f32(rng.integers(0x40, 0x00800000, n)),
             "2^125..2^126": f32(rng.integers(0x7e000000, 0x7e800000, n)),
             "2^126..max": f32(rng.integers(0x7e800000, 0x7f7ffff0, n))}
    out = {}
    for name, b in boxes.items():
        ks = (0, 1, 2) if name in MIN_IMAGE_RANGES[:3] else (0,)
        cols = []
        with np.errstate(all="ignore"):
            for k in ks:
                a0 = (F32(k + 0.5) * b).astype(F32)
                a0 = np.where(bits32(a0) < 8, f32([8])[0], a0)
                for s in (F32(1), F32(-1)):
                    m = _ulp_steps(s * a0, STEPS)
                    cols.append((m.ravel(), np.tile(b, len(STEPS))))
        a, bb = _stack(*cols)
        assert np.isfinite(a).all()
        out[name] = _frozen(a, bb)
    L = ladder32()[::17]
    nonfinite = f32([0x7f800000, SIGN | 0x7f800000, 0x7fc00000])
    e1 = _cross(np.concatenate([L, SPECIALS]), f32([0, SIGN]))
    e2 = _cross(nonfinite, np.concatenate([L, SPECIALS]))
    out["edges"] = _frozen(*_stack(e1, e2))
    return out


def min_image_takes_shortcut(a, b):
    """the kernel's own test tm < fma(-3e-7, qm, 0.5) on each case (dist_kernels.h: dist2_min_image_f32; the y and z axes of the
    probe's call are zero, so qm -- the sum of the three |q| -- is |qx|, and tm, a maximum that ignores a NaN, is |qx - rx| or 0)"""
    with np.errstate(all="ignore"):
        ib = (F32(1) / b).astype(F32)
        q = (a * ib).astype(F32)
        r = np.rint(q)
        tm = np.fmax((np.abs(q - r)).astype(F32), F32(0))
        qm = np.abs(q)                                                      # a NaN stays: the comparison is false then
        bound = (F64(F32(-3e-7)) * qm.astype(F64) + 0.5).astype(F32)        # the product is exact in float64
        return tm < bound


# ------------------------------------------------------------------------------------------------
# multiply, then add: two roundings, never one
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def muladd_triples32():
    rng = np.random.default_rng(1011)
    return _frozen(*(rng.uniform(-50, 50, 1 << 20).astype(F32) for _ in range(3)))


@functools.lru_cache(None)
def muladd_triples64():
    rng = np.random.default_rng(1012)
    return _frozen(*(rng.uniform(-50, 50, 4096) for _ in range(3)))


def fused32(a, b, c):
    """a * b + c rounded ONCE to float32 (the product is exact in float64; the sum is rounded to 53 bits first, which moves a float32
    result only where it sits within 2^-29 of a float32 rounding boundary)"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def fused64(a, b, c):
    """a * b + c rounded once to float64, through exact rationals"""
    return np.array([float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], F64)


# ------------------------------------------------------------------------------------------------
# acosf: chunks made on the way
# ------------------------------------------------------------------------------------------------
def acos_chunks():
    """every pattern of [0.5, 1] and [-1, -0.5] (where the split root and the sensitive angles live), every 64th pattern of
    2^-57 < |x| < 0.5 in both signs, then the specials, the ladder (|x| > 1 among it) and the patterns just above 1"""
    for lo, hi, step in ((0x3f000000, 0x3f800001, 1), (0x23000001, 0x3f000000, 64)):
        for s in (0, SIGN):
            for start in range(lo, hi, step * CHUNK):
                yield (f32(np.arange(start, min(hi, start + step * CHUNK), step, dtype=np.int64) | s),)
    above = np.arange(0x3f800001, 0x3f800001 + 300, dtype=np.int64)
    yield (np.concatenate([SPECIALS, ladder32(), f32(above), f32(above | SIGN)]),)


# ------------------------------------------------------------------------------------------------
# vectors and references per operation
# ------------------------------------------------------------------------------------------------
def wrap_decide_cases():
    """(group centre, box centre, box): the specials' cube and the ladder; the quotients next to a half-integer of the minimum
    image's ranges against a box centre of zero and against one that leaves the difference inexact"""
    mi = min_image_cases()
    parts = [ternary32()]
    for name in MIN_IMAGE_RANGES:
        a, b = mi[name]
        parts += [(a, np.zeros_like(a), b), (a, (b * F32(0.001)).astype(F32), b)]
    return _odd(_stack(*parts))


def inputs(op):
    """the operation's vectors, as a tuple of equally long columns (not for acosf / ring_angle: ``acos_chunks``)"""
    if op == "fsqrt":
        return (sqrt_layout()[0],)
    if op == "ring_sqrt":
        return _odd(_stack(unary32(), (sqrt_layout()[0],)))
    if op in ("roundf", "rint", "dround"):
        return _odd(_stack(unary32(), round_cases()))
    if op in ("fadd", "fsub", "fmul", "dih_wrap"):
        return binary32()
    if op in ("fdiv", "ring_div"):
        return _odd(_stack(binary32(), fdiv_cases(), round_quot_cases()))
    if op in ("round_quot", "ring_round_quot"):
        return _odd(_stack(binary32(), round_quot_cases(), _cross(round_cases()[0], f32([0x3f800000, 0x40000000, 0x3f000000]))))
    if op in ("min_image", "min_image_pk"):
        mi = min_image_cases()
        return _odd(_stack(binary32(), round_quot_cases(), *[mi[k] for k in MIN_IMAGE_RANGES + ("edges",)]))
    if op == "fmul_add":
        return _odd(_stack(ternary32(), muladd_triples32()))
    if op == "wrap_decide":
        return wrap_decide_cases()
    if op == "ddiv":
        return binary64()
    if op == "dmul_add":
        return _odd(_stack(ternary64(), muladd_triples64()))
    raise KeyError(op)


def chunks(op):
    if op in ("acosf", "ring_angle"):
        yield from acos_chunks()
        return
    cols = inputs(op)
    n = cols[0].size
    assert op != "fsqrt" or n <= CHUNK                  # the wave layout is one call
    for s in range(0, n, CHUNK):
        yield tuple(c[s:s + CHUNK] for c in cols)


def reference(op, a, b=None, c=None):
    """the independent numpy reference of ``op`` on the columns a, b, c"""
    with np.errstate(all="ignore"):
        if op == "fadd":
            r = a + b
        elif op == "fsub":
            r = a - b
        elif op == "fmul":
            r = a * b
        elif op == "fmul_add":
            r = (a * b).astype(F32) + c
        elif op == "dmul_add":
            r = (a * b).astype(F64) + c
        elif op in ("fdiv", "ring_div", "ddiv"):
            r = a / b
        elif op in ("fsqrt", "ring_sqrt"):
            r = np.sqrt(a)
        elif op == "roundf":
            r = c_roundf(a)
        elif op == "rint":
            r = np.rint(a)
        elif op == "dround":
            r = c_round64(a.astype(F64))
        elif op in ("round_quot", "ring_round_quot"):
            r = c_roundf((a / b).astype(F32))
        elif op == "min_image":
            v = (a - (b * c_roundf((a / b).astype(F32))).astype(F32)).astype(F32)
            r = ((v * v).astype(F32) + F32(0)) + F32(0)
        elif op == "min_image_pk":
            # (a, -a): the same d^2 twice (both roundings are symmetric); the third column is the kernel's to say -- see compare_pk
            r1, r2 = reference("min_image", a, b), reference("min_image", -a, b)
            r = np.stack([r1, r2, np.zeros_like(r1)], axis=1)
        elif op == "wrap_decide":
            # tests/wrap_restatement.py: half = box / 2; diff = centre - box centre; where |diff| > half the translation is
            # float32(float64(box) * round(float64(float32(diff / box)))), else nothing moves
            grp, centre, box = a, b, c
            half = box / F32(2)
            diff = (grp - centre).astype(F32)
            moved = np.abs(diff) > half
            q = (diff / box).astype(F32).astype(F64)
            t = (box.astype(F64) * c_round64(q)).astype(F32)
            r = np.stack([moved.astype(F32), np.where(moved, t, F32(0))], axis=1).astype(F32)
        elif op == "dih_wrap":
            h = (b * F32(0.5)).astype(F32)
            r = np.where(a < -h, a + b, np.where(a > h, a - b, a))
        elif op == "acosf":
            r = RR.acosf(a)
        elif op == "ring_angle":
            r = RR._angle(a)
        else:
            raise KeyError(op)
    from moleculekit_amd._lib import ARITH_OPS
    assert r.dtype == ARITH_OPS[op][3], (op, r.dtype)
    return r


Report = namedtuple("Report", "op elements mismatches first")


def compare(got, exp):
    """-> indexes (of elements) whose result is not the reference's: bit patterns, or NaN for NaN"""
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    u = U32 if exp.dtype == F32 else U64
    g, e = np.ascontiguousarray(got).view(u), np.ascontiguousarray(exp).view(u)
    bad = np.where(np.isnan(exp), ~np.isnan(got), g != e)
    if bad.ndim > 1:
        bad = bad.any(axis=1)
    return np.flatnonzero(bad)


def _hex(x):
    x = np.asarray(x)
    return "0x%08x" % int(x.view(U32)) if x.dtype == F32 else "0x%016x" % int(x.view(U64))


def compare_pk(got, exp):
    """min_image_pk: the third column is 1 (the caller redoes the pair: nothing is claimed of the values) or 0: then both squared
    separations are the reference's.  -> indexes of the elements that break this"""
    redo = got[:, 2]
    ok_flag = (redo == 0) | (redo == 1)
    wrong = np.zeros(len(got), bool)
    wrong[compare(got[:, :2], exp[:, :2])] = True
    return np.flatnonzero(~ok_flag | ((redo == 0) & wrong))


class _Tally:
    def __init__(self, op):
        self.op, self.n, self.bad, self.first = op, 0, 0, None

    def add(self, cols, got, exp):
        idx = compare_pk(got, exp) if self.op == "min_image_pk" else compare(got, exp)
        if idx.size and self.first is None:
            i = int(idx[0])
            self.first = "element %d: inputs %s -> %s, reference %s" % (
                self.n + i, ", ".join(_hex(c[i]) for c in cols), " ".join(_hex(v) for v in np.atleast_1d(got[i])),
                " ".join(_hex(v) for v in np.atleast_1d(exp[i])))
        self.n += cols[0].size
        self.bad += int(idx.size)

    def report(self):
        return Report(self.op, self.n, self.bad, self.first)


def run(probe, op, keep=None):
    """``op`` over all its vectors through ``probe(op, *columns)``.  ``keep``: a list that receives every chunk's result."""
    t = _Tally(op)
    for cols in chunks(op):
        got = probe(op, *cols)
        t.add(cols, got, reference(op, *cols))
        if keep is not None:
            keep.append(got)
    return t.report()


def run_acos(probe):
    """``acosf`` and ``ring_angle`` over ``acos_chunks``, the restated acosf evaluated once per chunk: the angle's reference is that
    value widened, times 57.29578, folded at 90 (rings_restatement._angle, which a slice of every chunk is held against)"""
    ta, tg = _Tally("acosf"), _Tally("ring_angle")
    for cols in acos_chunks():
        exp = RR.acosf(cols[0])
        with np.errstate(all="ignore"):
            ang = exp.astype(F64) * 57.29578
            ang = np.where(ang > 90, 180 - ang, ang)
        assert not compare(ang[:4096], RR._angle(cols[0][:4096])).size
        ta.add(cols, probe("acosf", *cols), exp)
        tg.add(cols, probe("ring_angle", *cols), ang)
    return ta.report(), tg.report()


def describe(reports):
    return "; ".join("%s: %d of %d%s" % (r.op, r.mismatches, r.elements, " (first: %s)" % r.first if r.first else "") for r in reports)


GROUPS = {
    "exact_ops": ("fadd", "fsub", "fmul", "fmul_add", "dmul_add"),
    "divisions": ("fdiv", "ring_div", "ddiv"),
    "roots": ("fsqrt", "ring_sqrt"),
    "roundings": ("roundf", "rint", "dround", "round_quot", "ring_round_quot"),
    "composites": ("min_image", "min_image_pk", "wrap_decide", "dih_wrap"),
}


def check_group(probe, group):
    """every operation of the group: no mismatch; for the root, also the same bits for the ordinary values in both wave layouts"""
    reports = []
    for op in GROUPS[group]:
        keep = [] if op in ("fsqrt", "min_image_pk") else None
        reports.append(run(probe, op, keep))
        # the packed form's test is the stricter one (tm + 3e-7 qm < 0.4999998: q at least 3.5e-7, six float32 steps of 0.5, from the
        # half-integer, where the cases move a by up to six): both outcomes must occur in the ranges with k up to 2 (k = 0 alone, the
        # huge boxes: six steps are just not enough)
        if op == "min_image_pk":
            redo = np.concatenate(keep)[:, 2]
            mi = min_image_cases()
            at = binary32()[0].size + round_quot_cases()[0].size
            for name in MIN_IMAGE_RANGES:
                n = mi[name][0].size
                if name in MIN_IMAGE_RANGES[:2]:
                    assert 0.05 <= 1 - redo[at:at + n].mean() <= 0.95, (name, 1 - redo[at:at + n].mean())
                at += n
        if op == "fsqrt":
            assert len(keep) == 1
            apart = sqrt_layout_disagreements(keep[0])
            assert apart == 0, f"mk_fsqrt_rn: {apart} ordinary values differ between a wave of ordinary values and a wave with a special in it"
    print(describe(reports))
    assert all(r.mismatches == 0 for r in reports), describe(reports)
    assert all(r.elements % 64 for r in reports)
    return reports


def check_acos(probe):
    reports = run_acos(probe)
    print(describe(reports))
    assert all(r.mismatches == 0 for r in reports), describe(reports)
    assert all(r.elements >= (1 << 24) + (1 << 23) for r in reports)
    return reports
