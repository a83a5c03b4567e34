"""tests/within_restatement.py -- TEST INFRASTRUCTURE: the reference's ``atomselect_utils.within_distance`` restated in numpy, float32
operation by operation, the gate included.  tests/golden/make_golden_within.py asserts that it equals the
compiled reference on every golden case; the CPU tier then uses it freely.

numpy's float32 ufuncs round every operation on its own (no multiply-add), which is what the compiled loop does: gcc turns
``powf(x, 2.0)`` into ``x * x`` at -O3, and x86-64 evaluates float expressions in float32.

Also here: the three OTHER formulations a port could fall into (``alt_*``), which tests/within_cases.py tells apart from the reference's.
"""
from fractions import Fraction

import numpy as np

F32 = np.float32


def f32_cutoff(cutoff):
    """the Python float as the C ``float`` argument receives it, and its float32 square"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        c = F32(cutoff)
        return c, F32(c * c)


def gate_open(xyz, mn, mx, cutoff):
    """bool [n]: per query, whether SOME axis has x >= min - cutoff or x <= max + cutoff, float32 as written"""
    c, _ = f32_cutoff(cutoff)
    xyz, mn, mx = np.asarray(xyz, F32), np.asarray(mn, F32), np.asarray(mx, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((xyz >= (mn - c)[None, :]) | (xyz <= (mx + c)[None, :])).any(axis=1)


def pair_diff(q, s):
    """float32 [nq, ns]: ((0 + dx dx) + dy dy) + dz dz, every operation a float32 one"""
    q, s = np.asarray(q, F32), np.asarray(s, F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = q[:, None, :] - s[None, :, :]
        sq = d * d
        return ((F32(0) + sq[..., 0]) + sq[..., 1]) + sq[..., 2]


def hits(q, s, cutoff, chunk=512):
    """bool [nq]: any source with diff < sq_cutoff"""
    _, sq_cutoff = f32_cutoff(cutoff)
    q, s = np.asarray(q, F32).reshape(-1, 3), np.asarray(s, F32).reshape(-1, 3)
    out = np.zeros(len(q), bool)
    for a in range(0, len(q), chunk):
        for b in range(0, len(s), 4096):
            with np.errstate(invalid="ignore"):
                out[a:a + chunk] |= (pair_diff(q[a:a + chunk], s[b:b + 4096]) < sq_cutoff).any(axis=1)
    return out


def within_distance(coords, cutoff, sel1, sel2, sel2_min_coords, sel2_max_coords, results):
    """the reference's signature: ``coords`` float32 [N, 3] of one frame; ORs into ``results`` in place"""
    coords = np.asarray(coords, F32)
    sel1, sel2 = np.asarray(sel1, np.int64), np.asarray(sel2, np.int64)
    if len(sel1) == 0:
        return
    q = coords[sel1]
    found = gate_open(q, sel2_min_coords, sel2_max_coords, cutoff) & hits(q, coords[sel2], cutoff)
    results |= found


def frames(coords, sel1, sel2, cutoff, gate=None, preset=None):
    """coords float32 [F, N, 3]; gate (min [F, 3], max [F, 3]) or None (no gate); preset bool [F, n1] or None -> bool [F, n1]"""
    coords = np.asarray(coords, F32)
    out = np.zeros((coords.shape[0], len(sel1)), bool) if preset is None else np.array(preset, bool)
    for f in range(coords.shape[0]):
        if gate is None:
            if len(sel1):
                out[f] |= hits(coords[f][np.asarray(sel1, np.int64)], coords[f][np.asarray(sel2, np.int64)], cutoff)
        else:
            within_distance(coords[f], cutoff, sel1, sel2, gate[0][f], gate[1][f], out[f])
    return out


# ------------------------------------------------------------------------------------------------
# what the reference is NOT (tests/within_cases.py: rounding_tellers), per single pair
# ------------------------------------------------------------------------------------------------
def round_f32(q):
    """the float32 nearest to the exact rational ``q``, ties to even"""
    r = F32(float(q))
    best = None
    for cand in (np.nextafter(r, F32(-np.inf)), r, np.nextafter(r, F32(np.inf))):
        err = abs(Fraction(float(cand)) - q)
        even = (int(np.array(cand, F32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, cand)
    return best[1]


def alt_float64(q, s, cutoff):
    """the sum in float64 over the widened coordinates, against the float32 square widened"""
    _, sq = f32_cutoff(cutoff)
    d = np.asarray(q, np.float64) - np.asarray(s, np.float64)
    return bool((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] < np.float64(sq))


def alt_fused(q, s, cutoff):
    """acc = fma(d, d, acc) in float32, d the float32 difference: one rounding per axis (exact rational arithmetic, rounded once)"""
    _, sq = f32_cutoff(cutoff)
    d = np.asarray(q, F32) - np.asarray(s, F32)
    acc = F32(0)
    for k in range(3):
        acc = round_f32(Fraction(float(d[k])) ** 2 + Fraction(float(acc)))
    return bool(acc < sq)


def alt_double_square(q, s, cutoff):
    """diff = float32(double(diff) + double(d) * double(d)): what ``powf`` through a double would give"""
    _, sq = f32_cutoff(cutoff)
    d = np.asarray(q, F32) - np.asarray(s, F32)
    acc = F32(0)
    for k in range(3):
        acc = F32(np.float64(acc) + np.float64(d[k]) * np.float64(d[k]))
    return bool(acc < sq)


ALTERNATIVES = {"float64": alt_float64, "fused": alt_fused, "double_square": alt_double_square}
