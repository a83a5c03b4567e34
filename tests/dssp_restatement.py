"""tests/dssp_restatement.py -- TEST INFRASTRUCTURE: Kabsch and Sander's DSSP as DESIGN.md section 19 states it, in numpy float32,
operation for operation (every product, sum, root and quotient rounded once; squared lengths x x + y y + z z left to right).

``dssp(coords, ca, nco, proline, chain)`` -> (slot acceptors int32 [F, R, 2], slot energies float32 [F, R, 2], full codes uint8
[F, R]).  ``literal=True`` walks the pairs and the bridge windows as the rules are written (the donors meet their acceptors in
ascending order; rule 4's double loop); the default takes the two smallest (E, acceptor) per donor and the bridge candidates from the
slots, which the rules say are the same -- the tests check that they are.  Never imported by the product.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
H, B, E, G, I, T, S, BLANK = 3, 4, 5, 6, 7, 8, 9, 10
LETTERS = {H: "H", B: "B", E: "E", G: "G", I: "I", T: "T", S: "S", BLANK: " "}
SIMPLE = np.zeros(11, np.uint8)
SIMPLE[[H, G, I]] = 2
SIMPLE[[E, B]] = 1
PAR, ANTI = 0, 1


def simplify(full):
    return SIMPLE[np.asarray(full)]


def _sq(d):
    """[..., 3] float32 -> x x + y y + z z, left to right"""
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def backbone(xyz, ca, nco, chain):
    """xyz float32 [N, 3] -> N, CA, C, O, H float32 [R, 3] (rule 1)"""
    xyz = np.asarray(xyz, F32)
    Nn, CA, C, O = xyz[nco[:, 0]], xyz[ca], xyz[nco[:, 1]], xyz[nco[:, 2]]
    Hh = Nn.copy()
    with np.errstate(all="ignore"):
        for r in range(1, len(ca)):
            if chain[r] != chain[r - 1]:
                continue
            v = C[r - 1] - O[r - 1]
            l2 = _sq(v)
            if l2 == 0:
                continue
            Hh[r] = Nn[r] + v / np.sqrt(l2)
    return Nn, CA, C, O, Hh


def _energy(Hd, Nd, Oa, Ca):
    """rule 2 on broadcastable [..., 3] arrays"""
    with np.errstate(all="ignore"):
        dHO, dHC = np.sqrt(_sq(Hd - Oa)), np.sqrt(_sq(Hd - Ca))
        dNC, dNO = np.sqrt(_sq(Nd - Ca)), np.sqrt(_sq(Nd - Oa))
        one = F32(1.0)
        e = F32(-27.888) * (((one / dHO - one / dHC) + one / dNC) - one / dNO)
        e = np.where(e < F32(-9.9), F32(-9.9), e)
        close = (dHO < F32(0.5)) | (dHC < F32(0.5)) | (dNC < F32(0.5)) | (dNO < F32(0.5))
        return np.where(close, F32(-9.9), e).astype(F32)


def slots_of_frame(bb, proline, literal=False):
    Nn, CA, C, O, Hh = bb
    R = len(CA)
    sa = np.full((R, 2), -1, np.int32)
    se = np.zeros((R, 2), F32)
    if R == 0:
        return sa, se
    with np.errstate(all="ignore"):
        near = _sq(CA[:, None, :] - CA[None, :, :]) < F32(81.0)
    if literal:
        def offer(d, a):
            if proline[d]:
                return
            e = _energy(Hh[d], Nn[d], O[a], C[a])
            if e < se[d, 0]:
                sa[d, 1], se[d, 1] = sa[d, 0], se[d, 0]
                sa[d, 0], se[d, 0] = a, e
            elif e < se[d, 1]:
                sa[d, 1], se[d, 1] = a, e
        for i in range(R):
            for j in range(i + 1, R):
                if near[i, j]:
                    offer(i, j)
                    if j != i + 1:
                        offer(j, i)
        return sa, se
    e = _energy(Hh[:, None, :], Nn[:, None, :], O[None, :, :], C[None, :, :])          # [donor, acceptor]
    d, a = np.arange(R)[:, None], np.arange(R)[None, :]
    with np.errstate(invalid="ignore"):
        ok = near & (a != d) & (a != d - 1) & ~np.asarray(proline, bool)[:, None] & (e < 0)
    key = np.where(ok, e, np.inf)
    order = np.argsort(key, axis=1, kind="stable")[:, :2]                               # ties: the lower acceptor
    for k in range(min(2, R)):
        pick = order[:, k]
        good = ok[np.arange(R), pick]
        sa[good, k] = pick[good]
        se[good, k] = e[np.arange(R), pick][good]
    return sa, se


def _u32(x):
    return int(x) & 0xFFFFFFFF


def labels_of_frame(sa, se, chain, CA, literal=False, trace=None):
    """rules 4 to 6 -> full codes uint8 [R]; trace (a dict) receives the ladders before and after the merge"""
    R = len(chain)
    ss = np.full(R, BLANK, np.uint8)
    bonded = [{int(sa[x, k]) for k in range(2) if sa[x, k] >= 0 and se[x, k] < F32(-0.5)} for x in range(R)]

    def hb(x, y):
        return y in bonded[x]

    def same(a, b):
        return all(chain[k] == chain[a] for k in range(a, b + 1))

    # rule 4
    def kind(i, j):
        a, b, c, d, e, f = i - 1, i, i + 1, j - 1, j, j + 1
        if not (same(a, c) and same(d, f)):
            return None
        if (hb(c, e) and hb(e, a)) or (hb(f, b) and hb(b, d)):
            return PAR
        if (hb(c, d) and hb(f, a)) or (hb(e, b) and hb(b, e)):
            return ANTI
        return None

    bridges = {}
    for i in range(1, R - 4):
        if literal:
            js = range(i + 3, R - 1)
        else:
            js = sorted({int(sa[x, k]) + o for x in (i, i + 1) for k in range(2) if sa[x, k] >= 0 for o in (0, 1)})
            js = [j for j in js if i + 3 <= j <= R - 2]
        for j in js:
            t = kind(i, j)
            if t is not None:
                bridges[(i, j)] = t
    # rule 5: maximal runs, in the order (first i, j of the bridge at that first i)
    ladders = []
    for (i, j), t in sorted(bridges.items()):
        step = 1 if t == PAR else -1
        if bridges.get((i - 1, j - step)) == t:
            continue
        li, lj = [i], [j]
        while bridges.get((li[-1] + 1, lj[-1] + step)) == t:
            li.append(li[-1] + 1)
            lj.append(lj[-1] + step)
        ladders.append({"t": t, "i": li, "j": sorted(lj)})
    if trace is not None:
        trace["ladders"] = [dict(l, i=list(l["i"]), j=list(l["j"])) for l in ladders]
        trace["merges"] = []
    p = 0
    while p < len(ladders):
        q = p + 1
        while q < len(ladders):
            lp, lq = ladders[p], ladders[q]
            ibi, iei, jbi, jei = lp["i"][0], lp["i"][-1], lp["j"][0], lp["j"][-1]
            ibj, iej, jbj, jej = lq["i"][0], lq["i"][-1], lq["j"][0], lq["j"][-1]
            if (lp["t"] != lq["t"] or not same(min(ibi, ibj), max(iei, iej)) or not same(min(jbi, jbj), max(jei, jej))
                    or _u32(ibj - iei) >= 6 or (iei >= ibj and ibi <= iej)):
                q += 1
                continue
            if lp["t"] == PAR:
                bulge = (_u32(jbj - jei) < 6 and _u32(ibj - iei) < 3) or _u32(jbj - jei) < 3
            else:
                bulge = (_u32(jbi - jej) < 6 and _u32(ibj - iei) < 3) or _u32(jbi - jej) < 3
            if trace is not None and (jbj - jei if lp["t"] == PAR else jbi - jej) < 0:
                trace["negative"] = trace.get("negative", 0) + 1    # the unsigned rule decides: a signed test would merge
            if not bulge:
                q += 1
                continue
            lp["i"] = lp["i"] + lq["i"]
            lp["j"] = lp["j"] + lq["j"] if lp["t"] == PAR else lq["j"] + lp["j"]
            if trace is not None:
                trace["merges"].append((p, q, lp["t"], jbj - jei if lp["t"] == PAR else jbi - jej))
            del ladders[q]
        p += 1
    for l in ladders:
        code = E if len(l["i"]) > 1 else B
        for lo, hi in ((l["i"][0], l["i"][-1]), (l["j"][0], l["j"][-1])):
            for r in range(lo, hi + 1):
                if code == E or ss[r] != E:
                    ss[r] = code
    # rule 6
    def turn(s, i):
        return 0 <= i < R - s and hb(i + s, i) and same(i, i + s)

    for i in range(1, R - 4):
        if turn(4, i - 1) and turn(4, i):
            ss[i:i + 4] = H
    for i in range(1, R - 3):
        if turn(3, i - 1) and turn(3, i) and all(ss[k] in (BLANK, G) for k in range(i, i + 3)):
            ss[i:i + 3] = G
    for i in range(1, R - 5):
        if turn(5, i - 1) and turn(5, i) and all(ss[k] in (BLANK, I, H) for k in range(i, i + 5)):
            ss[i:i + 5] = I
    bend = np.zeros(R, bool)
    with np.errstate(all="ignore"):
        for i in range(2, R - 2):
            if not same(i - 2, i + 2):
                continue
            u, v = CA[i] - CA[i - 2], CA[i + 2] - CA[i]
            prod = _sq(u) * _sq(v)
            c = F32(0.0) if prod == 0 else ((u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]) / np.sqrt(prod)
            bend[i] = bool(c < F32(0.34202014))
    for i in range(1, R - 1):
        if ss[i] != BLANK:
            continue
        if any(turn(s, i - k) for s in (3, 4, 5) for k in range(1, s) if i - k >= 0):
            ss[i] = T
        elif bend[i]:
            ss[i] = S
    return ss


def dssp(coords, ca, nco, proline, chain, literal=False, traces=None):
    coords = np.asarray(coords, F32)
    if coords.ndim == 2:
        coords = coords[:, :, None]
    ca, nco = np.asarray(ca, np.int64), np.asarray(nco, np.int64).reshape(-1, 3)
    F_, R = coords.shape[2], len(ca)
    sa = np.full((F_, R, 2), -1, np.int32)
    se = np.zeros((F_, R, 2), F32)
    full = np.full((F_, R), BLANK, np.uint8)
    for f in range(F_):
        bb = backbone(coords[:, :, f], ca, nco, chain)
        sa[f], se[f] = slots_of_frame(bb, proline, literal)
        tr = {} if traces is not None else None
        full[f] = labels_of_frame(sa[f], se[f], chain, bb[1], literal, tr)
        if traces is not None:
            traces.append(tr)
    return sa, se, full
