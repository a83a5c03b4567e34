// dssp_kernels.h -- HIP kernels of MetricSecondaryStructure on MI355X (gfx950): Kabsch and Sander's DSSP of every frame of a
// trajectory (which states the rules these kernels follow by number).
//
// A call works through its frames in chunks of Fc.  Everything between the kernels lives in a FRAME-MINOR workspace, [..][R][Fc]:
// lanes along frames load and store neighbours.
//   k_dssp_segments        run_start[r]: the first residue of the run of equal chain ids r sits in -- same(a, b) is run_start[b] <= a
//   k_dssp_backbone        N, CA, C, O gathered from the [N, 3, F] coordinates, the amide H of rule 1              bb [15][R][Fc]
//   k_dssp_energy_frames   lanes along FRAMES: a lane owns (frame, donor) and meets the acceptors in ascending order: rule 3 as written
//   k_dssp_energy_atoms    lanes along the ACCEPTORS of one (frame, donor): every lane the two best of its acceptors, then the wave's
//                          two best by a butterfly on (E, acceptor) keys -- a total order, so both plans give the same slots
//                          slot_a, slot_e [2][R][Fc]; hba [2][R][Fc]: the slot's acceptor where E < -0.5, else -1
//   k_dssp_local           per (frame, residue): the n-turns and the bend (flags), the bridges of rule 4 from the slot candidates
//                          flags [R][Fc], nbr [R][Fc], br [8][R][Fc] (partner j | antiparallel << 31, ascending)
//   k_dssp_sheets          a lane per frame: ladders, the greedy bulge merge and the E / B labels of rule 5, then H of rule 6
//   k_dssp_helix3          per (frame, residue): G of rule 6, from the labels after H into a second plane
//   k_dssp_finish          per (frame, residue): I, T, S of rule 6, the code, the [F, R] result (lanes along residues: rows out)
// The energies are float32 with every operation rounded once (mk_f*_rn), roots and quotients correctly rounded.  No atomics, no
// floating-point reduction: the same bits on every run.  Every loop is bounded by R or by a table's size.
#pragma once
#include "dist_kernels.h"

namespace mkamd {

enum { SS_H = 3, SS_B = 4, SS_E = 5, SS_G = 6, SS_I = 7, SS_T = 8, SS_S = 9, SS_BLANK = 10 };
enum { SS_TURN3 = 1, SS_TURN4 = 2, SS_TURN5 = 4, SS_BEND = 8 };
constexpr int SS_BRIDGES = 8;               // bridge partners j > i of a residue i: four slots name two candidates each (rule 4)
constexpr unsigned SS_ANTI = 0x80000000u;

// the chunk's workspace; L: ladders a frame's table holds (8 R: a ladder starts at a bridge, so the table cannot overflow)
struct DsspWs {
    long long R, Fc, L;
    const int* run_start;
    float* bb;
    int* slot_a; float* slot_e; int* hba;
    unsigned char *flags, *nbr, *label;
    unsigned* br;
    int* lad;
};

enum { SS_PN = 0, SS_PCA = 3, SS_PC = 6, SS_PO = 9, SS_PH = 12 };
MK_DEV size_t ss_at(const DsspWs& w, long long plane, long long r, long long f) { return ((size_t)plane * (size_t)w.R + (size_t)r) * (size_t)w.Fc + (size_t)f; }
MK_DEV bool ss_same(const DsspWs& w, long long a, long long b) { return (long long)w.run_start[b] <= a; }       // a <= b

// one wave: run_start by 64 residues at a time (the last break at or below a lane, else the carry)
MK_KERNEL(64) void k_dssp_segments(const int* __restrict__ chain, long long R, int* __restrict__ run_start)
{
    const int lane = threadIdx.x & (WAVE - 1);
    long long carry = 0;
    for (long long base = 0; base < R; base += WAVE) {
        const long long r = base + lane;
        const bool brk = r < R && (r == 0 || chain[r] != chain[r - 1]);
        const unsigned long long mask = mk_ballot(brk);
        const unsigned long long below = mask & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        if (r < R) run_start[r] = (int)(below ? base + 63 - mk_clz64(below) : carry);
        if (mask) carry = base + 63 - mk_clz64(mask);
    }
}

constexpr int SSB_THREADS = 256;

// thread -> (frame f of the chunk, residue r), frames fastest
MK_KERNEL(SSB_THREADS) void k_dssp_backbone(DsspWs w, const float* __restrict__ coords, long long F, long long f0, const unsigned* __restrict__ ca,
                                            const unsigned* __restrict__ nco, const int* __restrict__ chain)
{
    const long long t = (long long)blockIdx.x * SSB_THREADS + threadIdx.x;
    if (t >= w.R * w.Fc) return;
    const long long f = t % w.Fc, r = t / w.Fc;
    auto at = [&](unsigned atom, int ax) { return coords[((size_t)atom * 3 + (size_t)ax) * (size_t)F + (size_t)(f0 + f)]; };
    const unsigned an = nco[3 * r], ac = nco[3 * r + 1], ao = nco[3 * r + 2], aa = ca[r];
    float n[3], h[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        n[ax] = h[ax] = at(an, ax);
        w.bb[ss_at(w, SS_PN + ax, r, f)] = n[ax];
        w.bb[ss_at(w, SS_PCA + ax, r, f)] = at(aa, ax);
        w.bb[ss_at(w, SS_PC + ax, r, f)] = at(ac, ax);
        w.bb[ss_at(w, SS_PO + ax, r, f)] = at(ao, ax);
    }
    if (r > 0 && chain[r] == chain[r - 1]) {                        // rule 1
        const unsigned pc = nco[3 * (r - 1) + 1], po = nco[3 * (r - 1) + 2];
        float v[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) v[ax] = mk_fsub_rn(at(pc, ax), at(po, ax));
        const float l2 = mk_fadd_rn(mk_fadd_rn(mk_fmul_rn(v[0], v[0]), mk_fmul_rn(v[1], v[1])), mk_fmul_rn(v[2], v[2]));
        if (!(l2 == 0.0f)) {
            const float len = mk_fsqrt_rn(l2);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) h[ax] = mk_fadd_rn(n[ax], mk_fdiv_rn(v[ax], len));
        }
    }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) w.bb[ss_at(w, SS_PH + ax, r, f)] = h[ax];
}

MK_DEV float ss_sq(const float (&a)[3], const float (&b)[3])
{
    const float x = mk_fsub_rn(a[0], b[0]), y = mk_fsub_rn(a[1], b[1]), z = mk_fsub_rn(a[2], b[2]);
    return mk_fadd_rn(mk_fadd_rn(mk_fmul_rn(x, x), mk_fmul_rn(y, y)), mk_fmul_rn(z, z));
}

// rule 2
MK_DEV float ss_energy(const float (&hd)[3], const float (&nd)[3], const float (&oa)[3], const float (&ca)[3])
{
    const float dho = mk_fsqrt_rn(ss_sq(hd, oa)), dhc = mk_fsqrt_rn(ss_sq(hd, ca));
    const float dnc = mk_fsqrt_rn(ss_sq(nd, ca)), dno = mk_fsqrt_rn(ss_sq(nd, oa));
    const bool close = dho < 0.5f || dhc < 0.5f || dnc < 0.5f || dno < 0.5f;
    const float s = mk_fsub_rn(mk_fadd_rn(mk_fsub_rn(mk_fdiv_rn(1.0f, dho), mk_fdiv_rn(1.0f, dhc)), mk_fdiv_rn(1.0f, dnc)), mk_fdiv_rn(1.0f, dno));
    float e = mk_fmul_rn(-27.888f, s);
    e = e < -9.9f ? -9.9f : e;                                      // (a NaN stays one)
    return close ? -9.9f : e;
}

struct SsSlots { int a0, a1; float e0, e1; };
MK_DEV SsSlots ss_empty() { return SsSlots{-1, -1, 0.0f, 0.0f}; }
MK_DEV void ss_offer(SsSlots& s, int a, float e)                    // rule 3's update
{
    if (e < s.e0) { s.a1 = s.a0; s.e1 = s.e0; s.a0 = a; s.e0 = e; }
    else if (e < s.e1) { s.a1 = a; s.e1 = e; }
}
MK_DEV void ss_load3(const DsspWs& w, int plane, long long r, long long f, float (&v)[3])
{
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) v[ax] = w.bb[ss_at(w, plane + ax, r, f)];
}
MK_DEV void ss_store_slots(const DsspWs& w, long long d, long long f, const SsSlots& s)
{
    w.slot_a[ss_at(w, 0, d, f)] = s.a0; w.slot_e[ss_at(w, 0, d, f)] = s.e0;
    w.slot_a[ss_at(w, 1, d, f)] = s.a1; w.slot_e[ss_at(w, 1, d, f)] = s.e1;
    w.hba[ss_at(w, 0, d, f)] = s.e0 < -0.5f ? s.a0 : -1;
    w.hba[ss_at(w, 1, d, f)] = s.e1 < -0.5f ? s.a1 : -1;
}

constexpr int SSE_THREADS = 256;

// Lanes along frames.  A wave: 64 frames of ONE donor (wave-uniform: its proline gate and the acceptor loop do not diverge); the
// waves of a block take neighbouring donors over the same frames.  Per acceptor three coalesced loads (CA) and the 9 A test; the
// few that pass load O and C and pay for the energy.
MK_KERNEL(SSE_THREADS) void k_dssp_energy_frames(DsspWs w, const int* __restrict__ proline)
{
    const long long slabs = (w.Fc + WAVE - 1) / WAVE, tasks = slabs * w.R;
    const long long task = (long long)blockIdx.x * (SSE_THREADS / WAVE) + (long long)mk_uniform(threadIdx.x >> 6);
    if (task >= tasks) return;                                      // (the whole wave)
    const int lane = threadIdx.x & (WAVE - 1);
    const long long d = task % w.R, f0 = (task / w.R) * WAVE;
    const long long f = f0 + lane < w.Fc ? f0 + lane : w.Fc - 1;    // frames past the end compute on the last one (never stored)
    SsSlots s = ss_empty();
    if (!proline[d]) {
        float nd[3], hd[3], cd[3];
        ss_load3(w, SS_PN, d, f, nd); ss_load3(w, SS_PH, d, f, hd); ss_load3(w, SS_PCA, d, f, cd);
#pragma unroll 1
        for (long long a = 0; a < w.R; ++a) {
            if (a == d || a == d - 1) continue;
            float ca[3];
            ss_load3(w, SS_PCA, a, f, ca);
            if (ss_sq(cd, ca) < 81.0f) {
                float oa[3], cc[3];
                ss_load3(w, SS_PO, a, f, oa); ss_load3(w, SS_PC, a, f, cc);
                ss_offer(s, (int)a, ss_energy(hd, nd, oa, cc));
            }
        }
    }
    if (f0 + lane < w.Fc) ss_store_slots(w, d, f, s);
}

// (E, acceptor) keys: the lower energy, then the lower acceptor; an empty slot (0, -1) loses to every real one (E < 0)
MK_DEV bool ss_before(float ea, int aa, float eb, int ab) { return ea < eb || (ea == eb && (unsigned)aa < (unsigned)ab); }

// Lanes along the acceptors of ONE (frame, donor): lane k takes acceptors k, k + 64, ... in ascending order (its own two best by
// rule 3's update), then six butterfly steps leave the wave's two best in every lane.
MK_KERNEL(SSE_THREADS) void k_dssp_energy_atoms(DsspWs w, const int* __restrict__ proline)
{
    const long long tasks = w.Fc * w.R;
    const long long task = (long long)blockIdx.x * (SSE_THREADS / WAVE) + (long long)mk_uniform(threadIdx.x >> 6);
    if (task >= tasks) return;                                      // (the whole wave)
    const int lane = threadIdx.x & (WAVE - 1);
    const long long d = task % w.R, f = task / w.R;
    SsSlots s = ss_empty();
    if (!proline[d]) {                                              // (wave-uniform)
        float nd[3], hd[3], cd[3];
        ss_load3(w, SS_PN, d, f, nd); ss_load3(w, SS_PH, d, f, hd); ss_load3(w, SS_PCA, d, f, cd);
#pragma unroll 1
        for (long long a = lane; a < w.R; a += WAVE) {
            if (a == d || a == d - 1) continue;
            float ca[3];
            ss_load3(w, SS_PCA, a, f, ca);
            if (ss_sq(cd, ca) < 81.0f) {
                float oa[3], cc[3];
                ss_load3(w, SS_PO, a, f, oa); ss_load3(w, SS_PC, a, f, cc);
                ss_offer(s, (int)a, ss_energy(hd, nd, oa, cc));
            }
        }
#pragma unroll
        for (int m = 1; m < WAVE; m <<= 1) {
            SsSlots o;
            o.a0 = (int)mk_shfl((unsigned)s.a0, lane ^ m); o.e0 = mk_uint_as_float(mk_shfl(mk_float_bits(s.e0), lane ^ m));
            o.a1 = (int)mk_shfl((unsigned)s.a1, lane ^ m); o.e1 = mk_uint_as_float(mk_shfl(mk_float_bits(s.e1), lane ^ m));
            SsSlots r;
            if (ss_before(s.e0, s.a0, o.e0, o.a0)) {
                const bool mine = ss_before(s.e1, s.a1, o.e0, o.a0);
                r = SsSlots{s.a0, mine ? s.a1 : o.a0, s.e0, mine ? s.e1 : o.e0};
            } else {
                const bool theirs = ss_before(o.e1, o.a1, s.e0, s.a0);
                r = SsSlots{o.a0, theirs ? o.a1 : s.a0, o.e0, theirs ? o.e1 : s.e0};
            }
            s = r;
        }
    }
    if (lane == 0) ss_store_slots(w, d, f, s);
}

MK_DEV bool ss_hb(const DsspWs& w, long long x, long long y, long long f)
{
    return (long long)w.hba[ss_at(w, 0, x, f)] == y || (long long)w.hba[ss_at(w, 1, x, f)] == y;
}

constexpr int SSL_THREADS = 256;

// thread -> (frame, residue i), frames fastest: the flags of i and its bridges (i, j), j ascending
MK_KERNEL(SSL_THREADS) void k_dssp_local(DsspWs w)
{
    const long long t = (long long)blockIdx.x * SSL_THREADS + threadIdx.x;
    if (t >= w.R * w.Fc) return;
    const long long f = t % w.Fc, i = t / w.Fc, R = w.R;
    unsigned flags = 0;
#pragma unroll
    for (int s = 3; s <= 5; ++s)
        if (i < R - s && ss_hb(w, i + s, i, f) && ss_same(w, i, i + s)) flags |= 1u << (s - 3);
    if (i >= 2 && i <= R - 3 && ss_same(w, i - 2, i + 2)) {         // the bend of rule 6
        float a[3], b[3], c[3];
        ss_load3(w, SS_PCA, i - 2, f, a); ss_load3(w, SS_PCA, i, f, b); ss_load3(w, SS_PCA, i + 2, f, c);
        const float u[3] = {mk_fsub_rn(b[0], a[0]), mk_fsub_rn(b[1], a[1]), mk_fsub_rn(b[2], a[2])};
        const float v[3] = {mk_fsub_rn(c[0], b[0]), mk_fsub_rn(c[1], b[1]), mk_fsub_rn(c[2], b[2])};
        const float uu = mk_fadd_rn(mk_fadd_rn(mk_fmul_rn(u[0], u[0]), mk_fmul_rn(u[1], u[1])), mk_fmul_rn(u[2], u[2]));
        const float vv = mk_fadd_rn(mk_fadd_rn(mk_fmul_rn(v[0], v[0]), mk_fmul_rn(v[1], v[1])), mk_fmul_rn(v[2], v[2]));
        const float uv = mk_fadd_rn(mk_fadd_rn(mk_fmul_rn(u[0], v[0]), mk_fmul_rn(u[1], v[1])), mk_fmul_rn(u[2], v[2]));
        const float prod = mk_fmul_rn(uu, vv);
        const float c_ = prod == 0.0f ? 0.0f : mk_fdiv_rn(uv, mk_fsqrt_rn(prod));
        if (c_ < 0.34202014f) flags |= SS_BEND;
    }
    w.flags[ss_at(w, 0, i, f)] = (unsigned char)flags;
    int n = 0;
    if (i >= 1 && i <= R - 5 && ss_same(w, i - 1, i + 1)) {
        // every condition of rule 4 names a bond whose donor is i or i + 1: acceptor y of donor i + 1 -> j = y (parallel) or y + 1
        // (antiparallel), of donor i -> j = y + 1 or y
        long long cand[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long y = w.hba[ss_at(w, k & 1, i + (k >> 1), f)];
            cand[2 * k] = y < 0 ? -1 : y;
            cand[2 * k + 1] = y < 0 ? -1 : y + 1;
        }
        long long last = i + 2;                                      // j >= i + 3
#pragma unroll
        for (int round = 0; round < 8; ++round) {                   // ascending, each once
            long long j = R;
#pragma unroll
            for (int k = 0; k < 8; ++k) j = cand[k] > last && cand[k] < j ? cand[k] : j;
            if (j <= R - 2) {
                last = j;
                if (ss_same(w, j - 1, j + 1)) {
                    const long long a = i - 1, b = i, c = i + 1, d = j - 1, e = j, g = j + 1;
                    const bool par = (ss_hb(w, c, e, f) && ss_hb(w, e, a, f)) || (ss_hb(w, g, b, f) && ss_hb(w, b, d, f));
                    const bool anti = !par && ((ss_hb(w, c, d, f) && ss_hb(w, g, a, f)) || (ss_hb(w, e, b, f) && ss_hb(w, b, e, f)));
                    if (par || anti) {
                        w.br[ss_at(w, n, i, f)] = (unsigned)j | (anti ? SS_ANTI : 0u);
                        ++n;
                    }
                }
            } else last = R;                                         // none left
        }
    }
    w.nbr[ss_at(w, 0, i, f)] = (unsigned char)n;
}

MK_DEV bool ss_is_bridge(const DsspWs& w, long long i, unsigned key, long long f)
{
    const int n = w.nbr[ss_at(w, 0, i, f)];
    bool hit = false;
    for (int m = 0; m < n; ++m) hit = hit || w.br[ss_at(w, m, i, f)] == key;
    return hit;
}

enum { SS_LIB = 0, SS_LIE = 1, SS_LJB = 2, SS_LJE = 3, SS_LTN = 4 };     // a ladder: first and last i and j, type << 31 | entries of i (0: merged away)
constexpr int SSS_THREADS = 64;

// A lane per frame.  Ladders are found in the order rule 5 sorts them in (first i, then the j of the bridge there).  The greedy
// merge of a ladder p stops at the first later ladder that starts 6 or more residues behind p's last i: the ladders are sorted by
// their first i, so every ladder after it fails the same test.
MK_KERNEL(SSS_THREADS) void k_dssp_sheets(DsspWs w)
{
    const long long f = (long long)blockIdx.x * SSS_THREADS + threadIdx.x;
    if (f >= w.Fc) return;
    const long long R = w.R, L = w.L;
    auto lad = [&](int field, long long l) -> int& { return w.lad[((size_t)field * (size_t)L + (size_t)l) * (size_t)w.Fc + (size_t)f]; };
    for (long long r = 0; r < R; ++r) w.label[ss_at(w, 0, r, f)] = SS_BLANK;
    long long nl = 0;
    for (long long i = 1; i <= R - 5; ++i) {
        const int n = w.nbr[ss_at(w, 0, i, f)];
        for (int k = 0; k < n; ++k) {
            const unsigned v = w.br[ss_at(w, k, i, f)];
            const unsigned type = v & SS_ANTI;
            const long long j = (long long)(v & ~SS_ANTI), step = type ? -1 : 1;
            if (i > 1 && ss_is_bridge(w, i - 1, (unsigned)(j - step) | type, f)) continue;      // inside a run
            long long li = i, lj = j;
            while (li + 1 <= R - 5 && lj + step >= 0 && ss_is_bridge(w, li + 1, (unsigned)(lj + step) | type, f)) { ++li; lj += step; }
            if (nl < L) {
                lad(SS_LIB, nl) = (int)i; lad(SS_LIE, nl) = (int)li;
                lad(SS_LJB, nl) = (int)(j < lj ? j : lj); lad(SS_LJE, nl) = (int)(j < lj ? lj : j);
                lad(SS_LTN, nl) = (int)(type | (unsigned)(li - i + 1));
                ++nl;
            }
        }
    }
    for (long long p = 0; p < nl; ++p) {
        const unsigned tp = (unsigned)lad(SS_LTN, p);
        unsigned ni = tp & ~SS_ANTI;
        if (ni == 0) continue;
        const int ibi = lad(SS_LIB, p);
        int iei = lad(SS_LIE, p), jbi = lad(SS_LJB, p), jei = lad(SS_LJE, p);
        for (long long q = p + 1; q < nl; ++q) {
            const int ibj = lad(SS_LIB, q);
            if (ibj - iei >= 6) break;
            const unsigned tq = (unsigned)lad(SS_LTN, q);
            if ((tq & ~SS_ANTI) == 0 || ((tq ^ tp) & SS_ANTI) || ibj - iei < 0) continue;
            const int iej = lad(SS_LIE, q), jbj = lad(SS_LJB, q), jej = lad(SS_LJE, q);
            if (iei >= ibj && ibi <= iej) continue;
            if (!ss_same(w, ibi < ibj ? ibi : ibj, iei > iej ? iei : iej) || !ss_same(w, jbi < jbj ? jbi : jbj, jei > jej ? jei : jej)) continue;
            const unsigned di = (unsigned)(ibj - iei), dj = (tp & SS_ANTI) ? (unsigned)(jbi - jej) : (unsigned)(jbj - jei);
            if (!((dj < 6u && di < 3u) || dj < 3u)) continue;
            iei = iej;
            if (tp & SS_ANTI) jbi = jbj; else jei = jej;
            ni += tq & ~SS_ANTI;
            lad(SS_LTN, q) = (int)(tq & SS_ANTI);
        }
        lad(SS_LIE, p) = iei; lad(SS_LJB, p) = jbi; lad(SS_LJE, p) = jei;
        lad(SS_LTN, p) = (int)((tp & SS_ANTI) | ni);
    }
    for (long long p = 0; p < nl; ++p) {
        const unsigned ni = (unsigned)lad(SS_LTN, p) & ~SS_ANTI;
        if (ni == 0) continue;
        for (int side = 0; side < 2; ++side) {
            long long lo = lad(side ? SS_LJB : SS_LIB, p), hi = lad(side ? SS_LJE : SS_LIE, p);
            hi = hi < R ? hi : R - 1;
            for (long long r = lo < 0 ? 0 : lo; r <= hi; ++r) {
                unsigned char& c = w.label[ss_at(w, 0, r, f)];
                if (ni > 1) c = SS_E; else if (c != SS_E) c = SS_B;
            }
        }
    }
    for (long long i = 1; i <= R - 5; ++i)                          // H overwrites E and B
        if ((w.flags[ss_at(w, 0, i - 1, f)] & SS_TURN4) && (w.flags[ss_at(w, 0, i, f)] & SS_TURN4))
            for (int k = 0; k < 4; ++k) w.label[ss_at(w, 0, i + k, f)] = SS_H;
}

// G: a residue r takes it from a window i..i+2 that holds it, two consecutive 3-turns in front, all three residues still blank
// after H (a G written by another window was blank then: the sequential rule allows it for the same reason).  Plane 0 -> plane 1.
MK_KERNEL(SSL_THREADS) void k_dssp_helix3(DsspWs w)
{
    const long long t = (long long)blockIdx.x * SSL_THREADS + threadIdx.x;
    if (t >= w.R * w.Fc) return;
    const long long f = t % w.Fc, r = t / w.Fc, R = w.R;
    unsigned char c = w.label[ss_at(w, 0, r, f)];
    for (long long i = r - 2 < 1 ? 1 : r - 2; i <= r && i <= R - 4; ++i) {
        if (!((w.flags[ss_at(w, 0, i - 1, f)] & SS_TURN3) && (w.flags[ss_at(w, 0, i, f)] & SS_TURN3))) continue;
        bool blank = true;
        for (int k = 0; k < 3; ++k) blank = blank && w.label[ss_at(w, 0, i + k, f)] == SS_BLANK;
        if (blank) c = SS_G;
    }
    w.label[ss_at(w, 1, r, f)] = c;
}

// thread -> (frame, residue), RESIDUES fastest: the rows of the [F, R] result go out whole
MK_KERNEL(SSL_THREADS) void k_dssp_finish(DsspWs w, int simplified, long long f0, unsigned char* __restrict__ out)
{
    const long long t = (long long)blockIdx.x * SSL_THREADS + threadIdx.x;
    if (t >= w.R * w.Fc) return;
    const long long r = t % w.R, f = t / w.R, R = w.R;
    unsigned c = w.label[ss_at(w, 1, r, f)];
    for (long long i = r - 4 < 1 ? 1 : r - 4; i <= r && i <= R - 6; ++i) {      // I may overwrite H
        if (!((w.flags[ss_at(w, 0, i - 1, f)] & SS_TURN5) && (w.flags[ss_at(w, 0, i, f)] & SS_TURN5))) continue;
        bool free_ = true;
        for (int k = 0; k < 5; ++k) {
            const unsigned x = w.label[ss_at(w, 1, i + k, f)];
            free_ = free_ && (x == SS_BLANK || x == SS_H);
        }
        if (free_) c = SS_I;
    }
    if (c == SS_BLANK && r >= 1 && r <= R - 2) {
        bool turn = false;
#pragma unroll
        for (int s = 3; s <= 5; ++s)
            for (int k = 1; k < s; ++k)
                if (r - k >= 0) turn = turn || (w.flags[ss_at(w, 0, r - k, f)] & (1u << (s - 3)));
        c = turn ? SS_T : (w.flags[ss_at(w, 0, r, f)] & SS_BEND) ? SS_S : SS_BLANK;
    }
    if (simplified) c = (c == SS_H || c == SS_G || c == SS_I) ? 2u : (c == SS_E || c == SS_B) ? 1u : 0u;
    out[(size_t)(f0 + f) * (size_t)R + (size_t)r] = (unsigned char)c;
}

}  // namespace mkamd
