// dihedral_kernels.h -- HIP kernels of MetricDihedral (moleculekit projections/metricdihedral.py:_calcDihedralAngles ->
// dihedral.py:dihedralAngle) on MI355X (gfx950): the torsion angle of D atom quadruples in every frame of a trajectory (DESIGN.md
// section 11).
//
// THE TERMS are the reference's float32 arithmetic to the bit: r12 = x0 - x1, r23 = x1 - x2, r34 = x2 - x3 (each component wrapped
// ONCE where a box is given: _wrapBondedDistance), c1 = r23 x r34, c2 = r12 x r23 (numpy's cross: both products rounded, then the
// difference), p1 = (r12 . c1) * sqrt(r23 . r23), p2 = c1 . c2 (numpy's axis-0 sum: (a + b) + c), the root correctly rounded.  No
// multiply-add is fused anywhere in them.  THE ANGLE is -atan2(p1, p2), and what leaves the kernel is one of
//   DIH_TERMS    (p1, p2)                    [F, D, 2]
//   DIH_RADIANS  the angle                   [F, D]      float64 atan2 of the float32 terms, rounded once
//   DIH_DEGREES  the angle in degrees        [F, D]      the same, times 180 / pi in float64, rounded once
//   DIH_SINCOS   (sin, cos) of the angle     [F, 2 D]    (-p1 / h, p2 / h), h = sqrt(p1^2 + p2^2) in float64, rounded once: no
//                                                        trigonometry at all -- the reference's sc_metric layout
// p1 = p2 = 0 (collinear atoms): angle 0, sin 0, cos 1.  A NaN coordinate makes both terms NaN and with them every output of that
// (frame, dihedral), nothing else.
//
// Two lane assignments, as in the rest of the row:
//   k_dihedral_frames   lanes along FRAMES (the coordinates' fast axis: every load coalesced); a wave owns 64 frames x 16 dihedrals,
//                       the atom rows are wave-uniform, and the frame-major result is transposed through LDS into row stores;
//   k_dihedral_atoms    lanes along the DIHEDRALS of one frame (one structure, a handful of frames): gathers in, rows out.
#pragma once
#include "dist_kernels.h"

namespace mkamd {

enum { DIH_TERMS = 0, DIH_RADIANS = 1, DIH_DEGREES = 2, DIH_SINCOS = 3 };
constexpr int dih_width(int mode) { return mode == DIH_TERMS || mode == DIH_SINCOS ? 2 : 1; }       // floats per (frame, dihedral)

MK_DEV float dih_coord(const float* __restrict__ coords, long long F, unsigned atom, int ax, long long f)
{
    return coords[((size_t)atom * 3 + (size_t)ax) * (size_t)F + (size_t)f];
}

// _wrapBondedDistance on one component: strictly below -box / 2 the box is added, strictly above box / 2 it is subtracted, once
// (box / 2 is exact; a NaN component passes neither test and stays)
MK_DEV float dih_wrap(float d, float b)
{
    const float h = mk_fmul_rn(b, 0.5f);
    return d < -h ? mk_fadd_rn(d, b) : d > h ? mk_fsub_rn(d, b) : d;
}

// numpy's cross product of float32 vectors: c = a x b, every product rounded, then the difference
MK_DEV void dih_cross(const float (&a)[3], const float (&b)[3], float (&c)[3])
{
    c[0] = mk_fsub_rn(mk_fmul_rn(a[1], b[2]), mk_fmul_rn(a[2], b[1]));
    c[1] = mk_fsub_rn(mk_fmul_rn(a[2], b[0]), mk_fmul_rn(a[0], b[2]));
    c[2] = mk_fsub_rn(mk_fmul_rn(a[0], b[1]), mk_fmul_rn(a[1], b[0]));
}

// numpy's (a * b).sum(axis=0) over three rows: (a0 b0 + a1 b1) + a2 b2 -- accumulated from +0, which shows only where all three
// products are -0: the sum is +0 then (degenerate quads: an atom named twice).  Adding +0 last gives the same bits everywhere.
MK_DEV float dih_dot(const float (&a)[3], const float (&b)[3])
{
    return mk_fadd_rn(mk_fadd_rn(mk_fadd_rn(mk_fmul_rn(a[0], b[0]), mk_fmul_rn(a[1], b[1])), mk_fmul_rn(a[2], b[2])), 0.0f);
}

// X[k][ax]: the four atoms; bx: the frame's box (WRAP: the call's box is not all zeros)
template <bool WRAP>
MK_DEV void dih_terms(const float (&X)[4][3], const float (&bx)[3], float& p1, float& p2)
{
    float r12[3], r23[3], r34[3], c1[3], c2[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        r12[ax] = mk_fsub_rn(X[0][ax], X[1][ax]);
        r23[ax] = mk_fsub_rn(X[1][ax], X[2][ax]);
        r34[ax] = mk_fsub_rn(X[2][ax], X[3][ax]);
        if (WRAP) {
            r12[ax] = dih_wrap(r12[ax], bx[ax]);
            r23[ax] = dih_wrap(r23[ax], bx[ax]);
            r34[ax] = dih_wrap(r34[ax], bx[ax]);
        }
    }
    dih_cross(r23, r34, c1);
    dih_cross(r12, r23, c2);
    p1 = mk_fmul_rn(dih_dot(r12, c1), mk_fsqrt_rn(dih_dot(r23, r23)));
    p2 = dih_dot(c1, c2);
}

// 1 / sqrt(x) of a positive double to ~2^-45: the hardware's estimate (v_rsq_f64) and one Newton step -- 6 double-precision
// instructions where sqrt and a division take ~60.  (The host emulation of the tests has no such instruction: the plain expression.)
MK_DEV double dih_rsqrt(double x)
{
#ifdef MK_DEVICE_API_PROVIDED
    return 1.0 / sqrt(x);
#else
    const double y = __builtin_amdgcn_rsq(x);
    const double e = __builtin_fma(-x * y, y, 1.0);
    return __builtin_fma(0.5 * y, e, y);
#endif
}

// the terms -> what the mode stores (o0; o1 too where the mode is two floats wide)
template <int MODE>
MK_DEV void dih_finish(float p1, float p2, float& o0, float& o1)
{
    if constexpr (MODE == DIH_TERMS) { o0 = p1; o1 = p2; return; }
    const bool flat = p1 == 0.0f && p2 == 0.0f;                     // collinear atoms (a NaN is not equal to anything)
    if constexpr (MODE == DIH_SINCOS) {
        // sin(-atan2(p1, p2)) = -p1 / h, cos = p2 / h.  float32 terms are exact in float64 and their squares cannot overflow there
        const double a = (double)p1, b = (double)p2;
        const double inv = dih_rsqrt(a * a + b * b);
        o0 = flat ? 0.0f : (float)(-a * inv);
        o1 = flat ? 1.0f : (float)(b * inv);
        return;
    }
    const double ang = -atan2((double)p1, (double)p2);
    o0 = flat ? 0.0f : MODE == DIH_DEGREES ? (float)(ang * 57.295779513082320876798154814105) : (float)ang;
    o1 = 0.0f;
}

// ------------------------------------------------------------------------------------------------
// Lanes along frames.  A wave: 64 frames x DHF_D consecutive dihedrals.  Its 64 atom indices are ONE coalesced load (lane k holds
// index k of the 16 quads) handed out with readlane: the rows they name are wave-uniform bases and the 12 coordinate loads of a
// dihedral are 256 contiguous bytes each.  Consecutive backbone quads share three atoms; the rows are simply asked for again -- the
// wave touched them a few hundred cycles ago and the CU's cache answers (nothing is kept in registers: quads are arbitrary lists).
// The results go into the wave's LDS tile [64 frames][DHF_D * W floats] (row pitch odd: lanes of a column hit different banks) and
// leave it by rows: a store instruction writes 64 / (DHF_D * W) frames' pieces of DHF_D * W contiguous floats (128 / 64 bytes).
// ------------------------------------------------------------------------------------------------
constexpr int DHF_THREADS = 256, DHF_D = 16;

template <bool WRAP, int MODE>
MK_KERNEL(DHF_THREADS) void k_dihedral_frames(const float* __restrict__ coords, long long F, const float* __restrict__ box,
                                              const unsigned* __restrict__ quads, long long D, float* __restrict__ out)
{
    constexpr int W = dih_width(MODE), ROW = DHF_D * W, PITCH = ROW + 1;
    __shared__ float tiles[DHF_THREADS / WAVE][WAVE * PITCH];
    const long long groups = (D + DHF_D - 1) / DHF_D, tasks = ((F + WAVE - 1) / WAVE) * groups;
    const int wv = (int)mk_uniform(threadIdx.x >> 6);
    const long long task = (long long)blockIdx.x * (DHF_THREADS / WAVE) + (long long)wv;
    if (task >= tasks) return;                                       // (the whole wave; the waves of a block share nothing)
    const int lane = threadIdx.x & (WAVE - 1);
    // waves of a block: neighbouring groups of dihedrals over the SAME frames -- their rows of the result are neighbours
    const long long g = task % groups, slab = task / groups;
    const long long f0 = slab * WAVE;
    const long long f = f0 + lane < F ? f0 + lane : F - 1;          // frames past the end compute on the last one (never stored)
    const long long d0 = g * DHF_D;
    const int nd = D - d0 < DHF_D ? (int)(D - d0) : DHF_D;          // wave-uniform, >= 1
    const unsigned vq = quads[d0 * 4 + (lane < nd * 4 ? lane : nd * 4 - 1)];
    float bx[3] = {0.f, 0.f, 0.f};
    if (WRAP) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) bx[ax] = box[(size_t)ax * (size_t)F + (size_t)f];
    }
    float* __restrict__ tile = tiles[wv];
#pragma unroll 1
    for (int k = 0; k < nd; ++k) {
        float X[4][3];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const unsigned atom = mk_readlane(vq, 4 * k + a);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) X[a][ax] = dih_coord(coords, F, atom, ax, f);
        }
        float p1, p2, o0, o1;
        dih_terms<WRAP>(X, bx, p1, p2);
        dih_finish<MODE>(p1, p2, o0, o1);
        tile[lane * PITCH + k * W] = o0;
        if (W == 2) tile[lane * PITCH + k * W + 1] = o1;
    }
    mk_wave_sync();
    // rows out: lane -> (frame r0 + lane / ROW, column lane % ROW); columns past the call's last dihedral are not stored
    constexpr int RPI = WAVE / ROW;                                  // frames per store instruction (2 or 4)
    const int col = lane % ROW, sub = lane / ROW;
    const size_t pitch_out = (size_t)D * W;
#pragma unroll 4
    for (int r0 = 0; r0 < WAVE; r0 += RPI) {
        const int r = r0 + sub;
        if (f0 + r < F && col < nd * W) out[(size_t)(f0 + r) * pitch_out + (size_t)d0 * W + (size_t)col] = tile[r * PITCH + col];
    }
}

// ------------------------------------------------------------------------------------------------
// Lanes along the dihedrals of ONE frame.  A wave: frame f, 64 consecutive dihedrals; a lane gathers its own 12 coordinates (the
// frames of an atom are F floats apart: nothing coalesces, and nothing can with fewer frames than lanes) and stores its result --
// the lanes' results are neighbours in the frame's row.
// ------------------------------------------------------------------------------------------------
constexpr int DHA_THREADS = 256;

template <bool WRAP, int MODE>
MK_KERNEL(DHA_THREADS) void k_dihedral_atoms(const float* __restrict__ coords, long long F, const float* __restrict__ box,
                                             const unsigned* __restrict__ quads, long long D, float* __restrict__ out)
{
    constexpr int W = dih_width(MODE);
    const long long groups = (D + WAVE - 1) / WAVE, tasks = F * groups;
    const long long task = (long long)blockIdx.x * (DHA_THREADS / WAVE) + (long long)mk_uniform(threadIdx.x >> 6);
    if (task >= tasks) return;                                       // (the whole wave)
    const int lane = threadIdx.x & (WAVE - 1);
    const long long g = task % groups, f = task / groups;
    const long long d = g * WAVE + lane;
    const long long dq = d < D ? d : D - 1;                          // past the end: the last dihedral (computed, never stored)
    float X[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const unsigned atom = quads[dq * 4 + a];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) X[a][ax] = dih_coord(coords, F, atom, ax, f);
    }
    float bx[3] = {0.f, 0.f, 0.f};
    if (WRAP) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) bx[ax] = box[(size_t)ax * (size_t)F + (size_t)f];
    }
    float p1, p2, o0, o1;
    dih_terms<WRAP>(X, bx, p1, p2);
    dih_finish<MODE>(p1, p2, o0, o1);
    if (d < D) {
        float* __restrict__ o = out + ((size_t)f * (size_t)D + (size_t)d) * W;
        o[0] = o0;
        if (W == 2) o[1] = o1;
    }
}

}  // namespace mkamd
