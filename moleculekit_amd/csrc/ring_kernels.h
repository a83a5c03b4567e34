// ring_kernels.h -- HIP kernels of the ring interactions (moleculekit interactions/pipi/pipi.pyx, cationpi/cationpi.pyx,
// sigmahole/sigmahole.pyx: `calculate`) on MI355X (gfx950): pi-pi stacking between two lists of rings, cation-pi and sigma-hole
// contacts between a list of rings and a list of atoms, in every frame of a trajectory.
//
// THE TERMS are the reference's float32 arithmetic to the bit, up to the float32 squared distance and the float32 dot product:
//   centroid    a serial sum from 0 over the ring's atoms in list order, per axis, divided by float32(count)
//   normal      t1 = a0 - a2, t2 = a1 - a2 of the ring's first three atoms; t1 x t2 with both products rounded, then the difference; the
//               norm a sum from 0 of the squares, the root correctly rounded, every component divided by it (a degenerate ring: inf / NaN,
//               which flow on as they do in the reference)
//   wrapped d2  per axis val = p1 - p2; ONLY where |val| > box / 2 and box != 0: val = val - box * round(val / box), round() half away
//               from zero; d2 a sum from 0 of val * val
//   angle       acos(dot) * 57.29578, folded at 90 (a NaN -- |dot| just above 1 -- fails every comparison: the pair is dropped, as the
//               reference drops it)
// The three modules are C++ (they use libcpp.vector), and in C++ `round`, `sqrt` and `acos` of a float32 argument are the FLOAT32
// overloads: the wrap is float32 throughout (quotient, roundf, product, difference: four roundings), and the angle is the C library's
// float32 acosf, widened, times the float64 constant -- folded and compared in float64.  acosf is not correctly rounded in the C
// library the reference is built against (glibc before its correctly rounded rewrite: fdlibm's e_acosf.c, two rational approximations
// and a split square root in float32 operations), and after the fold at 90 one unit of acosf's last place is up to sixteen of the
// angle's: ring_acosf restates that algorithm operation by operation, so the angles are the reference's bits too.
// No float32 multiply-add is fused anywhere (mk_f*_rn).  The float32 divisions and roots are taken in float64 and rounded once more:
// for operands that are float32 numbers that IS the correctly rounded float32 result (53 >= 2 * 24 + 2 bits), and it keeps the float32
// pipeline free of the fused multiply-adds a float32 division or root expands to.
//
// Per chunk of frames: a pre-pass writes one record per (frame, ring) -- centroid, normal, first atom: the reference recomputes them for
// every partner -- and per (frame, partner); a count kernel decides every pair and leaves a 64-bit mask per (tile of 64 pairs, frame);
// k_contacts_scan (dist_kernels.h) turns the masks' populations into per-frame prefixes; a fill kernel walks the set bits -- ascending
// pair index q = r1 * n2 + r2 is the reference's loop order -- and writes (r1, second) and (distance, angle).
// Two lane assignments: lanes along FRAMES (records are frame-fastest: every load coalesced, the first ring's record stays in
// registers while r2 runs) or along the PAIRS of one frame (pose scoring: one frame, a few hundred pairs).
#pragma once
#include "dist_kernels.h"

namespace mkamd {

enum { RING_PIPI = 0, RING_CATIONPI = 1, RING_SIGMAHOLE = 2 };
constexpr int RING_REC = 9;                                          // floats of a ring's record: centroid, normal, first atom
constexpr int ring_part_width(int kind) { return kind == RING_SIGMAHOLE ? 6 : 3; }   // a partner's: position (, unit bond vector)
constexpr int RING_TILE = 64;                                        // pairs per mask

// what a pair is held against: pi-pi (d1^2, d2^2, a1max, a2min); cation-pi / sigma-hole (-, thr^2, -, angle min)
struct RingThr { float d1sq, d2sq, a1, a2; };

// the compiler must not see through the float64 detour of a division / a root (it would narrow them back to float32 operations)
MK_DEV double ring_opaque(double x)
{
#ifndef MK_DEVICE_API_PROVIDED
    asm("" : "+v"(x));
#endif
    return x;
}
MK_DEV float ring_div(float a, float b) { return (float)ring_opaque(ring_opaque((double)a) / ring_opaque((double)b)); }
MK_DEV float ring_sqrt(float x) { return (float)ring_opaque(sqrt(ring_opaque((double)x))); }

MK_DEV float ring_coord(const float* __restrict__ coords, long long F, unsigned atom, int ax, long long f)
{
    return coords[((size_t)atom * 3 + (size_t)ax) * (size_t)F + (size_t)f];
}

// box == nullptr: every axis open
MK_DEV void ring_box(const float* __restrict__ box, long long F, long long f, float (&bx)[3])
{
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) bx[ax] = box ? box[(size_t)ax * (size_t)F + (size_t)f] : 0.0f;
}

// _wrapped_dist
MK_DEV float ring_wdist2(const float (&p1)[3], const float (&p2)[3], const float (&bx)[3])
{
    float d2 = 0.0f;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        float val = mk_fsub_rn(p1[ax], p2[ax]);
        const float half = mk_fmul_rn(bx[ax], 0.5f);                 // box / 2 (exact)
        if (mk_abs(val) > half && bx[ax] != 0.0f) val = mk_fsub_rn(val, mk_fmul_rn(bx[ax], roundf(ring_div(val, bx[ax]))));
        d2 = mk_fadd_rn(d2, mk_fmul_rn(val, val));
    }
    return d2;
}

// _normalize
MK_DEV void ring_normalize(float (&v)[3])
{
    float n2 = 0.0f;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) n2 = mk_fadd_rn(n2, mk_fmul_rn(v[ax], v[ax]));
    const float n = ring_sqrt(n2);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) v[ax] = ring_div(v[ax], n);
}

MK_DEV float ring_dot(const float (&a)[3], const float (&b)[3])
{
    float d = 0.0f;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) d = mk_fadd_rn(d, mk_fmul_rn(a[ax], b[ax]));
    return d;
}

// fdlibm's __ieee754_acosf (e_acosf.c: "Developed at SunPro ... Permission to use, copy, modify, and distribute this software is
// freely granted"), the float32 acos of the C library the reference runs on, every operation rounded on its own
MK_DEV float ring_acos_ratio(float z)
{
    const float pS0 = 1.6666667163e-01f, pS1 = -3.2556581497e-01f, pS2 = 2.0121252537e-01f, pS3 = -4.0055535734e-02f, pS4 = 7.9153501429e-04f,
                pS5 = 3.4793309169e-05f, qS1 = -2.4033949375e+00f, qS2 = 2.0209457874e+00f, qS3 = -6.8828397989e-01f, qS4 = 7.7038154006e-02f;
    float p = mk_fadd_rn(pS4, mk_fmul_rn(z, pS5));
    p = mk_fadd_rn(pS3, mk_fmul_rn(z, p));
    p = mk_fadd_rn(pS2, mk_fmul_rn(z, p));
    p = mk_fadd_rn(pS1, mk_fmul_rn(z, p));
    p = mk_fmul_rn(z, mk_fadd_rn(pS0, mk_fmul_rn(z, p)));
    float q = mk_fadd_rn(qS3, mk_fmul_rn(z, qS4));
    q = mk_fadd_rn(qS2, mk_fmul_rn(z, q));
    q = mk_fadd_rn(qS1, mk_fmul_rn(z, q));
    q = mk_fadd_rn(1.0f, mk_fmul_rn(z, q));
    return ring_div(p, q);
}
MK_DEV float ring_acosf(float x)
{
    const float pi = 3.1415925026e+00f, pio2_hi = 1.5707962513e+00f, pio2_lo = 7.5497894159e-08f;
    const int hx = mk_float_as_int(x), ix = hx & 0x7fffffff;
    if (ix == 0x3f800000) return hx > 0 ? 0.0f : mk_fadd_rn(pi, mk_fmul_rn(2.0f, pio2_lo));      // |x| == 1
    if (ix > 0x3f800000) return mk_int_as_float(0x7fc00000);         // |x| > 1 (and NaN): NaN
    if (ix < 0x3f000000) {                                           // |x| < 0.5
        if (ix <= 0x23000000) return mk_fadd_rn(pio2_hi, pio2_lo);
        const float r = ring_acos_ratio(mk_fmul_rn(x, x));
        return mk_fsub_rn(pio2_hi, mk_fsub_rn(x, mk_fsub_rn(pio2_lo, mk_fmul_rn(x, r))));
    }
    if (hx < 0) {                                                    // x < -0.5
        const float z = mk_fmul_rn(mk_fadd_rn(1.0f, x), 0.5f);
        const float r = ring_acos_ratio(z), s = ring_sqrt(z);
        const float w = mk_fsub_rn(mk_fmul_rn(r, s), pio2_lo);
        return mk_fsub_rn(pi, mk_fmul_rn(2.0f, mk_fadd_rn(s, w)));
    }
    const float z = mk_fmul_rn(mk_fsub_rn(1.0f, x), 0.5f);           // x > 0.5
    const float s = ring_sqrt(z);
    const float df = mk_int_as_float(mk_float_as_int(s) & (int)0xfffff000);
    const float c = ring_div(mk_fsub_rn(z, mk_fmul_rn(df, df)), mk_fadd_rn(s, df));
    const float w = mk_fadd_rn(mk_fmul_rn(ring_acos_ratio(z), s), c);
    return mk_fmul_rn(2.0f, mk_fadd_rn(df, w));
}

// acos(dot) in degrees, folded at 90: the float32 acosf widened, the rest float64
MK_DEV double ring_angle(float dot)
{
    double angle = mk_dmul_rn((double)ring_acosf(dot), 57.29578);
    if (angle > 90.0) angle = 180.0 - angle;
    return angle;
}

// ------------------------------------------------------------------------------------------------
// Pre-pass: the record of every (frame of the chunk, ring), rec[(ring * 9 + c) * pitch + lf], rings of the second list behind those
// of the first.  FRAMES: consecutive lanes are consecutive frames (coalesced coordinate loads, the ring's atoms wave-uniform);
// otherwise consecutive rings of one frame.
// ------------------------------------------------------------------------------------------------
constexpr int RP_THREADS = 256;

template <bool FRAMES>
MK_KERNEL(RP_THREADS) void k_ring_prepass(const float* __restrict__ coords, long long F, long long f0, long long fc, long long pitch,
                                          const unsigned* __restrict__ ring_atoms, const unsigned* __restrict__ starts1, long long n1,
                                          const unsigned* __restrict__ starts2, long long n2, float* __restrict__ rec)
{
    // FRAMES: a wave is 64 frames (blockIdx.y) of one ring; otherwise a block is 256 rings of one frame (blockIdx.y)
    const long long R = n1 + n2;
    const long long ring = FRAMES ? (long long)blockIdx.x * (RP_THREADS / WAVE) + (threadIdx.x >> 6) : (long long)blockIdx.x * RP_THREADS + threadIdx.x;
    const long long lf = FRAMES ? (long long)blockIdx.y * WAVE + (threadIdx.x & (WAVE - 1)) : (long long)blockIdx.y;
    if (ring >= R || lf >= fc) return;
    const long long f = f0 + lf;
    const unsigned* __restrict__ st = ring < n1 ? starts1 + ring : starts2 + (ring - n1);
    const unsigned s = st[0], e = st[1];
    float sum[3] = {0.0f, 0.0f, 0.0f};
    for (unsigned k = s; k < e; ++k) {
        const unsigned atom = ring_atoms[k];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) sum[ax] = mk_fadd_rn(sum[ax], ring_coord(coords, F, atom, ax, f));
    }
    const float count = (float)(int)(e - s);
    float a[3][3];                                                   // the first three atoms (the host has checked that there are three)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const unsigned atom = ring_atoms[s + k];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) a[k][ax] = ring_coord(coords, F, atom, ax, f);
    }
    float t1[3], t2[3], nrm[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        t1[ax] = mk_fsub_rn(a[0][ax], a[2][ax]);
        t2[ax] = mk_fsub_rn(a[1][ax], a[2][ax]);
    }
    nrm[0] = mk_fsub_rn(mk_fmul_rn(t1[1], t2[2]), mk_fmul_rn(t1[2], t2[1]));
    nrm[1] = mk_fsub_rn(mk_fmul_rn(t1[2], t2[0]), mk_fmul_rn(t1[0], t2[2]));
    nrm[2] = mk_fsub_rn(mk_fmul_rn(t1[0], t2[1]), mk_fmul_rn(t1[1], t2[0]));
    ring_normalize(nrm);
    float* __restrict__ o = rec + (size_t)ring * RING_REC * (size_t)pitch + (size_t)lf;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        o[(size_t)ax * (size_t)pitch] = ring_div(sum[ax], count);
        o[(size_t)(3 + ax) * (size_t)pitch] = nrm[ax];
        o[(size_t)(6 + ax) * (size_t)pitch] = a[0][ax];
    }
}

// ... and of every (frame, partner): part[(p * PW + c) * pitch + lf] -- the cation's / halogen's position and, sigma-hole, the unit
// vector halogen - bonded atom (unwrapped; the reference normalises it again for every ring)
template <int KIND, bool FRAMES>
MK_KERNEL(RP_THREADS) void k_ring_partners(const float* __restrict__ coords, long long F, long long f0, long long fc, long long pitch,
                                           const unsigned* __restrict__ partners, long long n2, float* __restrict__ part)
{
    constexpr int PW = ring_part_width(KIND), STRIDE = KIND == RING_SIGMAHOLE ? 2 : 1;
    const long long p = FRAMES ? (long long)blockIdx.x * (RP_THREADS / WAVE) + (threadIdx.x >> 6) : (long long)blockIdx.x * RP_THREADS + threadIdx.x;
    const long long lf = FRAMES ? (long long)blockIdx.y * WAVE + (threadIdx.x & (WAVE - 1)) : (long long)blockIdx.y;
    if (p >= n2 || lf >= fc) return;
    const long long f = f0 + lf;
    const unsigned atom = partners[p * STRIDE];
    float pos[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) pos[ax] = ring_coord(coords, F, atom, ax, f);
    float* __restrict__ o = part + (size_t)p * PW * (size_t)pitch + (size_t)lf;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) o[(size_t)ax * (size_t)pitch] = pos[ax];
    if constexpr (KIND == RING_SIGMAHOLE) {
        const unsigned bonded = partners[p * STRIDE + 1];
        float v[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) v[ax] = mk_fsub_rn(pos[ax], ring_coord(coords, F, bonded, ax, f));
        ring_normalize(v);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) o[(size_t)(3 + ax) * (size_t)pitch] = v[ax];
    }
}

// ------------------------------------------------------------------------------------------------
// One pair in one frame.  A: the first ring's record (in registers); B: the records of the second rings (pi-pi) or of the partners,
// read as far as the pair gets.  Returns whether the reference reports the pair; dist2 and angle are what it reports then.
// ------------------------------------------------------------------------------------------------
MK_DEV void ring_load_first(const float* __restrict__ rec, size_t r1, size_t pitch, size_t lf, float (&A)[RING_REC])
{
#pragma unroll
    for (int c = 0; c < RING_REC; ++c) A[c] = rec[(r1 * RING_REC + (size_t)c) * pitch + lf];
}

template <int KIND>
MK_DEV bool ring_pair(const float (&A)[RING_REC], const float* __restrict__ B, size_t b, size_t pitch, size_t lf, const float (&bx)[3],
                      const RingThr& T, float& dist2, double& angle)
{
    constexpr int BW = KIND == RING_PIPI ? RING_REC : ring_part_width(KIND);
    const float* __restrict__ pb = B + b * BW * pitch + lf;
    const float mean[3] = {A[0], A[1], A[2]}, normal[3] = {A[3], A[4], A[5]};
    dist2 = 0.0f;
    angle = 0.0;
    if constexpr (KIND == RING_PIPI) {
        const float fa[3] = {A[6], A[7], A[8]}, fb[3] = {pb[6 * pitch], pb[7 * pitch], pb[8 * pitch]};
        if (ring_wdist2(fa, fb, bx) > 225.0f) return false;         // "two randomly picked atoms are more than 15 A apart"
        const float mb[3] = {pb[0], pb[pitch], pb[2 * pitch]};
        dist2 = ring_wdist2(mean, mb, bx);
        if (dist2 > T.d2sq) return false;
        const float nb[3] = {pb[3 * pitch], pb[4 * pitch], pb[5 * pitch]};
        angle = ring_angle(ring_dot(normal, nb));
        return (dist2 < T.d1sq && angle <= (double)T.a1) || (dist2 < T.d2sq && angle >= (double)T.a2);
    } else {
        const float pos[3] = {pb[0], pb[pitch], pb[2 * pitch]};
        dist2 = ring_wdist2(mean, pos, bx);
        if (dist2 > T.d2sq) return false;
        float v[3];
        if constexpr (KIND == RING_CATIONPI) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) v[ax] = mk_fsub_rn(pos[ax], mean[ax]);     // not wrapped
            ring_normalize(v);
        } else {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) v[ax] = pb[(size_t)(3 + ax) * pitch];
        }
        angle = 90.0 - ring_angle(ring_dot(normal, v));              // to the plane, not to its normal
        return angle >= (double)T.a2;
    }
}

// pi-pi: "skip self-interactions of identical rings" -- the same (start, end) in the concatenated atom list
MK_DEV bool ring_same(const unsigned* __restrict__ starts1, const unsigned* __restrict__ starts2, long long r1, long long r2)
{
    return starts1[r1] == starts2[r2] && starts1[r1 + 1] == starts2[r2 + 1];
}

// ------------------------------------------------------------------------------------------------
// Count, lanes along frames.  A wave: 64 frames x one tile of 64 consecutive pairs; the pair is wave-uniform, the first ring's record
// is loaded when r1 changes.  masks / cnt [tile][pitch]; frames past the chunk compute on its last frame and store nothing.
// ------------------------------------------------------------------------------------------------
constexpr int RC_THREADS = 256;

template <int KIND>
MK_KERNEL(RC_THREADS) void k_ring_count_frames(const float* __restrict__ rec, const float* __restrict__ part, long long pitch, long long fc,
                                               const float* __restrict__ box, long long F, long long f0, const unsigned* __restrict__ starts1,
                                               long long n1, const unsigned* __restrict__ starts2, long long n2, RingThr T,
                                               unsigned long long* __restrict__ masks, unsigned* __restrict__ cnt)
{
    const long long P = n1 * n2, tiles = (P + RING_TILE - 1) / RING_TILE;                     // (the host: P <= 2^30)
    const long long tile = (long long)blockIdx.x * (RC_THREADS / WAVE) + (long long)mk_uniform(threadIdx.x >> 6);
    if (tile >= tiles) return;                                       // (the whole wave)
    const int lane = threadIdx.x & (WAVE - 1);
    const long long lf = (long long)blockIdx.y * WAVE + lane;       // waves of a block: neighbouring tiles over the same frames
    const size_t lfc = (size_t)(lf < fc ? lf : fc - 1);
    float bx[3];
    ring_box(box, F, f0 + (long long)lfc, bx);
    const long long q0 = tile * RING_TILE;
    const int nq = P - q0 < RING_TILE ? (int)(P - q0) : RING_TILE;
    unsigned long long m = 0ull;
    long long cur = -1;
    float A[RING_REC];
#pragma unroll 1
    for (int k = 0; k < nq; ++k) {
        const unsigned q = (unsigned)(q0 + k), r1 = q / (unsigned)n2, r2 = q - r1 * (unsigned)n2;
        if ((long long)r1 != cur) { ring_load_first(rec, (size_t)r1, (size_t)pitch, lfc, A); cur = r1; }
        float d2;
        double ang;
        bool hit = false;
        if (!(KIND == RING_PIPI && ring_same(starts1, starts2, r1, r2)))
            hit = ring_pair<KIND>(A, KIND == RING_PIPI ? rec : part, (size_t)(KIND == RING_PIPI ? n1 + r2 : r2), (size_t)pitch, lfc, bx, T, d2, ang);
        m |= (unsigned long long)hit << k;
    }
    if (lf < fc) {
        masks[(size_t)tile * (size_t)pitch + (size_t)lf] = m;
        cnt[(size_t)tile * (size_t)pitch + (size_t)lf] = (unsigned)mk_popc64(m);
    }
}

// Count, lanes along the pairs of ONE frame.  A wave: frame lf, one tile of 64 consecutive pairs; the mask is a ballot.
template <int KIND>
MK_KERNEL(RC_THREADS) void k_ring_count_pairs(const float* __restrict__ rec, const float* __restrict__ part, long long pitch, long long fc,
                                              const float* __restrict__ box, long long F, long long f0, const unsigned* __restrict__ starts1,
                                              long long n1, const unsigned* __restrict__ starts2, long long n2, RingThr T,
                                              unsigned long long* __restrict__ masks, unsigned* __restrict__ cnt)
{
    const long long P = n1 * n2, tiles = (P + RING_TILE - 1) / RING_TILE;
    const long long tile = (long long)blockIdx.x * (RC_THREADS / WAVE) + (long long)mk_uniform(threadIdx.x >> 6), lf = (long long)blockIdx.y;
    if (tile >= tiles) return;                                       // (the whole wave)
    const int lane = threadIdx.x & (WAVE - 1);
    float bx[3];
    ring_box(box, F, f0 + lf, bx);
    const long long q = tile * RING_TILE + lane;
    const bool valid = q < P;
    const unsigned qq = (unsigned)(valid ? q : P - 1), r1 = qq / (unsigned)n2, r2 = qq - r1 * (unsigned)n2;    // past the end: the last pair (computed, never counted)
    float A[RING_REC];
    ring_load_first(rec, (size_t)r1, (size_t)pitch, (size_t)lf, A);
    float d2;
    double ang;
    bool hit = false;
    if (!(KIND == RING_PIPI && ring_same(starts1, starts2, r1, r2)))
        hit = ring_pair<KIND>(A, KIND == RING_PIPI ? rec : part, (size_t)(KIND == RING_PIPI ? n1 + r2 : r2), (size_t)pitch, (size_t)lf, bx, T, d2, ang);
    const unsigned long long m = mk_ballot(hit && valid);
    if (lane == 0) {
        masks[(size_t)tile * (size_t)pitch + (size_t)lf] = m;
        cnt[(size_t)tile * (size_t)pitch + (size_t)lf] = (unsigned)mk_popc64(m);
    }
}

// ------------------------------------------------------------------------------------------------
// Fill.  A lane owns one (tile, frame): its reported pairs go to frame_base[lf] + prefix[tile][lf] onwards, ascending pair index.  The
// terms are computed again (the same code on the same records: the same bits) -- reported pairs are few.  FRAMES: consecutive lanes are
// consecutive frames, as in the count kernel that wrote the masks; otherwise consecutive tiles.
// `emit`: what names the second partner in the list -- emit[r2 * estride] (the cation's / halogen's atom index), r2 itself where null.
// ------------------------------------------------------------------------------------------------
constexpr int RF_THREADS = 256;

template <int KIND, bool FRAMES>
MK_KERNEL(RF_THREADS) void k_ring_fill(const float* __restrict__ rec, const float* __restrict__ part, long long pitch, long long fc,
                                       const float* __restrict__ box, long long F, long long f0, long long n1, long long n2, RingThr T,
                                       const unsigned long long* __restrict__ masks, const unsigned* __restrict__ prefix,
                                       const unsigned long long* __restrict__ frame_base, const unsigned* __restrict__ emit, int estride,
                                       uint2* __restrict__ pairs, float2* __restrict__ distang)
{
    const long long P = n1 * n2, tiles = (P + RING_TILE - 1) / RING_TILE;
    const long long tile = FRAMES ? (long long)blockIdx.x * (RF_THREADS / WAVE) + (threadIdx.x >> 6) : (long long)blockIdx.x * RF_THREADS + threadIdx.x;
    const long long lf = FRAMES ? (long long)blockIdx.y * WAVE + (threadIdx.x & (WAVE - 1)) : (long long)blockIdx.y;
    if (tile >= tiles || lf >= fc) return;
    unsigned long long m = masks[(size_t)tile * (size_t)pitch + (size_t)lf];
    if (m == 0ull) return;
    unsigned long long pos = frame_base[lf] + prefix[(size_t)tile * (size_t)pitch + (size_t)lf];
    float bx[3];
    ring_box(box, F, f0 + lf, bx);
    while (m) {
        const int k = mk_ctz64(m);
        m &= m - 1ull;
        const unsigned q = (unsigned)(tile * RING_TILE + k), r1 = q / (unsigned)n2, r2 = q - r1 * (unsigned)n2;
        float A[RING_REC], d2;
        double ang;
        ring_load_first(rec, (size_t)r1, (size_t)pitch, (size_t)lf, A);
        (void)ring_pair<KIND>(A, KIND == RING_PIPI ? rec : part, (size_t)(KIND == RING_PIPI ? n1 + r2 : r2), (size_t)pitch, (size_t)lf, bx, T, d2, ang);
        pairs[pos] = make_uint2(r1, emit ? emit[(size_t)r2 * (size_t)estride] : r2);
        distang[pos] = make_float2(ring_sqrt(d2), (float)ang);
        ++pos;
    }
}

}  // namespace mkamd
