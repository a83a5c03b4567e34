// align_kernels.h -- rigid superposition of trajectory frames on a reference structure (moleculekit's Molecule.align /
// align.py _pp_align, and the RMSD of MetricRmsd), include/mkamd_distance.h "alignment".
//
// Layout: frame-major float32 [F, N, 3] (what the XTC decoder and the voxelizer use); the reference [Fr, Nr, 3].
//
//   k_align_sums<MODE>   per (listed frame, segment of the selection): sums in double over the selected atoms, shifted by the
//                        frame's FIRST selected atom (no cancellation against a far-away origin).  A group of G lanes (8..64,
//                        a power of two: several frames per wave for small selections) walks one segment; the group's lanes are
//                        reduced by butterfly shuffles (32-bit halves) and lane 0 writes the segment's record.  A large selection
//                        of few frames is split into many segments (many waves); the records are summed in segment order by the
//                        next kernel -- no floating-point atomics anywhere: the same bits on every run.
//                        MODE: AL_REF     the reference frame alone (sum b, sum |b|^2: once per call, not per frame)
//                              AL_SINGLE  frame vs one reference frame (sum a, sum a b^T, sum |a|^2)
//                              AL_MATCH   frame f vs reference frame f (everything)
//                              AL_RMSD    sum |float32(M p + t) - q|^2 over a second selection, after the frame's transform
//   k_align_fold         a selection split into many segments: their records summed in a fixed order, a wave per frame
//   k_align_solve<MODE>  one lane per frame, double: centroids, the centred cross-covariance H, Horn's quaternion (largest
//                        eigenvector of the 4x4 key matrix, cyclic Jacobi with a fixed sweep cap: always a proper rotation, no
//                        reflection branch, coplanar selections included) -> affine [12] (include/mkamd_voxel.h (3b)) + fit RMSD
//   k_align_apply        float32(M x + t) for every atom of the listed frames (MK_AFFINE_APPLY: the voxelizer's expression), a
//                        block per 1 024 atoms of a frame, staged through LDS so that global memory moves in aligned 16-byte
//                        pieces whatever the frame's start; in place allowed
//   k_align_rmsd_finish  sqrt(sum / n) per frame, segments summed in order, rounded once to float32
#pragma once
#ifndef MK_DEVICE_API_PROVIDED
#include "mk_device.h"
#endif
#include "mk_affine.h"

namespace mkamd {

enum AlignMode { AL_REF = 0, AL_SINGLE = 1, AL_MATCH = 2, AL_RMSD = 3 };
constexpr int AL_BLOCK = 256;
constexpr int AL_NS = 24;                   // doubles per (frame, segment) record: see AL_* slots
constexpr int AL_SA = 0, AL_SB = 3, AL_SAB = 6, AL_SAA = 15, AL_SBB = 16, AL_SHP = 17, AL_SHQ = 20;
constexpr int AL_JACOBI_SWEEPS = 16;        // a 4x4 symmetric matrix converges in 4-6 cyclic sweeps
constexpr int AL_APPLY_ATOMS = 1024;        // atoms of one frame per k_align_apply block

MK_DEV double al_shfl(double v, int src)
{
    unsigned long long u;
    __builtin_memcpy(&u, &v, 8);
    const unsigned lo = mk_shfl((unsigned)u, src), hi = mk_shfl((unsigned)(u >> 32), src);
    u = ((unsigned long long)hi << 32) | lo;
    double r;
    __builtin_memcpy(&r, &u, 8);
    return r;
}

// sum over the G-lane group (every lane of the wave takes part; the result is valid in every lane of the group)
template <int NV>
MK_DEV void al_group_sum(double (&v)[NV], int glog2)
{
    const int lane = (int)(threadIdx.x & 63);
    for (int off = (1 << glog2) >> 1; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] += al_shfl(v[k], lane ^ off);
    }
}

// Grid: x = groups of items (AL_BLOCK >> glog2 items per block), y = segments of seg_len selected atoms.
// Item i: frame frames[i] (frames == nullptr: frame i) of xyz; its reference frame is refframe, or the same frame (AL_MATCH).
// AL_REF: the single item is the reference frame itself (P = ref over refsel).  AL_RMSD: affine[12 i] moves P first.
// out: records [n_items][segs][AL_NS] (AL_RMSD: [n_items][segs]).
template <int MODE>
MK_KERNEL(AL_BLOCK) void k_align_sums(const float* __restrict__ xyz, long long frame_floats, const float* __restrict__ ref,
                                      long long ref_frame_floats, const unsigned* __restrict__ sel, const unsigned* __restrict__ refsel,
                                      int n, const long long* __restrict__ frames, int n_items, long long refframe, int glog2,
                                      int seg_len, const double* __restrict__ affine, double* __restrict__ out)
{
    const int G = 1 << glog2;
    const int l = (int)threadIdx.x & (G - 1);
    const long long item = (long long)blockIdx.x * (AL_BLOCK >> glog2) + ((int)threadIdx.x >> glog2);
    const int seg = (int)blockIdx.y, segs = (int)gridDim.y;
    const bool valid = item < n_items;
    const float* P = nullptr;
    const float* Q = nullptr;
    if (valid) {
        if constexpr (MODE == AL_REF) {
            P = ref + refframe * ref_frame_floats;
        } else {
            const long long f = frames ? frames[item] : item;
            P = xyz + f * frame_floats;
            Q = ref + ((MODE == AL_MATCH || refframe < 0) ? f : refframe) * ref_frame_floats;   // (AL_RMSD: refframe < 0 = matching)
        }
    }
    const unsigned* psel = MODE == AL_REF ? refsel : sel;
    constexpr int NV = MODE == AL_REF ? 4 : MODE == AL_SINGLE ? 13 : MODE == AL_MATCH ? 17 : 1;
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    double sp[3] = {0.0, 0.0, 0.0}, sq[3] = {0.0, 0.0, 0.0};
    double A[12];
    if (valid && n > 0) {
        if constexpr (MODE != AL_RMSD) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sp[c] = (double)P[3 * (size_t)psel[0] + c];
            if constexpr (MODE != AL_REF) {
#pragma unroll
                for (int c = 0; c < 3; ++c) sq[c] = (double)Q[3 * (size_t)refsel[0] + c];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) A[k] = affine[12 * item + k];
        }
        const long long k0 = (long long)seg * seg_len;
        const long long k1 = k0 + seg_len < n ? k0 + seg_len : n;
        for (long long k = k0 + l; k < k1; k += G) {
            const size_t pi = 3 * (size_t)psel[k];
            if constexpr (MODE == AL_RMSD) {
                float x[3] = {P[pi], P[pi + 1], P[pi + 2]};
                MK_AFFINE_APPLY(A, x);
                const size_t qi = 3 * (size_t)refsel[k];
                const double d0 = (double)x[0] - (double)Q[qi], d1 = (double)x[1] - (double)Q[qi + 1], d2 = (double)x[2] - (double)Q[qi + 2];
                acc[0] += d0 * d0 + d1 * d1 + d2 * d2;
            } else {
                const double a[3] = {(double)P[pi] - sp[0], (double)P[pi + 1] - sp[1], (double)P[pi + 2] - sp[2]};
                if constexpr (MODE == AL_REF) {
                    acc[0] += a[0]; acc[1] += a[1]; acc[2] += a[2];
                    acc[3] += a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
                } else {
                    const size_t qi = 3 * (size_t)refsel[k];
                    const double b[3] = {(double)Q[qi] - sq[0], (double)Q[qi + 1] - sq[1], (double)Q[qi + 2] - sq[2]};
                    acc[0] += a[0]; acc[1] += a[1]; acc[2] += a[2];
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[3 + 3 * r + c] += a[r] * b[c];
                    }
                    acc[12] += a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
                    if constexpr (MODE == AL_MATCH) {
                        acc[13] += b[0]; acc[14] += b[1]; acc[15] += b[2];
                        acc[16] += b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
                    }
                }
            }
        }
    }
    al_group_sum(acc, glog2);
    if (!valid || l != 0) return;
    if constexpr (MODE == AL_RMSD) {
        out[item * segs + seg] = acc[0];
    } else {
        double* o = out + (item * segs + seg) * AL_NS;
        for (int k = 0; k < AL_NS; ++k) o[k] = 0.0;
        for (int c = 0; c < 3; ++c) {
            o[AL_SA + c] = acc[c];
            o[AL_SHP + c] = sp[c];
            o[AL_SHQ + c] = sq[c];
        }
        if constexpr (MODE == AL_REF) {
            o[AL_SAA] = acc[3];
        } else {
            for (int k = 0; k < 9; ++k) o[AL_SAB + k] = acc[3 + k];
            o[AL_SAA] = acc[12];
            if constexpr (MODE == AL_MATCH) {
                for (int c = 0; c < 3; ++c) o[AL_SB + c] = acc[13 + c];
                o[AL_SBB] = acc[16];
            }
        }
    }
}

// The fixed-order second stage of a selection split into segments: one wave per item, lane l sums the records of segments
// l, l + 64, ... in order, the lanes are folded by butterfly shuffles, lane 0 writes the item's record (NV sums, then for the
// statistics records the shifts of segment 0).  part: [n_items][segs][STRIDE] -> out: [n_items][STRIDE].
template <int NV, int STRIDE>
MK_KERNEL(64) void k_align_fold(const double* __restrict__ part, int segs, double* __restrict__ out)
{
    const long long i = blockIdx.x;
    const int lane = (int)threadIdx.x;
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    for (int s = lane; s < segs; s += WAVE) {
        const double* r = part + (i * segs + s) * STRIDE;
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] += r[k];
    }
    al_group_sum(acc, 6);
    if (lane != 0) return;
    double* o = out + i * STRIDE;
    for (int k = 0; k < NV; ++k) o[k] = acc[k];
    for (int k = NV; k < STRIDE; ++k) o[k] = part[i * segs * STRIDE + k];
}

// one Jacobi rotation of the symmetric 4x4 `a` zeroing a[p][q]; v accumulates the eigenvectors (columns)
template <int p, int q>
MK_DEV void al_jacobi_rot(double (&a)[4][4], double (&v)[4][4])
{
    const double apq = a[p][q];
    if (apq == 0.0) return;
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    double t = 1.0 / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double akp = a[k][p], akq = a[k][q];
        a[k][p] = c * akp - s * akq;
        a[k][q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double apk = a[p][k], aqk = a[q][k];
        a[p][k] = c * apk - s * aqk;
        a[q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = v[k][p], vkq = v[k][q];
        v[k][p] = c * vkp - s * vkq;
        v[k][q] = s * vkp + c * vkq;
    }
}

// One lane per listed frame.  part: records [n_items][segs][AL_NS]; refpart (AL_SINGLE): the reference's records [ref_segs][AL_NS].
// affine [n_items][12]: row-major R, then t = c_Q - R c_P;  fit_rmsd [n_items] (nullable): sqrt(max(0, E_P + E_Q - 2 lambda_max) / n).
template <int MODE>
MK_KERNEL(64) void k_align_solve(const double* __restrict__ part, int segs, const double* __restrict__ refpart, int ref_segs, int n,
                                 int n_items, double* __restrict__ affine, double* __restrict__ fit_rmsd)
{
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n_items) return;
    double S[AL_NS];
    for (int k = 0; k < AL_NS; ++k) S[k] = 0.0;
    for (int s = 0; s < segs; ++s) {
        const double* r = part + (i * segs + s) * AL_NS;
        for (int k = 0; k < AL_SHP; ++k) S[k] += r[k];
    }
    for (int k = AL_SHP; k < AL_NS; ++k) S[k] = part[i * segs * AL_NS + k];
    if constexpr (MODE == AL_SINGLE) {
        S[AL_SB] = S[AL_SB + 1] = S[AL_SB + 2] = S[AL_SBB] = 0.0;
        for (int s = 0; s < ref_segs; ++s) {
            const double* r = refpart + (long long)s * AL_NS;
            for (int c = 0; c < 3; ++c) S[AL_SB + c] += r[AL_SA + c];
            S[AL_SBB] += r[AL_SAA];
        }
        for (int c = 0; c < 3; ++c) S[AL_SHQ + c] = refpart[AL_SHP + c];
    }
    double* A = affine + 12 * i;
    if (n == 0) {                            // the reference's means of nothing: NaN coordinates, not an error
        const double nan = __builtin_nan("");
        for (int k = 0; k < 9; ++k) A[k] = (k % 4 == 0) ? 1.0 : 0.0;
        A[9] = A[10] = A[11] = nan;
        if (fit_rmsd) fit_rmsd[i] = nan;
        return;
    }
    const double nd = (double)n;
    const double* Sa = S + AL_SA;
    const double* Sb = S + AL_SB;
    double H[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) H[r][c] = S[AL_SAB + 3 * r + c] - Sa[r] * Sb[c] / nd;
    const double EP = S[AL_SAA] - (Sa[0] * Sa[0] + Sa[1] * Sa[1] + Sa[2] * Sa[2]) / nd;
    const double EQ = S[AL_SBB] - (Sb[0] * Sb[0] + Sb[1] * Sb[1] + Sb[2] * Sb[2]) / nd;
    // Horn's key matrix: its largest eigenvalue's eigenvector is the unit quaternion of the rotation taking P onto Q
    const double Sxx = H[0][0], Sxy = H[0][1], Sxz = H[0][2], Syx = H[1][0], Syy = H[1][1], Syz = H[1][2];
    const double Szx = H[2][0], Szy = H[2][1], Szz = H[2][2];
    double a[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double v[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < AL_JACOBI_SWEEPS; ++sweep) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3] + a[1][2] * a[1][2] + a[1][3] * a[1][3] + a[2][3] * a[2][3];
        const double dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2] + a[3][3] * a[3][3];
        if (!(off > 1e-40 * dia)) break;     // converged (also: a zero matrix, a NaN)
        al_jacobi_rot<0, 1>(a, v);
        al_jacobi_rot<0, 2>(a, v);
        al_jacobi_rot<0, 3>(a, v);
        al_jacobi_rot<1, 2>(a, v);
        al_jacobi_rot<1, 3>(a, v);
        al_jacobi_rot<2, 3>(a, v);
    }
    // the largest eigenvalue (ties: the lowest index -- a zero covariance keeps the identity)
    int m = 0;
    double lam = a[0][0];
    for (int k = 1; k < 4; ++k)
        if (a[k][k] > lam) { lam = a[k][k]; m = k; }
    double w = v[0][m], x = v[1][m], y = v[2][m], z = v[3][m];
    const double qn = 1.0 / __builtin_sqrt(w * w + x * x + y * y + z * z);
    w *= qn; x *= qn; y *= qn; z *= qn;
    const double R[9] = {w * w + x * x - y * y - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                         2.0 * (x * y + w * z), w * w - x * x + y * y - z * z, 2.0 * (y * z - w * x),
                         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), w * w - x * x - y * y + z * z};
    double cP[3], cQ[3];
    for (int c = 0; c < 3; ++c) {
        cP[c] = S[AL_SHP + c] + Sa[c] / nd;
        cQ[c] = S[AL_SHQ + c] + Sb[c] / nd;
    }
    for (int k = 0; k < 9; ++k) A[k] = R[k];
    for (int r = 0; r < 3; ++r) A[9 + r] = cQ[r] - (R[3 * r] * cP[0] + R[3 * r + 1] * cP[1] + R[3 * r + 2] * cP[2]);
    if (fit_rmsd) {
        const double e = EP + EQ - 2.0 * lam;
        fit_rmsd[i] = __builtin_sqrt((e > 0.0 ? e : 0.0) / nd);
    }
}

// Grid: n_items * segs blocks (segs = ceil(N / AL_APPLY_ATOMS)); block b: item b / segs, atoms [AL_APPLY_ATOMS (b % segs), ...).
// out may be xyz (in place): every float is read and written by one block only.  xyz / out only need 4-byte alignment: the
// 16-byte pieces are those of the actual addresses, the partial pieces at a frame's ends go float by float.
MK_KERNEL(AL_BLOCK) void k_align_apply(const float* xyz, long long frame_floats, const long long* __restrict__ frames, int segs,
                                       const double* __restrict__ affine, float* out)
{
    __shared__ __attribute__((aligned(16))) float s_x[3 * AL_APPLY_ATOMS + 8];
    const long long b = blockIdx.x;
    const long long item = b / segs;
    const long long a0 = (b - item * segs) * (long long)AL_APPLY_ATOMS;
    const long long natoms = frame_floats / 3;
    const int na = (int)(natoms - a0 < AL_APPLY_ATOMS ? natoms - a0 : AL_APPLY_ATOMS);
    const long long f = frames ? frames[item] : item;
    const long long g0 = f * frame_floats + 3 * a0, g1 = g0 + 3 * (long long)na;   // this block's floats [g0, g1)
    const int in_mis = (int)(((unsigned long long)(size_t)xyz >> 2) & 3), out_mis = (int)(((unsigned long long)(size_t)out >> 2) & 3);
    const long long in_s0 = ((g0 + in_mis) & ~3LL) - in_mis;                         // first 16-byte piece (float index)
    const long long out_s0 = ((g0 + out_mis) & ~3LL) - out_mis;
    const int in_pieces = (int)((g1 - in_s0 + 3) >> 2), out_pieces = (int)((g1 - out_s0 + 3) >> 2);
    // s_x[4 + g - in_s0] holds float g
    for (int k = (int)threadIdx.x; k < in_pieces; k += AL_BLOCK) {
        const long long g = in_s0 + 4LL * k;
        if (g >= g0 && g + 4 <= g1) {
            const float4 v = *reinterpret_cast<const float4*>(xyz + g);
            *reinterpret_cast<float4*>(s_x + 4 + 4 * k) = v;
        } else {
            for (int j = 0; j < 4; ++j)
                if (g + j >= g0 && g + j < g1) s_x[4 + 4 * k + j] = xyz[g + j];
        }
    }
    mk_block_sync();
    const double* A = affine + 12 * item;
    const int head = 4 + (int)(g0 - in_s0);
    for (int a = (int)threadIdx.x; a < na; a += AL_BLOCK) {
        float p[3] = {s_x[head + 3 * a], s_x[head + 3 * a + 1], s_x[head + 3 * a + 2]};
        MK_AFFINE_APPLY(A, p);
        s_x[head + 3 * a] = p[0];
        s_x[head + 3 * a + 1] = p[1];
        s_x[head + 3 * a + 2] = p[2];
    }
    mk_block_sync();
    const int shift = (int)(out_s0 - in_s0);                                          // 0 unless in and out differ in phase
    for (int k = (int)threadIdx.x; k < out_pieces; k += AL_BLOCK) {
        const long long g = out_s0 + 4LL * k;
        const int li = 4 + 4 * k + shift;
        if (g >= g0 && g + 4 <= g1) {
            float4 v;
            if (shift == 0) {
                v = *reinterpret_cast<const float4*>(s_x + li);
            } else {
                v.x = s_x[li]; v.y = s_x[li + 1]; v.z = s_x[li + 2]; v.w = s_x[li + 3];
            }
            *reinterpret_cast<float4*>(out + g) = v;
        } else {
            for (int j = 0; j < 4; ++j)
                if (g + j >= g0 && g + j < g1) out[g + j] = s_x[li + j];
        }
    }
}

// rmsd [n_items] = float32(sqrt(sum over segments, in order / n))
MK_KERNEL(64) void k_align_rmsd_finish(const double* __restrict__ part, int segs, int n, int n_items, float* __restrict__ rmsd)
{
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n_items) return;
    double s = 0.0;
    for (int k = 0; k < segs; ++k) s += part[i * segs + k];
    rmsd[i] = (float)__builtin_sqrt(s / (double)n);
}

}  // namespace mkamd
