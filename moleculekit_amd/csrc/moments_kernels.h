// moments_kernels.h -- HIP kernels of the group-moment projections (moleculekit projections/metriccoordinate.py, metricgyration.py,
// metricfluctuation.py, metricsphericalcoordinate.py) on MI355X (gfx950): weighted first and second moments of small sets of atoms in
// every frame of a trajectory, optionally after each frame's rigid transform.
//
// Layout: coordinates frame-major float32 [F, N, 3] (the XTC decoder's, align.py's and the voxelizer's); the optional affine float64
// [F, 12] of include/mkamd_voxel.h (3b) -- what k_align_solve writes; groups CSR: atoms uint32 [n_sel], offsets uint32 [G + 1],
// weights float32 [n_sel] or NULL (1).  Every gathered atom goes through MK_AFFINE_APPLY first where an affine is given: the value
// summed has the bits k_align_apply would have stored, and the aligned trajectory is never written.  All sums in double.
//
//   k_mom_sums<MODE, SEG>   per (frame, group): a group of L lanes (8..64, a power of two: several small groups per wave) walks the
//                           group's atoms (SEG: one segment of them, blockIdx.y); butterfly shuffles on 32-bit halves fold the lanes
//                           (al_group_sum); lane 0 finishes the (frame, group) and stores it (SEG: stores the segment's record for
//                           k_mom_fold).  No floating-point atomics anywhere: the same bits on every run.
//   k_mom_fold<MODE>        a wave per (frame, group): the segments' records summed in a fixed order, then the same finish
//   k_mom_mean              per selected atom the mean position over all frames, in double, lanes along the frames in a fixed order
//   k_mom_fluct_atoms       a lane per (frame, selected atom): sum_c (x_c - ref_c)^2 in double
//
// MODE (include/mkamd_distance.h MKAMD_MOM_*):
//   MOM_CENTER     sum w, sum w x                     -> float32 [F, 3 G], column c G + g:  sum w x_c / sum w, rounded once
//   MOM_GYRATION   sum w, sum w a, sum w a_c^2 with a = x - s, s the group's FIRST atom in that frame (the shift of k_align_sums: the
//                  second moment about the centre of mass m_c = sum w a_c^2 / W - (sum w a_c / W)^2 loses nothing to a far-away origin)
//                                                     -> float32 [F, G, 4]: sqrt of m_x + m_y + m_z, m_y + m_z, m_x + m_z, m_x + m_y
//   MOM_SPHERICAL  exactly two unweighted groups (target, reference) per frame: d = centroid_0 - centroid_1
//                                                     -> float32 [F, 3]: |d|, acos(d_z / |d|), atan2(d_y, d_x)
//   MOM_FLUCT      sum over the group of sum_c (x_c - ref[k]_c)^2, ref float64 [n_sel, 3]
//                                                     -> float64 [F, G]: the sum / the group's size
#pragma once
#include "align_kernels.h"

namespace mkamd {

enum { MOM_CENTER = 0, MOM_GYRATION = 1, MOM_SPHERICAL = 2, MOM_FLUCT = 3 };
constexpr int MOM_BLOCK = 256;
constexpr int mom_nv(int mode) { return mode == MOM_GYRATION ? 7 : mode == MOM_SPHERICAL ? 6 : mode == MOM_FLUCT ? 1 : 4; }   // sums
constexpr int mom_rec(int mode) { return mom_nv(mode) + (mode == MOM_GYRATION ? 3 : 0); }     // doubles per segment record (+ shift)

// atom `atom` of frame P, moved by the frame's transform where there is one
MK_DEV void mom_load(const float* __restrict__ P, unsigned atom, bool has_aff, const double (&A)[12], float (&x)[3])
{
    const size_t i = 3 * (size_t)atom;
    x[0] = P[i]; x[1] = P[i + 1]; x[2] = P[i + 2];
    if (has_aff) MK_AFFINE_APPLY(A, x);
}

MK_DEV double mom_nonneg(double m) { return m < 0.0 ? 0.0 : m; }      // (rounding of a zero spread; a NaN stays)

// the sums S (and the shift s) of one (frame, group) -> what the mode stores.  n0 / n1: the group's size (MOM_FLUCT), the two
// groups' sizes (MOM_SPHERICAL).
template <int MODE>
MK_DEV void mom_finish(const double (&S)[mom_nv(MODE)], const double (&s)[3], long long f, long long g, long long G, double n0, double n1,
                       void* __restrict__ out_)
{
    if constexpr (MODE == MOM_CENTER) {
        float* o = static_cast<float*>(out_) + (size_t)f * 3 * (size_t)G + (size_t)g;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(size_t)c * (size_t)G] = (float)(S[1 + c] / S[0]);
    } else if constexpr (MODE == MOM_GYRATION) {
        double m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double com = S[1 + c] / S[0];
            m[c] = mom_nonneg(S[4 + c] / S[0] - com * com);
        }
        float* o = static_cast<float*>(out_) + ((size_t)f * (size_t)G + (size_t)g) * 4;
        o[0] = (float)__builtin_sqrt(m[0] + m[1] + m[2]);
        o[1] = (float)__builtin_sqrt(m[1] + m[2]);
        o[2] = (float)__builtin_sqrt(m[0] + m[2]);
        o[3] = (float)__builtin_sqrt(m[0] + m[1]);
    } else if constexpr (MODE == MOM_SPHERICAL) {
        const double dx = S[0] / n0 - S[3] / n1, dy = S[1] / n0 - S[4] / n1, dz = S[2] / n0 - S[5] / n1;
        const double r = __builtin_sqrt(dx * dx + dy * dy + dz * dz);
        float* o = static_cast<float*>(out_) + (size_t)f * 3;
        o[0] = (float)r;
        o[1] = (float)acos(dz / r);                                   // (|d| = 0: 0 / 0, NaN, as numpy)
        o[2] = (float)atan2(dy, dx);
    } else {
        static_cast<double*>(out_)[(size_t)f * (size_t)G + (size_t)g] = S[0] / n0;
    }
}

// Grid: x = groups of items (MOM_BLOCK >> glog2 items per block), y = segments (SEG; else 1).  Item i: frame i / G, group i % G
// (MOM_SPHERICAL: frame i, both groups: the atoms [offsets[0], offsets[2]) walked as one list).  SEG: segment y covers seg_len atoms
// of the item's list, the LAST segment everything that is left; its record goes to part [n_items][segs][mom_rec(MODE)].
template <int MODE, bool SEG>
MK_KERNEL(MOM_BLOCK) void k_mom_sums(const float* __restrict__ xyz, long long frame_floats, const double* __restrict__ affine,
                                     const unsigned* __restrict__ atoms, const unsigned* __restrict__ offsets,
                                     const float* __restrict__ weights, const double* __restrict__ ref, long long G, long long n_items,
                                     int glog2, int seg_len, void* __restrict__ out, double* __restrict__ part)
{
    constexpr int NV = mom_nv(MODE), REC = mom_rec(MODE);
    const int L = 1 << glog2;
    const int l = (int)threadIdx.x & (L - 1);
    const long long item = (long long)blockIdx.x * (MOM_BLOCK >> glog2) + ((int)threadIdx.x >> glog2);
    const int seg = SEG ? (int)blockIdx.y : 0, segs = SEG ? (int)gridDim.y : 1;
    const bool valid = item < n_items;
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    double s[3] = {0.0, 0.0, 0.0};
    long long f = 0, g = 0;
    double n0 = 0.0, n1 = 0.0;
    if (valid) {
        f = MODE == MOM_SPHERICAL ? item : item / G;
        g = MODE == MOM_SPHERICAL ? 0 : item - f * G;
        const float* __restrict__ P = xyz + f * frame_floats;
        const bool has_aff = affine != nullptr;
        double A[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) A[k] = has_aff ? affine[12 * f + k] : 0.0;
        const long long b = offsets[g], mid = offsets[g + 1], e = MODE == MOM_SPHERICAL ? (long long)offsets[2] : mid;
        n0 = (double)(mid - b);
        n1 = (double)(e - mid);
        float x[3];
        if constexpr (MODE == MOM_GYRATION) {
            mom_load(P, atoms[b], has_aff, A, x);
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] = (double)x[c];
        }
        const long long k0 = b + (long long)seg * seg_len;
        const long long k1 = (!SEG || seg == segs - 1 || k0 + seg_len > e) ? e : k0 + seg_len;
        for (long long k = k0 + l; k < k1; k += L) {
            mom_load(P, atoms[k], has_aff, A, x);
            if constexpr (MODE == MOM_SPHERICAL) {
                const bool first = k < mid;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    acc[c] += first ? (double)x[c] : 0.0;
                    acc[3 + c] += first ? 0.0 : (double)x[c];
                }
            } else if constexpr (MODE == MOM_FLUCT) {
                const double d0 = (double)x[0] - ref[3 * k], d1 = (double)x[1] - ref[3 * k + 1], d2 = (double)x[2] - ref[3 * k + 2];
                acc[0] += d0 * d0 + d1 * d1 + d2 * d2;
            } else {
                const double w = weights ? (double)weights[k] : 1.0;
                acc[0] += w;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double a = (double)x[c] - s[c];             // (s = 0 but for MOM_GYRATION)
                    acc[1 + c] += w * a;
                    if constexpr (MODE == MOM_GYRATION) acc[4 + c] += w * a * a;
                }
            }
        }
    }
    al_group_sum(acc, glog2);
    if (!valid || l != 0) return;
    if constexpr (SEG) {
        double* o = part + (item * segs + seg) * REC;
#pragma unroll
        for (int k = 0; k < NV; ++k) o[k] = acc[k];
        if constexpr (MODE == MOM_GYRATION) { o[NV] = s[0]; o[NV + 1] = s[1]; o[NV + 2] = s[2]; }
    } else {
        mom_finish<MODE>(acc, s, f, g, G, n0, n1, out);
    }
}

// The fixed-order second stage: one wave per item, lane l sums the records of segments l, l + 64, ... in order, the lanes are folded
// by butterfly shuffles, lane 0 finishes the item (the shift: segment 0's, every segment of an item has the same).
template <int MODE>
MK_KERNEL(64) void k_mom_fold(const double* __restrict__ part, int segs, const unsigned* __restrict__ offsets, long long G,
                              void* __restrict__ out)
{
    constexpr int NV = mom_nv(MODE), REC = mom_rec(MODE);
    const long long item = blockIdx.x;
    const int lane = (int)threadIdx.x;
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    for (int sg = lane; sg < segs; sg += WAVE) {
        const double* r = part + (item * segs + sg) * REC;
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] += r[k];
    }
    al_group_sum(acc, 6);
    if (lane != 0) return;
    const long long f = MODE == MOM_SPHERICAL ? item : item / G;
    const long long g = MODE == MOM_SPHERICAL ? 0 : item - f * G;
    double s[3] = {0.0, 0.0, 0.0};
    if constexpr (MODE == MOM_GYRATION) {
        const double* r = part + item * segs * REC + NV;
        s[0] = r[0]; s[1] = r[1]; s[2] = r[2];
    }
    const long long b = offsets[g], mid = offsets[g + 1], e = MODE == MOM_SPHERICAL ? (long long)offsets[2] : mid;
    mom_finish<MODE>(acc, s, f, g, G, (double)(mid - b), (double)(e - mid), out);
}

// ref [n_sel, 3] float64: the mean over the F frames of selected atom k's (transformed) position.  A group of 2^glog2 lanes per atom,
// lane l sums frames l, l + L, ... in order, then the butterfly: a fixed order.  Grid: ceil(n_sel / (MOM_BLOCK >> glog2)) blocks.
MK_KERNEL(MOM_BLOCK) void k_mom_mean(const float* __restrict__ xyz, long long frame_floats, long long F, const double* __restrict__ affine,
                                     const unsigned* __restrict__ atoms, long long n_sel, int glog2, double* __restrict__ ref)
{
    const int L = 1 << glog2;
    const int l = (int)threadIdx.x & (L - 1);
    const long long k = (long long)blockIdx.x * (MOM_BLOCK >> glog2) + ((int)threadIdx.x >> glog2);
    const bool valid = k < n_sel;
    double acc[3] = {0.0, 0.0, 0.0};
    if (valid) {
        const unsigned atom = atoms[k];
        const bool has_aff = affine != nullptr;
        for (long long f = l; f < F; f += L) {
            double A[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) A[j] = has_aff ? affine[12 * f + j] : 0.0;
            float x[3];
            mom_load(xyz + f * frame_floats, atom, has_aff, A, x);
            acc[0] += (double)x[0]; acc[1] += (double)x[1]; acc[2] += (double)x[2];
        }
    }
    al_group_sum(acc, glog2);
    if (!valid || l != 0) return;
    ref[3 * k] = acc[0] / (double)F;
    ref[3 * k + 1] = acc[1] / (double)F;
    ref[3 * k + 2] = acc[2] / (double)F;
}

// out [F, n_sel] float64: sum_c (x_c - ref[k]_c)^2 of selected atom k in frame f; a lane per (f, k)
MK_KERNEL(MOM_BLOCK) void k_mom_fluct_atoms(const float* __restrict__ xyz, long long frame_floats, const double* __restrict__ affine,
                                            const unsigned* __restrict__ atoms, const double* __restrict__ ref, long long n_sel,
                                            long long n_items, double* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * MOM_BLOCK + threadIdx.x;
    if (i >= n_items) return;
    const long long f = i / n_sel, k = i - f * n_sel;
    const bool has_aff = affine != nullptr;
    double A[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) A[j] = has_aff ? affine[12 * f + j] : 0.0;
    float x[3];
    mom_load(xyz + f * frame_floats, atoms[k], has_aff, A, x);
    const double d0 = (double)x[0] - ref[3 * k], d1 = (double)x[1] - ref[3 * k + 1], d2 = (double)x[2] - ref[3 * k + 2];
    out[i] = d0 * d0 + d1 * d1 + d2 * d2;
}

}  // namespace mkamd
