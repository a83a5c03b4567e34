// sasa_kernels.h -- solvent-accessible surface area of trajectory frames (Shrake-Rupley; moleculekit's MetricSasa, which hands
// the work to mdtraj's sasa.cpp), include/mkamd_distance.h "surface area".  DESIGN.md section 9.
//
// Every decision is a comparison of two float32 values built by a fixed sequence of IEEE operations (separate multiplies and adds,
// mk_fmul_rn / mk_fadd_rn / mk_fsub_rn: never contracted), so the accessible COUNT of an atom is the reference's whatever the
// order in which neighbours are tested, and the area ((float32(4 pi / n) * count) * R) * R with it.
//
//   k_sasa_pack     per (frame, atom): {x / div, y / div, z / div, R} as one float4 (div = 10 turns Angstrom into the reference's
//                   nanometres with the reference's IEEE division; div = 1 copies); frame 0's threads also check the mapping
//                   (inside [0, n_out), non-decreasing: equal values are then contiguous -- what the ordered sums rely on)
//   k_sasa_count    a workgroup per (frame, atom); atoms outside the selection leave at once.  The four waves scan the frame's
//                   atoms (one 16-byte load each) for neighbours |x_i - x_j|^2 < (R_i + R_j)^2 and append {x_j, R_j^2} to a list in
//                   LDS; then a lane per sphere point walks the list (every lane reads the same entry: an LDS broadcast) and leaves
//                   at the first neighbour that buries its point; accessible points are counted by ballot.  An atom with more
//                   neighbours than the list holds (SA_MAX_NB) tests its points against the frame's atoms in global memory, the
//                   neighbour condition evaluated on the way: same count.  Two atoms closer than sqrt(1e-10) set the refusal flag.
//   k_sasa_scatter  a lane per (frame, atom): the first atom of each run of equal mapping values adds the run's selected areas to
//                   out[frame, mapping] one after the other in float32 (the reference's order).  No floating-point atomics: the
//                   same bits on every run.  Writes nothing once a refusal flag is set.
#pragma once
#ifndef MK_DEVICE_API_PROVIDED
#include "mk_device.h"
#endif

namespace mkamd {

constexpr int SA_BLOCK = 256;
constexpr int SA_MAX_NB = 1024;             // neighbours of one atom kept in LDS (16 KB); proteins have 40-90
constexpr float SA_COINCIDENT_R2 = 1e-10f;  // the reference aborts the process below this squared distance (its nanometres)
enum SasaError { SA_ERR_COINCIDENT = 1, SA_ERR_MAP_RANGE = 2, SA_ERR_MAP_ORDER = 4 };

// ((dx dx + dy dy) + dz dz), one rounding per operation
MK_DEV float sa_dist2(float ax, float ay, float az, float bx, float by, float bz)
{
    const float dx = mk_fsub_rn(ax, bx), dy = mk_fsub_rn(ay, by), dz = mk_fsub_rn(az, bz);
    return mk_fadd_rn(mk_fadd_rn(mk_fmul_rn(dx, dx), mk_fmul_rn(dy, dy)), mk_fmul_rn(dz, dz));
}

MK_KERNEL(SA_BLOCK) void k_sasa_pack(const float* __restrict__ xyz, const float* __restrict__ radii, long long n_atoms, long long n_items,
                                     float div, const int* __restrict__ mapping, long long n_out, int check_mapping,
                                     float4* __restrict__ packed, int* __restrict__ err)
{
    const long long t = (long long)blockIdx.x * SA_BLOCK + threadIdx.x;
    if (t >= n_items) return;
    const long long i = t % n_atoms;
    float x = xyz[3 * t], y = xyz[3 * t + 1], z = xyz[3 * t + 2];
    if (div != 1.0f) { x = mk_fdiv_rn(x, div); y = mk_fdiv_rn(y, div); z = mk_fdiv_rn(z, div); }
    packed[t] = make_float4(x, y, z, radii[i]);
    if (check_mapping && t < n_atoms) {
        const int m = mapping[i];
        if (m < 0 || m >= n_out) mk_atomic_or(err, SA_ERR_MAP_RANGE);
        if (i > 0 && m < mapping[i - 1]) mk_atomic_or(err, SA_ERR_MAP_ORDER);
    }
}

// packed [n_frames][n_atoms]; points [n_points][3]; area [n_frames][n_atoms] (selected atoms only are written)
MK_KERNEL(SA_BLOCK) void k_sasa_count(const float4* __restrict__ packed, int n_atoms, const int* __restrict__ mask,
                                      const float* __restrict__ points, int n_points, float area_const, float* __restrict__ area,
                                      int* __restrict__ err)
{
    __shared__ float4 nb[SA_MAX_NB];
    __shared__ unsigned n_nb, n_free;
    const long long item = blockIdx.x;
    const int i = (int)(item % n_atoms);
    if (!mask[i]) return;                                               // (uniform over the workgroup)
    const float4* __restrict__ fr = packed + (item - i);
    const int tid = (int)threadIdx.x;
    if (tid == 0) { n_nb = 0; n_free = 0; }
    mk_block_sync();
    const float4 me = fr[i];
    for (int j = tid; j < n_atoms; j += SA_BLOCK) {
        if (j == i) continue;
        const float4 o = fr[j];
        const float r2 = sa_dist2(me.x, me.y, me.z, o.x, o.y, o.z);
        const float cut = mk_fadd_rn(me.w, o.w);
        if (r2 < mk_fmul_rn(cut, cut)) {
            const unsigned at = mk_lds_add(&n_nb, 1u);
            if (at < (unsigned)SA_MAX_NB) nb[at] = make_float4(o.x, o.y, o.z, mk_fmul_rn(o.w, o.w));
        }
        if (r2 < SA_COINCIDENT_R2) mk_atomic_or(err, SA_ERR_COINCIDENT);
    }
    mk_block_sync();
    const int count = (int)n_nb;
    const bool in_lds = count <= SA_MAX_NB;
    int mine = 0;
    for (int p0 = 0; p0 < n_points; p0 += SA_BLOCK) {                  // (uniform trip count: the ballot below takes every lane)
        const int p = p0 + tid;
        bool open = p < n_points;
        if (open) {
            const float px = mk_fadd_rn(me.x, mk_fmul_rn(me.w, points[3 * p]));
            const float py = mk_fadd_rn(me.y, mk_fmul_rn(me.w, points[3 * p + 1]));
            const float pz = mk_fadd_rn(me.z, mk_fmul_rn(me.w, points[3 * p + 2]));
            if (in_lds) {
                for (int k = 0; k < count; ++k) {
                    const float4 o = nb[k];
                    if (sa_dist2(px, py, pz, o.x, o.y, o.z) < o.w) { open = false; break; }
                }
            } else {
                for (int j = 0; j < n_atoms; ++j) {
                    if (j == i) continue;
                    const float4 o = fr[j];
                    const float cut = mk_fadd_rn(me.w, o.w);
                    if (sa_dist2(me.x, me.y, me.z, o.x, o.y, o.z) < mk_fmul_rn(cut, cut) &&
                        sa_dist2(px, py, pz, o.x, o.y, o.z) < mk_fmul_rn(o.w, o.w)) { open = false; break; }
                }
            }
        }
        mine += mk_popc64(mk_ballot(open));
    }
    if ((tid & 63) == 0) mk_lds_add(&n_free, (unsigned)mine);
    mk_block_sync();
    if (tid == 0) area[item] = mk_fmul_rn(mk_fmul_rn(mk_fmul_rn(area_const, (float)n_free), me.w), me.w);
}

// out [n_frames][n_out]
MK_KERNEL(SA_BLOCK) void k_sasa_scatter(const float* __restrict__ area, long long n_atoms, long long n_items, const int* __restrict__ mapping,
                                        const int* __restrict__ mask, long long n_out, float* __restrict__ out, const int* __restrict__ err)
{
    const long long t = (long long)blockIdx.x * SA_BLOCK + threadIdx.x;
    if (t >= n_items || *err) return;
    const long long i = t % n_atoms, f = t / n_atoms;
    const int m = mapping[i];
    if (i > 0 && mapping[i - 1] == m) return;                           // not the first atom of its run
    const float* a = area + f * n_atoms;
    float acc = out[f * n_out + m];
    bool any = false;
    for (long long j = i; j < n_atoms && mapping[j] == m; ++j)
        if (mask[j]) { acc = mk_fadd_rn(acc, a[j]); any = true; }
    if (any) out[f * n_out + m] = acc;
}

}  // namespace mkamd
