// clash_kernels.h -- HIP kernels of the steric-clash search (moleculekit distance.py: `find_clashes`) on MI355X (gfx950): one frame, two
// selections, a per-pair threshold, an exclusion table, values in the output.
//
// THE CONTRACT is the reference's, to the bit:
//   candidates  owners a from the first selection, partners b from the second; in self mode (one selection) only a < b
//   pair test   float32: d = x_a - x_b per axis, dist2 = (dx dx + dy dy) + dz dz, every operation rounded on its own (mk_f*_rn: no
//               multiply-add), dist = the correctly rounded root; a clash where dist < float32(float32(r_a + r_b) - float32(overlap)),
//               strictly; overlap of the pair = float32(float32(r_a + r_b) - dist)
//   pre-filter  the reference finds its candidates with a kd-tree over the coordinates widened to float64: a pair passes where
//               (dx dx + dy dy) + dz dz in float64, every operation rounded on its own, is <= cutoff * cutoff.  Only pairs within a few
//               ulps of the largest threshold can fail it, so it is evaluated for the pairs that passed the float32 test
//   exclusions  a CSR over the atoms: row a holds, ascending, the partners b >= a the pair (a, b) is excluded with.  The reference
//               looks a row (a, b) up AS FOUND in a set of (min, max) tuples, so a row with a > b is never excluded: no look-up then
//
// THE CELL LIST is the bond guesser's (bond_kernels.h: k_bond_bounds .. k_bond_sort, as they are), built over the atoms of either
// selection: k_clash_select flags them, a scan numbers them, k_clash_compact gathers their coordinates.  After the sort k_clash_pack
// writes one cell-ordered record per atom -- x, y, z and the radius as ONE 16-byte element, the atom's index, its selection bits, its
// box -- so that a box's candidates are contiguous 16-byte loads.  k_clash_owners lists the positions of the first selection's atoms.
//
// THE PAIRS: count -> scan -> fill over the owners, the same decision function in both passes; an owner walks the 27 boxes around its
// own, z slowest, and a box's candidates in their (ascending) order, so the rows leave the fill in one defined order.  A thread per
// owner, or a wave per owner with the lanes along 64 consecutive candidates, a ballot's population for the count and its prefix for
// the fill.  The fill writes (a, b), dist and overlap.
#pragma once
#include "bond_kernels.h"

namespace mkamd {

constexpr int CL_THREADS = 256;
constexpr unsigned CL_SEL1 = 1u, CL_SEL2 = 2u;                        // selection bits of an atom

struct ClashParams {
    float overlap;                 // float32(overlap)
    double cutoff2;                // cutoff * cutoff in float64, cutoff = 2 max(radii) - overlap
    int self_mode;                 // != 0: one selection, pairs a < b
};

MK_DEV unsigned clash_bits(const unsigned* __restrict__ sel1, const unsigned* __restrict__ sel2, int self_mode, long long a)
{
    const unsigned s1 = sel1[a] ? CL_SEL1 : 0u;
    if (self_mode) return s1 ? (CL_SEL1 | CL_SEL2) : 0u;
    return s1 | (sel2[a] ? CL_SEL2 : 0u);
}

// flag[a] = 1 where atom a is in either selection
MK_KERNEL(CL_THREADS) void k_clash_select(const unsigned* __restrict__ sel1, const unsigned* __restrict__ sel2, int self_mode, long long n,
                                          unsigned* __restrict__ flag)
{
    const long long a = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (a >= n) return;
    flag[a] = clash_bits(sel1, sel2, self_mode, a) ? 1u : 0u;
}

// pos [n + 1]: the exclusive scan of the flags.  The selected atoms' coordinates and indices, ascending
MK_KERNEL(CL_THREADS) void k_clash_compact(const float* __restrict__ coords, long long n, const unsigned* __restrict__ pos,
                                           float* __restrict__ sub_coords, unsigned* __restrict__ sub_atom)
{
    const long long a = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (a >= n) return;
    const unsigned s = pos[a];
    if (pos[a + 1] == s) return;
    sub_coords[3 * (size_t)s] = coords[3 * a];
    sub_coords[3 * (size_t)s + 1] = coords[3 * a + 1];
    sub_coords[3 * (size_t)s + 2] = coords[3 * a + 2];
    sub_atom[s] = (unsigned)a;
}

// the cell-ordered records: position p of `order` holds selected atom order[p]
MK_KERNEL(CL_THREADS) void k_clash_pack(long long m, const unsigned* __restrict__ order, const float* __restrict__ sub_coords,
                                        const unsigned* __restrict__ sub_atom, const unsigned* __restrict__ sub_box, const float* __restrict__ radii,
                                        const unsigned* __restrict__ sel1, const unsigned* __restrict__ sel2, int self_mode, float4* __restrict__ rec,
                                        unsigned* __restrict__ idx, unsigned* __restrict__ bits, unsigned* __restrict__ box, unsigned* __restrict__ own)
{
    const long long p = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (p >= m) return;
    const unsigned s = order[p], a = sub_atom[s];
    rec[p] = make_float4(sub_coords[3 * (size_t)s], sub_coords[3 * (size_t)s + 1], sub_coords[3 * (size_t)s + 2], radii[a]);
    idx[p] = a;
    const unsigned b = clash_bits(sel1, sel2, self_mode, (long long)a);
    bits[p] = b;
    box[p] = sub_box[s];
    own[p] = b & CL_SEL1;
}

// opos [m + 1]: the exclusive scan of `own`.  owner[k] = the position of the k-th atom of the first selection, in cell order
MK_KERNEL(CL_THREADS) void k_clash_owners(long long m, const unsigned* __restrict__ opos, unsigned* __restrict__ owner)
{
    const long long p = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (p >= m) return;
    const unsigned k = opos[p];
    if (opos[p + 1] != k) owner[k] = (unsigned)p;
}

// ------------------------------------------------------------------------------------------------
// The pair test
// ------------------------------------------------------------------------------------------------
// is b in the ascending row [s, e) of the exclusion table?
MK_DEV bool clash_excluded(const unsigned* __restrict__ ex_partner, unsigned s, unsigned e, unsigned b)
{
    while (s < e) {
        const unsigned mid = s + ((e - s) >> 1);
        const unsigned v = ex_partner[mid];
        if (v == b) return true;
        if (v < b) s = mid + 1u; else e = mid;
    }
    return false;
}

// The arithmetic of a pair, for every lane alike (the root's slow path is a wave-wide decision): dist and the sum of the radii.
MK_DEV void clash_dist(const float4& A, const float4& B, float* dist, float* vsum)
{
    const float dx = mk_fsub_rn(A.x, B.x), dy = mk_fsub_rn(A.y, B.y), dz = mk_fsub_rn(A.z, B.z);
    const float dist2 = mk_fadd_rn(mk_fadd_rn(mk_fmul_rn(dx, dx), mk_fmul_rn(dy, dy)), mk_fmul_rn(dz, dz));
    *dist = mk_fsqrt_rn(dist2);
    *vsum = mk_fadd_rn(A.w, B.w);
}

// ... and the decision: the selection, the order of a self pair, the float32 threshold, the float64 pre-filter, the exclusion table
MK_DEV bool clash_is_hit(const float4& A, unsigned ia, const float4& B, unsigned ib, unsigned bbits, float dist, float vsum, const ClashParams& P,
                         const unsigned* __restrict__ ex_start, const unsigned* __restrict__ ex_partner)
{
    if (!(bbits & CL_SEL2)) return false;
    if (P.self_mode && !(ia < ib)) return false;
    if (!(dist < mk_fsub_rn(vsum, P.overlap))) return false;
    const double ex = (double)A.x - (double)B.x, ey = (double)A.y - (double)B.y, ez = (double)A.z - (double)B.z;
    const double d2 = mk_dadd_rn(mk_dadd_rn(mk_dmul_rn(ex, ex), mk_dmul_rn(ey, ey)), mk_dmul_rn(ez, ez));
    if (!(d2 <= P.cutoff2)) return false;
    if (ex_start && ia <= ib && clash_excluded(ex_partner, ex_start[ia], ex_start[ia + 1u], ib)) return false;
    return true;
}

// the candidates of neighbour k (0 .. 26: dx fastest, dz slowest, each -1 .. +1) of the box (bx, by, bz): positions [*s, *e) of the
// records; false where the box does not exist or is empty
MK_DEV bool clash_rel(int k, int bx, int by, int bz, const BondGrid& g, const unsigned* __restrict__ box_rank, const unsigned* __restrict__ start,
                      unsigned* s, unsigned* e)
{
    const int kz = k / 9, ky = (k - 9 * kz) / 3, kx = k - 9 * kz - 3 * ky;
    const int x = bx + kx - 1, y = by + ky - 1, z = bz + kz - 1;
    if (x < 0 || x >= g.nx || y < 0 || y >= g.ny || z < 0 || z >= g.nz) return false;
    const unsigned r = box_rank[(z * g.ny + y) * g.nx + x];
    if (r == BOND_NONE) return false;
    *s = start[r];
    *e = start[r + 1];
    return *s < *e;
}

MK_DEV void clash_write(size_t row, unsigned ia, unsigned ib, float dist, float vsum, int* __restrict__ pairs, float* __restrict__ dists,
                        float* __restrict__ overs)
{
    pairs[2 * row] = (int)ia;
    pairs[2 * row + 1] = (int)ib;
    dists[row] = dist;
    overs[row] = mk_fsub_rn(vsum, dist);
}

// Pairs, a THREAD per owner: the k-th owner.  FILL = false: cnt[k] = its rows, and their sum over the wave goes to the call's 64-bit
// total (one atomic per wave that found any); FILL = true: its rows from offs[k] onwards.
template <bool FILL>
MK_KERNEL(CL_THREADS) void k_clash_pairs_thread(const float4* __restrict__ rec, const unsigned* __restrict__ idx, const unsigned* __restrict__ bits,
                                                const unsigned* __restrict__ box, const unsigned* __restrict__ owner, long long n_owners, BondGrid g,
                                                ClashParams P, const unsigned* __restrict__ box_rank, const unsigned* __restrict__ start,
                                                const unsigned* __restrict__ ex_start, const unsigned* __restrict__ ex_partner,
                                                unsigned* __restrict__ cnt, const unsigned* __restrict__ offs, unsigned long long* __restrict__ total,
                                                int* __restrict__ pairs, float* __restrict__ dists, float* __restrict__ overs)
{
    const long long k0 = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
    unsigned found = 0;
    if (k0 < n_owners) {
        const unsigned p = owner[k0], ia = idx[p], b = box[p];
        const float4 A = rec[p];
        const int bz = (int)(b / (unsigned)(g.nx * g.ny)), rem = (int)(b - (unsigned)bz * (unsigned)(g.nx * g.ny)), by = rem / g.nx, bx = rem - by * g.nx;
        size_t at = FILL ? (size_t)offs[k0] : 0;
#pragma unroll 1
        for (int k = 0; k < 27; ++k) {
            unsigned s, e;
            if (!clash_rel(k, bx, by, bz, g, box_rank, start, &s, &e)) continue;
            for (unsigned q = s; q < e; ++q) {
                const float4 B = rec[q];
                float dist, vsum;
                clash_dist(A, B, &dist, &vsum);
                const unsigned ib = idx[q];
                if (!clash_is_hit(A, ia, B, ib, bits[q], dist, vsum, P, ex_start, ex_partner)) continue;
                if constexpr (FILL) clash_write(at++, ia, ib, dist, vsum, pairs, dists, overs);
                ++found;
            }
        }
        if constexpr (!FILL) cnt[k0] = found;
    }
    if constexpr (!FILL) {
        unsigned sum = found;
#pragma unroll
        for (int d = WAVE / 2; d >= 1; d >>= 1) sum += mk_shfl_down(sum, d);
        if ((threadIdx.x & (WAVE - 1)) == 0 && sum) mk_atomic_add64(total, (unsigned long long)sum);
    }
}

// Pairs, a WAVE per owner: the lanes take 64 consecutive candidates of a neighbour box at a time; ascending (box, candidate) is the
// order of the thread kernel, so a hit's row is the running position plus the hits in the lanes below it.
template <bool FILL>
MK_KERNEL(CL_THREADS) void k_clash_pairs_wave(const float4* __restrict__ rec, const unsigned* __restrict__ idx, const unsigned* __restrict__ bits,
                                              const unsigned* __restrict__ box, const unsigned* __restrict__ owner, long long n_owners, BondGrid g,
                                              ClashParams P, const unsigned* __restrict__ box_rank, const unsigned* __restrict__ start,
                                              const unsigned* __restrict__ ex_start, const unsigned* __restrict__ ex_partner,
                                              unsigned* __restrict__ cnt, const unsigned* __restrict__ offs, unsigned long long* __restrict__ total,
                                              int* __restrict__ pairs, float* __restrict__ dists, float* __restrict__ overs)
{
    const long long k0 = (long long)blockIdx.x * (CL_THREADS / WAVE) + (long long)mk_uniform(threadIdx.x >> 6);
    if (k0 >= n_owners) return;                                      // (the whole wave)
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned p = owner[k0], ia = idx[p], b = box[p];
    const float4 A = rec[p];
    const int bz = (int)(b / (unsigned)(g.nx * g.ny)), rem = (int)(b - (unsigned)bz * (unsigned)(g.nx * g.ny)), by = rem / g.nx, bx = rem - by * g.nx;
    size_t at = FILL ? (size_t)offs[k0] : 0;
    unsigned found = 0;
#pragma unroll 1
    for (int k = 0; k < 27; ++k) {
        unsigned s, e;
        if (!clash_rel(k, bx, by, bz, g, box_rank, start, &s, &e)) continue;       // (wave-uniform)
        for (unsigned q0 = s; q0 < e; q0 += WAVE) {
            const unsigned q = q0 + (unsigned)lane;
            const bool valid = q < e;
            const unsigned qq = valid ? q : e - 1u;                  // past the end: the last candidate (computed, never counted)
            const float4 B = rec[qq];
            float dist, vsum;
            clash_dist(A, B, &dist, &vsum);
            const unsigned ib = idx[qq];
            const bool hit = valid && clash_is_hit(A, ia, B, ib, bits[qq], dist, vsum, P, ex_start, ex_partner);
            const unsigned long long m = mk_ballot(hit);
            if constexpr (FILL) {
                if (hit) clash_write(at + (size_t)mk_rank_in_mask(m), ia, ib, dist, vsum, pairs, dists, overs);
                at += (size_t)mk_popc64(m);
            }
            found += (unsigned)mk_popc64(m);
        }
    }
    if constexpr (!FILL) {
        if (lane == 0) {
            cnt[k0] = found;
            if (found) mk_atomic_add64(total, (unsigned long long)found);
        }
    }
}

}  // namespace mkamd
