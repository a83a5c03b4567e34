// bond_kernels.h -- HIP kernels of the bond guesser (moleculekit bondguesser.py: `bond_grid_search`, and the pair test of
// bondguesser_utils.pyx) on MI355X (gfx950): one frame, a non-periodic grid.
//
// THE CONTRACT is the reference's, to the bit and to the ORDER of its list:
//   grid       per-axis float32 minimum; the box of an atom is floor((x - min) / pairdist) per axis, a float32 subtraction and a
//              correctly rounded float32 division by float32(pairdist), clipped to [0, count - 1], flattened z * nx * ny + y * nx + x.
//              The counts and pairdist come from the host (bond_pipeline.h: bond_grid)
//   pair test  skipped where both atoms are hydrogens; d = x_i - x_j per axis, dist2 = (dx dx + dy dy) + dz dz, every float32 operation
//              rounded on its own (mk_f*_rn: no multiply-add); rejected where dist2 > cutoff2 = float32(pairdist)^2, where
//              double(dist2) < 0.001 (the reference compares against the double literal), and where dist2 > cut * cut with
//              cut = float32(0.6 * double(r_i + r_j)) -- the sum and the square in float32.  Equality bonds
//   order      occupied boxes in the order of their LOWEST atom index (the reference walks a dict keyed by box in insertion order);
//              inside a box the owners i ascending; per owner the up-to-14 neighbour boxes in the reference's order (bond_rel), each
//              only where it exists; inside a neighbour box j ascending, in the owner's own box only j behind i.  Rows are (i, j) as
//              found: not sorted within themselves
//
// THE CELL LIST needs no sort.  k_bond_cells counts every box and takes the minimum atom index of it (integer atomics: the outcome
// does not depend on their order).  An atom that IS its box's minimum sets a flag; the exclusive scan of the flags over the atoms
// ranks the occupied boxes in the reference's order.  The occupancies by rank, scanned, are the boxes' starts.  The atoms drop into
// their box's range through the box's counter in whatever order the hardware takes them (k_bond_scatter), and then every atom
// counts the smaller indices of its own box and writes itself to start + that count (k_bond_sort): a rank sort, the same bits on
// every run.  `order` then holds the atoms in the reference's owner order, every box's atoms ascending.
//
// THE CAP: a box may hold at most BOND_BOX_CAP atoms.  The rank sort is quadratic in a box's atoms and the pair kernels walk up to 14
// such boxes per owner, so a frame that puts more into one box (the all-zero coordinates of an empty molecule; 4 097 coincident
// atoms) ends the call with a status -- the most crowded box and its occupancy -- instead of running for minutes.  The reference
// itself escalates the box side only by the box COUNT, so such frames exist; it then takes the same quadratic time on one thread.
//
// THE PAIRS: count -> scan -> fill over the owners in `order`, the same decision function in both passes.  Two lane assignments that
// produce the same list: a thread per owner (1-4 atoms a box at the usual 2.4-2.7 A box side: ~20 tests an owner), or a wave per
// owner with the lanes along the candidates of a neighbour box, a ballot's population for the count and its prefix for the ordered
// fill (an escalated grid over an unwrapped frame puts hundreds of atoms into a box).
#pragma once
#include "kernels.h"

#include <cstring>

namespace mkamd {

constexpr unsigned BOND_BOX_CAP = 4096;                               // atoms one box may hold
constexpr unsigned BOND_NONE = 0xffffffffu;                           // a box no atom is in (its `low` word)
constexpr int BD_THREADS = 256;

// status words of a call (device, read by the host between the stages)
enum { BD_MIN = 0, BD_MAX = 3, BD_NONFINITE = 6, BD_MAXOCC = 7, BD_CROWDED = 8, BD_NBOXES = 9, BD_TOTAL = 10 /* 64 bits */, BD_WORDS = 12 };

struct BondGrid { int nx, ny, nz; float pd, cutoff2; float mn[3]; };  // pd: float32(pairdist); cutoff2 = pd * pd in float32

// float32 -> unsigned key of the same order (and back): integer atomicMin / atomicMax then order floats.  -0 < +0 here, which no
// result depends on (x - (-0) == x - (+0) wherever the box index looks).
MK_DEV unsigned bond_key(float f) { const unsigned b = mk_float_bits(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
inline float bond_unkey(unsigned k)
{
    const unsigned b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// ------------------------------------------------------------------------------------------------
// Bounds: per-axis minimum and maximum keys, and whether any coordinate is not finite.  stat: BD_MIN.. = 0xffffffff, BD_MAX.. = 0,
// BD_NONFINITE = 0 from the host.  A lane folds its atoms, a wave folds its lanes, one lane of the wave issues the atomics.
// ------------------------------------------------------------------------------------------------
MK_KERNEL(BD_THREADS) void k_bond_bounds(const float* __restrict__ coords, long long n, unsigned* __restrict__ stat)
{
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, bad = 0u;
    for (long long a = (long long)blockIdx.x * BD_THREADS + threadIdx.x; a < n; a += (long long)gridDim.x * BD_THREADS) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const float v = coords[3 * a + ax];
            bad |= (mk_float_bits(v) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;          // inf or NaN
            const unsigned k = bond_key(v);
            lo[ax] = k < lo[ax] ? k : lo[ax];
            hi[ax] = k > hi[ax] ? k : hi[ax];
        }
    }
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const unsigned l = mk_shfl_down(lo[ax], d), h = mk_shfl_down(hi[ax], d);
            lo[ax] = l < lo[ax] ? l : lo[ax];
            hi[ax] = h > hi[ax] ? h : hi[ax];
        }
        bad |= mk_shfl_down(bad, d);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            mk_atomic_min(&stat[BD_MIN + ax], lo[ax]);
            mk_atomic_max(&stat[BD_MAX + ax], hi[ax]);
        }
        if (bad) mk_atomic_max(&stat[BD_NONFINITE], 1u);
    }
}

// the box of a coordinate along one axis (count >= 1; the coordinate is finite and >= mn, so the quotient is >= 0)
MK_DEV int bond_axis_box(float x, float mn, float pd, int count)
{
    const float q = floorf(mk_fdiv_rn(mk_fsub_rn(x, mn), pd));
    if (!(q > 0.0f)) return 0;
    if (q >= 1073741824.0f) return count - 1;                        // (count <= 2^28; below 2^30 the conversion is exact)
    const int iq = (int)q;
    return iq < count ? iq : count - 1;
}

// Cells: the box of every atom, the boxes' populations and lowest atom indices.  box_cnt zeroed, box_low = BOND_NONE by the host.
MK_KERNEL(BD_THREADS) void k_bond_cells(const float* __restrict__ coords, long long n, BondGrid g, unsigned* __restrict__ atom_box,
                                        unsigned* __restrict__ box_cnt, unsigned* __restrict__ box_low)
{
    const long long a = (long long)blockIdx.x * BD_THREADS + threadIdx.x;
    if (a >= n) return;
    const int bx = bond_axis_box(coords[3 * a + 0], g.mn[0], g.pd, g.nx), by = bond_axis_box(coords[3 * a + 1], g.mn[1], g.pd, g.ny),
              bz = bond_axis_box(coords[3 * a + 2], g.mn[2], g.pd, g.nz);
    const unsigned b = (unsigned)((bz * g.ny + by) * g.nx + bx);       // < nx ny nz <= 2^28
    atom_box[a] = b;
    mk_atomic_add(&box_cnt[b], 1u);
    mk_atomic_min(&box_low[b], (unsigned)a);
}

// flag[a] = 1 where atom a is the lowest index of its box (after k_bond_cells has finished)
MK_KERNEL(BD_THREADS) void k_bond_flags(long long n, const unsigned* __restrict__ atom_box, const unsigned* __restrict__ box_low,
                                        unsigned* __restrict__ flag)
{
    const long long a = (long long)blockIdx.x * BD_THREADS + threadIdx.x;
    if (a >= n) return;
    flag[a] = box_low[atom_box[a]] == (unsigned)a ? 1u : 0u;
}

// rank [n + 1]: the exclusive scan of the flags, so atom a is a box's lowest exactly where rank[a + 1] != rank[a] -- box_low is
// not read here and takes the box's RANK instead.  occ[rank] = the box's population; the status words take the largest population,
// the lowest box that exceeds the cap and the number of occupied boxes.
MK_KERNEL(BD_THREADS) void k_bond_ranks(long long n, const unsigned* __restrict__ atom_box, const unsigned* __restrict__ rank,
                                        const unsigned* __restrict__ box_cnt, unsigned* __restrict__ box_low, unsigned* __restrict__ occ,
                                        unsigned* __restrict__ stat)
{
    const long long a = (long long)blockIdx.x * BD_THREADS + threadIdx.x;
    if (a >= n) return;
    if (a == n - 1) stat[BD_NBOXES] = rank[n];
    const unsigned r = rank[a];
    if (rank[a + 1] == r) return;
    const unsigned b = atom_box[a], c = box_cnt[b];
    box_low[b] = r;
    occ[r] = c;
    mk_atomic_max(&stat[BD_MAXOCC], c);
    if (c > BOND_BOX_CAP) mk_atomic_min(&stat[BD_CROWDED], b);
}

// the atoms into their box's range, in any order: the box's counter runs down to zero
MK_KERNEL(BD_THREADS) void k_bond_scatter(long long n, const unsigned* __restrict__ atom_box, const unsigned* __restrict__ box_rank,
                                          const unsigned* __restrict__ start, unsigned* __restrict__ box_cnt, unsigned* __restrict__ tmp)
{
    const long long a = (long long)blockIdx.x * BD_THREADS + threadIdx.x;
    if (a >= n) return;
    const unsigned b = atom_box[a];
    const unsigned slot = mk_atomic_sub(&box_cnt[b], 1u) - 1u;        // in [0, population)
    tmp[start[box_rank[b]] + slot] = (unsigned)a;
}

// rank sort inside every box (at most BOND_BOX_CAP atoms: the host has checked)
MK_KERNEL(BD_THREADS) void k_bond_sort(long long n, const unsigned* __restrict__ atom_box, const unsigned* __restrict__ box_rank,
                                       const unsigned* __restrict__ start, const unsigned* __restrict__ tmp, unsigned* __restrict__ order)
{
    const long long a = (long long)blockIdx.x * BD_THREADS + threadIdx.x;
    if (a >= n) return;
    const unsigned r = box_rank[atom_box[a]], s = start[r], e = start[r + 1];
    unsigned below = 0;
    for (unsigned k = s; k < e; ++k) below += tmp[k] < (unsigned)a ? 1u : 0u;
    order[s + below] = (unsigned)a;
}

// ------------------------------------------------------------------------------------------------
// The pair test and the neighbour relations
// ------------------------------------------------------------------------------------------------
struct BondAtom { float x, y, z, r; unsigned h; };

MK_DEV BondAtom bond_load(const float* __restrict__ coords, const float* __restrict__ radii, const unsigned* __restrict__ is_h, unsigned a)
{
    BondAtom A;
    A.x = coords[3 * (size_t)a]; A.y = coords[3 * (size_t)a + 1]; A.z = coords[3 * (size_t)a + 2];
    A.r = radii[a];
    A.h = is_h[a];
    return A;
}

MK_DEV bool bond_is_close(const BondAtom& I, const BondAtom& J, float cutoff2)
{
    if (I.h && J.h) return false;
    const float dx = mk_fsub_rn(I.x, J.x), dy = mk_fsub_rn(I.y, J.y), dz = mk_fsub_rn(I.z, J.z);
    const float dist2 = mk_fadd_rn(mk_fadd_rn(mk_fmul_rn(dx, dx), mk_fmul_rn(dy, dy)), mk_fmul_rn(dz, dz));
    if (dist2 > cutoff2 || (double)dist2 < 0.001) return false;
    const float cut = (float)mk_dmul_rn(0.6, (double)mk_fadd_rn(I.r, J.r));
    if (dist2 > mk_fmul_rn(cut, cut)) return false;
    return true;
}

// the k-th of the reference's 14 neighbour relations as offsets in {-1, 0, +1}, two bits each (offset + 1), k = 0 in the low bits:
//   self, +x, +y, +z, +x+y, +x+z, +y+z, +x-y, -x+z, -y+z, +x+y+z, -x+y+z, +x-y+z, -x-y+z
constexpr unsigned bond_pack14(const int (&d)[14])
{
    unsigned v = 0;
    for (int k = 0; k < 14; ++k) v |= (unsigned)(d[k] + 1) << (2 * k);
    return v;
}
constexpr int BOND_DX[14] = {0, 1, 0, 0, 1, 1, 0, 1, -1, 0, 1, -1, 1, -1};
constexpr int BOND_DY[14] = {0, 0, 1, 0, 1, 0, 1, -1, 0, -1, 1, 1, -1, -1};
constexpr int BOND_DZ[14] = {0, 0, 0, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1};
constexpr unsigned BOND_RX = bond_pack14(BOND_DX), BOND_RY = bond_pack14(BOND_DY), BOND_RZ = bond_pack14(BOND_DZ);

// the candidates of relation k of the owner's box (bx, by, bz): positions [*s, *e) of `order`; false where the box does not exist
// or is empty.  In the owner's own box only what stands behind the owner (position p).
MK_DEV bool bond_rel(int k, int bx, int by, int bz, const BondGrid& g, unsigned p, const unsigned* __restrict__ box_rank,
                     const unsigned* __restrict__ start, unsigned* s, unsigned* e)
{
    const int x = bx + (int)((BOND_RX >> (2 * k)) & 3u) - 1, y = by + (int)((BOND_RY >> (2 * k)) & 3u) - 1,
              z = bz + (int)((BOND_RZ >> (2 * k)) & 3u) - 1;
    if (x < 0 || x >= g.nx || y < 0 || y >= g.ny || z >= g.nz) return false;       // (z never goes down)
    const unsigned r = box_rank[(z * g.ny + y) * g.nx + x];
    if (r == BOND_NONE) return false;
    *s = k == 0 ? p + 1u : start[r];
    *e = start[r + 1];
    return *s < *e;
}

// Pairs, a THREAD per owner: the owner at position p of `order`.  FILL = false: cnt[p] = its bonds, and their sum over the wave
// goes to the call's 64-bit total (one atomic per wave that found any); FILL = true: its rows from offs[p] onwards.
template <bool FILL>
MK_KERNEL(BD_THREADS) void k_bond_pairs_thread(const float* __restrict__ coords, const float* __restrict__ radii, const unsigned* __restrict__ is_h,
                                               long long n, BondGrid g, const unsigned* __restrict__ atom_box, const unsigned* __restrict__ box_rank,
                                               const unsigned* __restrict__ start, const unsigned* __restrict__ order, unsigned* __restrict__ cnt,
                                               const unsigned* __restrict__ offs, unsigned long long* __restrict__ total, int* __restrict__ pairs)
{
    const long long p = (long long)blockIdx.x * BD_THREADS + threadIdx.x;
    unsigned found = 0;
    if (p < n) {
        const unsigned i = order[p], b = atom_box[i];
        const BondAtom I = bond_load(coords, radii, is_h, i);
        const int bz = (int)(b / (unsigned)(g.nx * g.ny)), rem = (int)(b - (unsigned)bz * (unsigned)(g.nx * g.ny)), by = rem / g.nx, bx = rem - by * g.nx;
        size_t at = FILL ? (size_t)offs[p] : 0;
#pragma unroll 1
        for (int k = 0; k < 14; ++k) {
            unsigned s, e;
            if (!bond_rel(k, bx, by, bz, g, (unsigned)p, box_rank, start, &s, &e)) continue;
            for (unsigned q = s; q < e; ++q) {
                const unsigned j = order[q];
                if (!bond_is_close(I, bond_load(coords, radii, is_h, j), g.cutoff2)) continue;
                if constexpr (FILL) {
                    pairs[2 * at] = (int)i;
                    pairs[2 * at + 1] = (int)j;
                    ++at;
                }
                ++found;
            }
        }
        if constexpr (!FILL) cnt[p] = found;
    }
    if constexpr (!FILL) {
        unsigned sum = found;
#pragma unroll
        for (int d = WAVE / 2; d >= 1; d >>= 1) sum += mk_shfl_down(sum, d);
        if ((threadIdx.x & (WAVE - 1)) == 0 && sum) mk_atomic_add64(total, (unsigned long long)sum);
    }
}

// Pairs, a WAVE per owner: the lanes take 64 consecutive candidates of a neighbour box at a time; ascending (relation, candidate) is
// the reference's order, so a hit's row is the running position plus the hits in the lanes below it.
template <bool FILL>
MK_KERNEL(BD_THREADS) void k_bond_pairs_wave(const float* __restrict__ coords, const float* __restrict__ radii, const unsigned* __restrict__ is_h,
                                             long long n, BondGrid g, const unsigned* __restrict__ atom_box, const unsigned* __restrict__ box_rank,
                                             const unsigned* __restrict__ start, const unsigned* __restrict__ order, unsigned* __restrict__ cnt,
                                             const unsigned* __restrict__ offs, unsigned long long* __restrict__ total, int* __restrict__ pairs)
{
    const long long p = (long long)blockIdx.x * (BD_THREADS / WAVE) + (long long)mk_uniform(threadIdx.x >> 6);
    if (p >= n) return;                                              // (the whole wave)
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned i = order[p], b = atom_box[i];
    const BondAtom I = bond_load(coords, radii, is_h, i);
    const int bz = (int)(b / (unsigned)(g.nx * g.ny)), rem = (int)(b - (unsigned)bz * (unsigned)(g.nx * g.ny)), by = rem / g.nx, bx = rem - by * g.nx;
    size_t at = FILL ? (size_t)offs[p] : 0;
    unsigned found = 0;
#pragma unroll 1
    for (int k = 0; k < 14; ++k) {
        unsigned s, e;
        if (!bond_rel(k, bx, by, bz, g, (unsigned)p, box_rank, start, &s, &e)) continue;     // (wave-uniform)
        for (unsigned q0 = s; q0 < e; q0 += WAVE) {
            const unsigned q = q0 + (unsigned)lane;
            const bool valid = q < e;
            const unsigned j = order[valid ? q : e - 1u];            // past the end: the last candidate (computed, never counted)
            const bool hit = valid && bond_is_close(I, bond_load(coords, radii, is_h, j), g.cutoff2);
            const unsigned long long m = mk_ballot(hit);
            if constexpr (FILL) {
                if (hit) {
                    const size_t row = at + (size_t)mk_rank_in_mask(m);
                    pairs[2 * row] = (int)i;
                    pairs[2 * row + 1] = (int)j;
                }
                at += (size_t)mk_popc64(m);
            }
            found += (unsigned)mk_popc64(m);
        }
    }
    if constexpr (!FILL) {
        if (lane == 0) {
            cnt[p] = found;
            if (found) mk_atomic_add64(total, (unsigned long long)found);
        }
    }
}

}  // namespace mkamd
