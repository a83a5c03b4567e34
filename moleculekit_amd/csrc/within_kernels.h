// within_kernels.h -- HIP kernels of the proximity selection (moleculekit atomselect_utils.pyx: `within_distance`, the loop behind
// `within X of ...` / `exwithin X of ...`) on MI355X (gfx950): per frame one bit per query atom, "is any source atom closer than the
// cutoff" (DESIGN.md section 18).
//
// THE CONTRACT is the reference's, to the bit:
//   cutoff     a float32; sq_cutoff = cutoff * cutoff, a float32 product
//   pair test  diff = ((0 + dx dx) + dy dy) + dz dz with d = x_query - x_source per axis, every float32 operation rounded on its own
//              (mk_f*_rn: no multiply-add; 0 + t == t bit for bit where t is a square, so the first addition is not issued); within
//              where diff < sq_cutoff, strictly.  A NaN anywhere decides "not within"
//   gate       with the caller's six floats (min[3], max[3]) a query is looked at only where on SOME axis x >= min - cutoff or
//              x <= max + cutoff, float32 as written.  With finite min <= max and cutoff >= 0 it is always open; it closes with NaNs
//              and with a negative cutoff.  It is semantics, not an optimisation (within_gate)
//   result     one byte per (frame, query), queries in the order of sel1 (unsorted, duplicates, overlap with sel2: all allowed)
//
// THE SOURCES are compacted first (k_within_gather): [F][n2][3], so that the all-pairs kernel reads them at wave-uniform addresses.
//
// THE CULL (k_within_bounds, within_culled).  Per frame the bounding box [lo, hi] of the sources whose three coordinates are all
// finite.  A query with lo_k - x_k > |cutoff| or x_k - hi_k > |cutoff| on some axis k (the subtraction in float64) has no source
// within, for these reasons:
//   * a source with a non-finite coordinate is within of nothing: its diff is inf or NaN, and neither is < anything.  So only the
//     sources inside the box count.
//   * rounding is monotone.  Had the real difference lo_k - x_k been below |cutoff| (a float32, so a float64), its float64 rounding
//     would be <= |cutoff|; it is greater, so the real difference is >= |cutoff|, and so is s_k - x_k >= lo_k - x_k for every source
//     of the box.  The pair test's float32 difference d = x_k - s_k is the rounding of that: |d| >= |cutoff|.
//   * its float32 square is then >= the float32 square of |cutoff|, which is sq_cutoff (monotone again; both inf where it overflows).
//   * adding non-negative float32 terms to a float32 a never rounds below a.  So diff >= sq_cutoff, or diff is NaN: not within.
// A NaN query coordinate makes both comparisons false: not culled, and the loop finds nothing.  An empty box (no finite source) culls
// every query.  The plan applies the cull only where sq_cutoff is finite (within_pipeline.h): where the square overflows every finite
// pair is within, the first source ends the search, and nothing is gained by leaning on "inf < inf is false".
//
// THE CELL LIST (one large frame) is the bond guesser's (bond_kernels.h: k_bond_bounds .. k_bond_sort, as they are) over the compacted
// SOURCES only, the box side from clash_grid with |cutoff|.  k_within_pack writes the cell-ordered source records.  A query is not in
// the grid: k_within_cells computes its box per axis with the sources' arithmetic, UNCLIPPED (within_axis_box), and walks the 27 boxes
// around it that exist, ending at its first hit.
#pragma once
#include "bond_kernels.h"

namespace mkamd {

constexpr int WI_THREADS = 256;
constexpr int WI_CHECK = 8;                                           // sources between two looks at "is any lane still searching"
enum { WI_LO = 0, WI_HINV = 3, WI_WORDS = 8 };                         // per frame: keys of lo[3], inverted keys of hi[3]; filled with 0xff

struct WithinParams {
    float cutoff;                  // float32(cutoff)
    float sq_cutoff;               // cutoff * cutoff in float32
    float acut;                    // |cutoff|
    int cull;                      // != 0: the bounding-box cull applies (sq_cutoff is finite)
};

MK_DEV float within_unkey(unsigned k) { return mk_uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// the reference's gate, float32 as written: open where some axis has x >= min - cutoff or x <= max + cutoff.  b: min[3], max[3]
MK_DEV bool within_gate(float x, float y, float z, const float* __restrict__ b, float cutoff)
{
    return x >= mk_fsub_rn(b[0], cutoff) || x <= mk_fadd_rn(b[3], cutoff) || y >= mk_fsub_rn(b[1], cutoff) || y <= mk_fadd_rn(b[4], cutoff) ||
           z >= mk_fsub_rn(b[2], cutoff) || z <= mk_fadd_rn(b[5], cutoff);
}

// the cull (the argument stands at the head of this file).  box: the frame's WI_WORDS words
MK_DEV bool within_culled(float x, float y, float z, const unsigned* __restrict__ box, float acut)
{
    if (box[WI_LO] == 0xffffffffu) return true;                      // no source with three finite coordinates
    const double a = (double)acut;
    const float q[3] = {x, y, z};
    bool out = false;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const double lo = (double)within_unkey(box[WI_LO + ax]), hi = (double)within_unkey(~box[WI_HINV + ax]);
        out = out || lo - (double)q[ax] > a || (double)q[ax] - hi > a;
    }
    return out;
}

// diff < sq_cutoff, the reference's float32 sequence
MK_DEV bool within_pair(float x, float y, float z, float sx, float sy, float sz, float sq_cutoff)
{
    const float dx = mk_fsub_rn(x, sx), dy = mk_fsub_rn(y, sy), dz = mk_fsub_rn(z, sz);
    const float diff = mk_fadd_rn(mk_fadd_rn(mk_fmul_rn(dx, dx), mk_fmul_rn(dy, dy)), mk_fmul_rn(dz, dz));
    return diff < sq_cutoff;
}

// A load at a wave-uniform address of memory that no kernel of the same launch writes (the compacted sources): through the constant
// address space, so that the compiler takes the scalar unit and the value arrives in a scalar register, not in 64 lanes.
#ifdef MK_DEVICE_API_PROVIDED
MK_DEV float within_uniform_load(const float* p) { return *p; }      // (the host emulation)
#else
MK_DEV float within_uniform_load(const float* p) { return *(const __attribute__((address_space(4))) float*)p; }
#endif

// src [F][n2][3] = coords [F][N][3] at sel2.  Grid: frames x ceil(n2 / WI_THREADS) blocks, the frame slowest
MK_KERNEL(WI_THREADS) void k_within_gather(const float* __restrict__ coords, long long n_atoms, const unsigned* __restrict__ sel2, long long n2,
                                           unsigned blocks_per_frame, float* __restrict__ src)
{
    const unsigned f = blockIdx.x / blocks_per_frame;
    const long long j = (long long)(blockIdx.x - f * blocks_per_frame) * WI_THREADS + threadIdx.x;
    if (j >= n2) return;
    const float* c = coords + ((size_t)f * (size_t)n_atoms + (size_t)sel2[j]) * 3;
    float* s = src + ((size_t)f * (size_t)n2 + (size_t)j) * 3;
    s[0] = c[0]; s[1] = c[1]; s[2] = c[2];
}

// box [F][WI_WORDS] (0xff bytes from the host): the bounding box of the frame's sources whose three coordinates are all finite.
// Grid: frames x blocks_per_frame; a lane folds its sources, a wave folds its lanes, one lane of the wave issues the atomics.
MK_KERNEL(WI_THREADS) void k_within_bounds(const float* __restrict__ src, long long n2, unsigned blocks_per_frame, unsigned* __restrict__ box)
{
    const unsigned f = blockIdx.x / blocks_per_frame, part = blockIdx.x - f * blocks_per_frame;
    const float* s = src + (size_t)f * (size_t)n2 * 3;
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hinv[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
    for (long long j = (long long)part * WI_THREADS + threadIdx.x; j < n2; j += (long long)blocks_per_frame * WI_THREADS) {
        const float v[3] = {s[3 * j], s[3 * j + 1], s[3 * j + 2]};
        unsigned bad = 0u;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) bad |= (mk_float_bits(v[ax]) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;          // inf or NaN
        if (bad) continue;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const unsigned k = bond_key(v[ax]), ki = ~k;
            lo[ax] = k < lo[ax] ? k : lo[ax];
            hinv[ax] = ki < hinv[ax] ? ki : hinv[ax];
        }
    }
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const unsigned l = mk_shfl_down(lo[ax], d), h = mk_shfl_down(hinv[ax], d);
            lo[ax] = l < lo[ax] ? l : lo[ax];
            hinv[ax] = h < hinv[ax] ? h : hinv[ax];
        }
    }
    if ((threadIdx.x & (WAVE - 1)) == 0 && lo[0] != 0xffffffffu) {
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            mk_atomic_min(&box[(size_t)f * WI_WORDS + WI_LO + ax], lo[ax]);
            mk_atomic_min(&box[(size_t)f * WI_WORDS + WI_HINV + ax], hinv[ax]);
        }
    }
}

// the query of a lane: its coordinates, and whether the gate and the cull leave it anything to search.  gate: [F][2][3] or NULL
MK_DEV bool within_query(const float* __restrict__ coords, long long n_atoms, const unsigned* __restrict__ sel1, unsigned f, long long q,
                         const float* __restrict__ gate, const unsigned* __restrict__ box, const WithinParams& P, float* x, float* y, float* z)
{
    const float* c = coords + ((size_t)f * (size_t)n_atoms + (size_t)sel1[q]) * 3;
    *x = c[0]; *y = c[1]; *z = c[2];
    if (gate && !within_gate(*x, *y, *z, gate + (size_t)f * 6, P.cutoff)) return false;
    if (P.cull && within_culled(*x, *y, *z, box + (size_t)f * WI_WORDS, P.acut)) return false;
    return true;
}

// All pairs with early exit.  Grid: frames x ceil(n1 / WI_THREADS) blocks, the frame slowest; one lane owns one query of one frame.
// The source index is the same in every lane of a wave, so the sources may be loaded as scalars.  A lane that has its hit computes
// on (the result is sticky) rather than branch; every WI_CHECK sources the wave asks whether any lane still searches and leaves
// the loop when none does.
MK_KERNEL(WI_THREADS) void k_within_pairs(const float* __restrict__ coords, long long n_atoms, const unsigned* __restrict__ sel1, long long n1,
                                          const float* __restrict__ src, long long n2, const float* __restrict__ gate,
                                          const unsigned* __restrict__ box, WithinParams P, unsigned blocks_per_frame,
                                          unsigned char* __restrict__ out)
{
    const unsigned f = blockIdx.x / blocks_per_frame;
    const long long q = (long long)(blockIdx.x - f * blocks_per_frame) * WI_THREADS + threadIdx.x;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    const bool mine = q < n1;
    const bool search = mine && within_query(coords, n_atoms, sel1, f, q, gate, box, P, &x, &y, &z);
    bool hit = false;
    const float* s = src + (size_t)mk_uniform(f) * (size_t)n2 * 3;
    for (long long j = 0; j < n2; j += WI_CHECK) {
        if (mk_ballot(search && !hit) == 0ull) break;                // (wave-uniform)
        if (j + WI_CHECK <= n2) {
#pragma unroll
            for (int u = 0; u < WI_CHECK; ++u)
                hit = hit | within_pair(x, y, z, within_uniform_load(s + 3 * (j + u)), within_uniform_load(s + 3 * (j + u) + 1),
                                        within_uniform_load(s + 3 * (j + u) + 2), P.sq_cutoff);
        } else {
#pragma unroll 1
            for (long long t = j; t < n2; ++t)
                hit = hit | within_pair(x, y, z, within_uniform_load(s + 3 * t), within_uniform_load(s + 3 * t + 1), within_uniform_load(s + 3 * t + 2),
                                        P.sq_cutoff);
        }
    }
    if (mine) out[(size_t)f * (size_t)n1 + (size_t)q] = (search && hit) ? 1 : 0;
}

// the cell-ordered source records: position p of `order` holds source order[p]; 16 bytes a source, w unused
MK_KERNEL(WI_THREADS) void k_within_pack(long long m, const unsigned* __restrict__ order, const float* __restrict__ src, float4* __restrict__ rec)
{
    const long long p = (long long)blockIdx.x * WI_THREADS + threadIdx.x;
    if (p >= m) return;
    const size_t s = order[p];
    rec[p] = make_float4(src[3 * s], src[3 * s + 1], src[3 * s + 2], 0.0f);
}

// The box of a QUERY along one axis: the sources' arithmetic (bond_axis_box), but not clipped to the grid -- a query may lie outside
// it by any amount.  The float is clamped before it becomes an integer: below -2 (or NaN) -> -2, from 2^30 on -> 2^30; both are more
// than one box outside any grid (count <= 2^28), so such a query has no neighbour box on this axis.
MK_DEV int within_axis_box(float x, float mn, float pd)
{
    const float q = floorf(mk_fdiv_rn(mk_fsub_rn(x, mn), pd));
    if (!(q >= -2.0f)) return -2;
    if (q >= 1073741824.0f) return 1073741824;
    return (int)q;                                                   // (exact: |q| < 2^30)
}

// One large frame over the sources' cell list, a THREAD per query.  A source within |cutoff| of the query along an axis has a box
// index within one of the query's unclipped one (clash_grid's margin: within_pipeline.h), so the 27 boxes around the query's hold
// every source the pair test can accept.  The search of a lane ends at its first hit.
MK_KERNEL(WI_THREADS) void k_within_cells(const float* __restrict__ coords, long long n_atoms, const unsigned* __restrict__ sel1, long long n1,
                                          const float4* __restrict__ rec, BondGrid g, const unsigned* __restrict__ box_rank,
                                          const unsigned* __restrict__ start, const float* __restrict__ gate, const unsigned* __restrict__ box,
                                          WithinParams P, unsigned char* __restrict__ out)
{
    const long long q = (long long)blockIdx.x * WI_THREADS + threadIdx.x;
    if (q >= n1) return;
    float x, y, z;
    bool hit = false;
    if (within_query(coords, n_atoms, sel1, 0u, q, gate, box, P, &x, &y, &z)) {
        const int bx = within_axis_box(x, g.mn[0], g.pd), by = within_axis_box(y, g.mn[1], g.pd), bz = within_axis_box(z, g.mn[2], g.pd);
        const bool near = bx >= -1 && bx <= g.nx && by >= -1 && by <= g.ny && bz >= -1 && bz <= g.nz;
#pragma unroll 1
        for (int k = 0; near && !hit && k < 27; ++k) {
            const int kz = k / 9, ky = (k - 9 * kz) / 3, kx = k - 9 * kz - 3 * ky;
            const int cx = bx + kx - 1, cy = by + ky - 1, cz = bz + kz - 1;
            if (cx < 0 || cx >= g.nx || cy < 0 || cy >= g.ny || cz < 0 || cz >= g.nz) continue;
            const unsigned r = box_rank[((size_t)cz * (size_t)g.ny + (size_t)cy) * (size_t)g.nx + (size_t)cx];
            if (r == BOND_NONE) continue;
            const unsigned e = start[r + 1];
            for (unsigned p = start[r]; p < e && !hit; ++p) {
                const float4 S = rec[p];
                hit = within_pair(x, y, z, S.x, S.y, S.z, P.sq_cutoff);
            }
        }
    }
    out[q] = hit ? 1 : 0;
}

}  // namespace mkamd
