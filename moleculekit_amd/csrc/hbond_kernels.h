// hbond_kernels.h -- HIP kernels of the hydrogen bonds (moleculekit interactions/hbonds/hbonds.pyx: `calculate`) on MI355X (gfx950):
// every (donor row, acceptor) pair the two selections allow, in every frame of a trajectory.
//
// THE TERMS are the reference's float32 arithmetic to the bit -- what its generated C++ computes, every operation rounded on its own:
//   wrapped vec  per axis val = c[a] - c[d] (d: the hydrogen; the heavy atom under ignore_hs); ONLY where |val| > box / 2 and box != 0:
//                val = val - box * roundf(val / box), all float32; d2 a sum from 0 of val * val
//   distance     the pair is dropped where d2_a > thr_d2 (a NaN passes); ignore_hs: reported here
//   angle        second vector c[heavy] - c[hydrogen], wrapped the same way; dropped where d2_a == 0 or d2_b == 0; dot a sum from 0 of
//                rounded products; ratio = float32(double(dot) / double(float32(sqrtf(d2_a) * sqrtf(d2_b)))), clamped to [-1, 1] (a NaN
//                passes both clamps); reported where acosf(ratio) > thr_ang in float32
// The ratio's division widens float32 operands and narrows the float64 quotient: for float32 operands that IS the correctly rounded
// float32 quotient (53 >= 2 * 24 + 2 bits), which is what ring_div computes; ring_sqrt is the correctly rounded sqrtf and ring_acosf the
// C library's acosf (ring_kernels.h).  No float32 multiply-add is fused anywhere (mk_f*_rn).
//
// THE PAIR SPACE is the ALLOWED pairs, not donors x acceptors.  Whether a pair is allowed depends on the donor's HEAVY atom and on the
// acceptor alone, so a donor row is held against one of three order-preserving SUBLISTS of the acceptors (class 0: those in sel1 -- rows
// whose heavy atom is in sel2 only, and every row of an intra call; class 1: those in sel2 -- heavy atom in sel1 only; class 2: those in
// either -- heavy atom in both); rows whose heavy atom is in neither selection do not exist here.  A row's pairs are cut into TILES of 64
// consecutive entries of its sublist; the tiles are numbered row after row (HbRow::tile0), so ascending (tile, bit) is the reference's
// order: donors outer, acceptors inner.
//
// Per chunk of frames: a count kernel leaves a 64-bit mask per (tile, frame) and adds its population to the counter of the tile's ROW
// (integer atomics, only where a bit is set: the sums do not depend on the order); k_contacts_scan (dist_kernels.h) turns the rows'
// counters into per-frame prefixes -- over the rows, not the tiles: with 16 tiles a row it is a sixteenth of the work, and the scan has
// only one block per 64 frames --; the fill kernel walks the tiles of a row and their set bits and writes int32 (heavy, hydrogen | -1,
// acceptor).
// Two lane assignments: lanes along FRAMES (coordinates are frame-fastest: every load coalesced; a wave keeps hbond_group() donor rows of one
// class in registers and holds each acceptor it loads against all of them -- the acceptor's re-read is what bounds the kernel), or
// along the ACCEPTORS of one tile in ONE frame (single poses and short trajectories; the mask is a ballot).
#pragma once
#include "ring_kernels.h"

namespace mkamd {

constexpr int HB_TILE = 64;                                          // sublist entries per mask
// donor rows a frame-lane wave keeps in registers: what fits 64 of them (with hydrogens a row is seven floats and the angle's tail)
constexpr int hbond_group(bool hs) { return hs ? 2 : 4; }

struct HbRow { unsigned heavy, ref, tile0, cls; };                   // ref: the hydrogen (the heavy atom again under ignore_hs); tile0: its first tile
struct HbThr { float d2, ang; };                                     // threshold^2 (float32 product); the angle threshold in radians
// the three sublists inside `acc` (off, len), the rows of each class inside `crow` (coff, cnum) and where each class's work items --
// (group of hbond_group() rows, tile) -- begin in the frame-lane grid (wstart[3]: their number)
struct HbPlan { unsigned off[3], len[3], coff[3], cnum[3], wstart[4]; };

// v[c] of a class that is not a compile-time constant (a kernel argument indexed at run time would move to scratch)
MK_DEV unsigned hbond_pick(const unsigned (&v)[3], unsigned c) { return c == 0u ? v[0] : (c == 1u ? v[1] : v[2]); }

// _wrapped vector p1 - p2 and its squared length
MK_DEV float hbond_wvec(const float (&p1)[3], const float (&p2)[3], const float (&bx)[3], float (&v)[3])
{
    float d2 = 0.0f;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        float val = mk_fsub_rn(p1[ax], p2[ax]);
        const float half = mk_fmul_rn(bx[ax], 0.5f);                 // box / 2 (exact)
        if (mk_abs(val) > half && bx[ax] != 0.0f) val = mk_fsub_rn(val, mk_fmul_rn(bx[ax], roundf(ring_div(val, bx[ax]))));
        v[ax] = val;
        d2 = mk_fadd_rn(d2, mk_fmul_rn(val, val));
    }
    return d2;
}

MK_DEV void hbond_atom(const float* __restrict__ coords, long long F, unsigned atom, size_t f, float (&p)[3])
{
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) p[ax] = ring_coord(coords, F, atom, ax, (long long)f);
}

// a donor row in one frame: the position the acceptors are measured from and, with hydrogens, the wrapped vector heavy - hydrogen and
// the root of its squared length (0 exactly where d2_b == 0: the pair is dropped)
template <bool HS>
struct HbDonor {
    float ref[3], vb[3], sb;
    MK_DEVFN void load(const float* __restrict__ coords, long long F, const HbRow& r, size_t f, const float (&bx)[3])
    {
        hbond_atom(coords, F, r.ref, f, ref);
        if constexpr (HS) {
            float h[3];
            hbond_atom(coords, F, r.heavy, f, h);
            sb = ring_sqrt(hbond_wvec(h, ref, bx, vb));
        }
    }
};

// does the reference report (donor row, acceptor at pa)?  (acceptor == heavy atom and the selections: the caller's)
template <bool HS>
MK_DEV bool hbond_pair(const HbDonor<HS>& d, const float (&pa)[3], const float (&bx)[3], const HbThr& T)
{
    float va[3];
    const float d2a = hbond_wvec(pa, d.ref, bx, va);
    if (d2a > T.d2) return false;                                    // (a NaN goes on)
    if constexpr (!HS) {
        return true;
    } else {
        if (d2a == 0.0f || d.sb == 0.0f) return false;
        float ratio = ring_div(ring_dot(va, d.vb), mk_fmul_rn(ring_sqrt(d2a), d.sb));
        if (ratio > 1.0f) ratio = 1.0f;
        if (ratio < -1.0f) ratio = -1.0f;
        return ring_acosf(ratio) > T.ang;                            // (NaN: not reported)
    }
}

// ------------------------------------------------------------------------------------------------
// Count, lanes along frames.  A wave: 64 frames x one work item = (a group of up to HB_G rows of one class, one tile of the class's
// sublist); the acceptor is wave-uniform and is loaded once for the group's rows.  masks [tile][pitch], cnt [row][pitch] (zeroed by the
// host); frames past the chunk compute on its last frame and store nothing; rows past the group's end compute on its last row and store
// nothing.
// ------------------------------------------------------------------------------------------------
constexpr int HC_THREADS = 256;

template <bool HS, int HB_G>
MK_KERNEL(HC_THREADS) void k_hbond_count_frames(const float* __restrict__ coords, long long F, long long f0, long long fc, long long pitch,
                                                const float* __restrict__ box, const HbRow* __restrict__ rows, const unsigned* __restrict__ crow,
                                                const unsigned* __restrict__ acc, HbPlan P, HbThr T, unsigned long long* __restrict__ masks,
                                                unsigned* __restrict__ cnt)
{
    const unsigned w = blockIdx.x * (HC_THREADS / WAVE) + mk_uniform(threadIdx.x >> 6);
    if (w >= P.wstart[3]) return;                                    // (the whole wave)
    const unsigned c = (w >= P.wstart[1] ? 1u : 0u) + (w >= P.wstart[2] ? 1u : 0u);
    const unsigned len = hbond_pick(P.len, c), wfirst = c == 0u ? P.wstart[0] : (c == 1u ? P.wstart[1] : P.wstart[2]);
    const unsigned tiles = (len + HB_TILE - 1) / HB_TILE, wl = w - wfirst, g = wl / tiles, t = wl - g * tiles;
    const int lane = threadIdx.x & (WAVE - 1);
    const long long lf = (long long)blockIdx.y * WAVE + lane;
    const size_t f = (size_t)(f0 + (lf < fc ? lf : fc - 1));
    float bx[3];
    ring_box(box, F, (long long)f, bx);
    const unsigned r0 = g * HB_G, left = hbond_pick(P.cnum, c) - r0;             // >= 1
    const int ng = left < (unsigned)HB_G ? (int)left : HB_G;
    HbRow R[HB_G];
    HbDonor<HS> D[HB_G];
    unsigned long long m[HB_G];
    unsigned ri[HB_G];
#pragma unroll
    for (int i = 0; i < HB_G; ++i) {
        ri[i] = crow[hbond_pick(P.coff, c) + r0 + (unsigned)(i < ng ? i : ng - 1)];
        R[i] = rows[ri[i]];
        D[i].load(coords, F, R[i], f, bx);
        m[i] = 0ull;
    }
    const unsigned* __restrict__ a = acc + hbond_pick(P.off, c) + t * HB_TILE;
    const unsigned rest = len - t * HB_TILE;
    const int nq = rest < (unsigned)HB_TILE ? (int)rest : HB_TILE;
#pragma unroll 1
    for (int k = 0; k < nq; ++k) {
        const unsigned atom = a[k];
        float pa[3];
        hbond_atom(coords, F, atom, f, pa);
#pragma unroll
        for (int i = 0; i < HB_G; ++i) {
            const bool hit = atom != R[i].heavy && hbond_pair<HS>(D[i], pa, bx, T);   // "identical donor-acceptor atom"
            m[i] |= (unsigned long long)hit << k;
        }
    }
    if (lf < fc) {
#pragma unroll
        for (int i = 0; i < HB_G; ++i)
            if (i < ng) {
                masks[(size_t)(R[i].tile0 + t) * (size_t)pitch + (size_t)lf] = m[i];
                if (m[i]) mk_atomic_add(&cnt[(size_t)ri[i] * (size_t)pitch + (size_t)lf], (unsigned)mk_popc64(m[i]));
            }
    }
}

// Count, lanes along the acceptors of ONE frame.  A wave: frame lf, one tile (its row: tile_row); the mask is a ballot.
template <bool HS>
MK_KERNEL(HC_THREADS) void k_hbond_count_pairs(const float* __restrict__ coords, long long F, long long f0, long long pitch,
                                               const float* __restrict__ box, const HbRow* __restrict__ rows, const unsigned* __restrict__ tile_row,
                                               long long tiles, const unsigned* __restrict__ acc, HbPlan P, HbThr T,
                                               unsigned long long* __restrict__ masks, unsigned* __restrict__ cnt)
{
    const long long tile = (long long)blockIdx.x * (HC_THREADS / WAVE) + (long long)mk_uniform(threadIdx.x >> 6), lf = (long long)blockIdx.y;
    if (tile >= tiles) return;                                       // (the whole wave)
    const int lane = threadIdx.x & (WAVE - 1);
    const size_t f = (size_t)(f0 + lf);
    float bx[3];
    ring_box(box, F, (long long)f, bx);
    const unsigned row = tile_row[tile];
    const HbRow R = rows[row];
    HbDonor<HS> D;
    D.load(coords, F, R, f, bx);
    const unsigned j = ((unsigned)tile - R.tile0) * HB_TILE + (unsigned)lane, len = hbond_pick(P.len, R.cls);
    const bool valid = j < len;
    const unsigned atom = acc[hbond_pick(P.off, R.cls) + (valid ? j : len - 1)];   // past the end: the last entry (computed, never counted)
    float pa[3];
    hbond_atom(coords, F, atom, f, pa);
    const bool hit = atom != R.heavy && hbond_pair<HS>(D, pa, bx, T);
    const unsigned long long m = mk_ballot(hit && valid);
    if (lane == 0) {
        masks[(size_t)tile * (size_t)pitch + (size_t)lf] = m;
        if (m) mk_atomic_add(&cnt[(size_t)row * (size_t)pitch + (size_t)lf], (unsigned)mk_popc64(m));
    }
}

// ------------------------------------------------------------------------------------------------
// Fill.  A lane owns one (row, frame): its reported pairs go to frame_base[lf] + prefix[row][lf] onwards -- it walks the row's tiles and
// their set bits in ascending order until it has written what the row counted (most rows of most frames counted nothing and leave at
// once).  FRAMES: consecutive lanes are consecutive frames, as in the count kernel that wrote the masks; otherwise consecutive rows.
// `names`: what the list calls an atom -- names[atom] (the host entry's packed rows), the index itself where null; hs == 0: the
// hydrogen's place holds -1.
// ------------------------------------------------------------------------------------------------
constexpr int HF_THREADS = 256;

template <bool FRAMES>
MK_KERNEL(HF_THREADS) void k_hbond_fill(long long pitch, long long fc, const HbRow* __restrict__ rows, long long n_rows,
                                        const unsigned* __restrict__ acc, HbPlan P, const unsigned long long* __restrict__ masks,
                                        const unsigned* __restrict__ prefix, const unsigned long long* __restrict__ totals,
                                        const unsigned long long* __restrict__ frame_base, const unsigned* __restrict__ names, int hs,
                                        int* __restrict__ triples)
{
    const long long row = FRAMES ? (long long)blockIdx.x * (HF_THREADS / WAVE) + (threadIdx.x >> 6) : (long long)blockIdx.x * HF_THREADS + threadIdx.x;
    const long long lf = FRAMES ? (long long)blockIdx.y * WAVE + (threadIdx.x & (WAVE - 1)) : (long long)blockIdx.y;
    if (row >= n_rows || lf >= fc) return;
    const unsigned first = prefix[(size_t)row * (size_t)pitch + (size_t)lf];
    const unsigned next = row + 1 < n_rows ? prefix[(size_t)(row + 1) * (size_t)pitch + (size_t)lf] : (unsigned)totals[lf];
    if (next == first) return;
    unsigned long long pos = frame_base[lf] + first;
    const unsigned long long end = frame_base[lf] + next;
    const HbRow R = rows[row];
    const unsigned len = hbond_pick(P.len, R.cls), tiles = (len + HB_TILE - 1) / HB_TILE;
    const unsigned* __restrict__ a = acc + hbond_pick(P.off, R.cls);
    const int heavy = (int)(names ? names[R.heavy] : R.heavy), hyd = hs ? (int)(names ? names[R.ref] : R.ref) : -1;
    for (unsigned t = 0; t < tiles && pos < end; ++t) {
        unsigned long long m = masks[(size_t)(R.tile0 + t) * (size_t)pitch + (size_t)lf];
        while (m) {
            const int k = mk_ctz64(m);
            m &= m - 1ull;
            const unsigned atom = a[t * HB_TILE + (unsigned)k];
            int* __restrict__ o = triples + 3 * pos;
            o[0] = heavy;
            o[1] = hyd;
            o[2] = (int)(names ? names[atom] : atom);
            ++pos;
        }
    }
}

}  // namespace mkamd
