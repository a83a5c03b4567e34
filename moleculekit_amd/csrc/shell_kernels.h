// shell_kernels.h -- HIP kernels of MetricShell (moleculekit projections/metricshell.py) on MI355X (gfx950): how many atoms of a second
// selection lie in each of S concentric shells around every atom of a first one, per frame -- WITHOUT the [frames, n1 * n2] distance
// matrix the reference histograms on the host.
//
// A pair is in shell s iff e_s < d <= e_(s+1), d = fl32(sqrt(d2)) the reference's float32 distance.  The correctly rounded root is
// monotone, so d <= e is the same as d2 <= T(e), T(e) the largest float32 whose rounded root is still <= e (the host finds it:
// moleculekit_amd/shell.py shell_thresholds): the kernels take no root at all.  They keep, per (frame, centre), the S + 1 running
// counts of d2 <= T_s and leave their differences: integers, so the sums do not depend on the order and every run gives the same.
// d2 itself is dist_kernels.h' dist2_min_image_f32 -- the bits of every other kernel of the row.  A NaN passes no test.
//
// Two lane assignments, as in the rest of the row:
//   k_shell_frames   lanes along FRAMES (the coordinates' fast axis: every load coalesced), C centres per lane in registers, the
//                    second atoms wave-uniform;
//   k_shell_atoms    lanes along the SECOND atoms of one frame (one structure, a handful of frames), the centre wave-uniform, a
//                    count is the population of a ballot.
#pragma once
#include "dist_kernels.h"

namespace mkamd {

constexpr int SH_MAX_SHELLS = 32, SH_MAX_EDGES = SH_MAX_SHELLS + 1;
struct ShellEdges { float t[SH_MAX_EDGES]; };        // thresholds on d2, by value: kernel arguments live in scalar registers
                                                     // (entries past the call's edges: -1, which no d2 is below)

MK_DEV float shell_coord(const float* __restrict__ coords, long long F, unsigned atom, int ax, long long f)
{
    return coords[((size_t)atom * 3 + (size_t)ax) * (size_t)F + (size_t)f];
}

// counts[f, i, s] += (running count s + 1) - (running count s), zeros left alone (the call has cleared the array)
template <int NE>
MK_DEV void shell_add(const unsigned (&cnt)[NE], int S, int* __restrict__ counts, long long n1, long long f, long long i)
{
    unsigned* __restrict__ o = reinterpret_cast<unsigned*>(counts) + ((size_t)f * (size_t)n1 + (size_t)i) * (size_t)S;
#pragma unroll
    for (int s = 0; s < NE - 1; ++s) {
        const unsigned v = cnt[s + 1] - cnt[s];
        if (s < S && v != 0u) mk_atomic_add(o + s, v);
    }
}

// ------------------------------------------------------------------------------------------------
// Lanes along frames.  A wave: 64 frames x C consecutive centres x one slice of the second selection.  The slice's atom indices and
// chain ids come in 64 at a time (lane k holds atom k, handed out with readlane: the rows they name are wave-uniform bases), the
// coordinates of SHF_BATCH second atoms are requested together, and each is used for the C centres in registers: 3 loads per C pairs.
// Per pair: the 8 operations of d2 (27 more where it wraps) and a compare and an add-with-carry per edge.
// ------------------------------------------------------------------------------------------------
constexpr int SHF_THREADS = 256, SHF_BATCH = 4;

template <bool PBC, int NE, int C>
MK_KERNEL(SHF_THREADS) void k_shell_frames(const float* __restrict__ coords, long long F, const float* __restrict__ box,
                                           const unsigned* __restrict__ sel1, long long n1, const unsigned* __restrict__ sel2, long long n2,
                                           const unsigned* __restrict__ chains, int symmetric, ShellEdges T, int S, long long splits,
                                           long long per_split, int* __restrict__ counts)
{
    const long long groups = (n1 + C - 1) / C, tasks = ((F + WAVE - 1) / WAVE) * groups * splits;
    const long long task = (long long)blockIdx.x * (SHF_THREADS / WAVE) + (long long)mk_uniform(threadIdx.x >> 6);
    if (task >= tasks) return;                                       // (the whole wave)
    const int lane = threadIdx.x & (WAVE - 1);
    // waves of a block: neighbouring groups of centres over the SAME frames and slice -- they read the same rows
    const long long g = task % groups, sp = (task / groups) % splits, slab = task / (groups * splits);
    const bool live = slab * WAVE + lane < F;
    const long long f = live ? slab * WAVE + lane : F - 1;          // frames past the end compute on the last one (never added)
    const long long i0 = g * C;
    const int nc = n1 - i0 < C ? (int)(n1 - i0) : C;                // wave-uniform, >= 1
    float A[C][3];
    unsigned ca[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const unsigned a = sel1[c < nc ? i0 + c : i0];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) A[c][ax] = shell_coord(coords, F, a, ax, f);
        ca[c] = PBC ? chains[a] : 0u;
    }
    float bx = 0.f, by = 0.f, bz = 0.f, ibx = 0.f, iby = 0.f, ibz = 0.f;
    if (PBC) {
        bx = box[0 * F + f]; by = box[1 * F + f]; bz = box[2 * F + f];
        ibx = mk_fdiv_rn(1.f, bx); iby = mk_fdiv_rn(1.f, by); ibz = mk_fdiv_rn(1.f, bz);
    }
    unsigned cnt[C][NE];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int e = 0; e < NE; ++e) cnt[c][e] = 0u;
    const long long jb = sp * per_split, je = jb + per_split < n2 ? jb + per_split : n2;       // (jb < n2: the host's splits)
    for (long long j0 = jb; j0 < je; j0 += WAVE) {
        const int m = je - j0 < WAVE ? (int)(je - j0) : WAVE;       // wave-uniform, >= 1
        const unsigned vb = sel2[j0 + (lane < m ? lane : m - 1)], vc = PBC ? chains[vb] : 0u;
#pragma unroll 1
        for (int k0 = 0; k0 < m; k0 += SHF_BATCH) {
            unsigned cb[SHF_BATCH];
            float B[SHF_BATCH][3];
#pragma unroll
            for (int u = 0; u < SHF_BATCH; ++u) {
                const int k = k0 + u < m ? k0 + u : m - 1;          // past the slice: its last atom again (loaded, not counted)
                const unsigned b = mk_readlane(vb, k);
                cb[u] = mk_readlane(vc, k);
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) B[u][ax] = shell_coord(coords, F, b, ax, f);
            }
#pragma unroll
            for (int u = 0; u < SHF_BATCH; ++u) {
                if (k0 + u >= m) break;                              // wave-uniform
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    // (wave-uniform conditions: centres past the end; the pair (i, i) of a selection against itself; the image shift)
                    if (c >= nc || (symmetric && j0 + k0 + u == i0 + c)) continue;
                    const float d2 = dist2_min_image_f32(A[c][0], A[c][1], A[c][2], B[u][0], B[u][1], B[u][2], bx, by, bz, ibx, iby, ibz,
                                                         PBC && ca[c] != cb[u]);
#pragma unroll
                    for (int e = 0; e < NE; ++e) cnt[c][e] += d2 <= T.t[e] ? 1u : 0u;
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (c < nc) shell_add(cnt[c], S, counts, n1, f, i0 + c);
    }
}

// ------------------------------------------------------------------------------------------------
// Lanes along the second atoms of ONE frame.  A wave: frame f, SHA_CI consecutive centres, 64 * JPL second atoms kept in registers
// (gathered once: 12 bytes per atom and frame); a centre's coordinates are wave-uniform loads.  A running count is the population of
// the ballot of d2 <= T_s -- scalar arithmetic --, and lane 0 adds a centre's S differences to the result: the slices of the second
// selection meet in integer atomics.
// ------------------------------------------------------------------------------------------------
constexpr int SHA_THREADS = 256, SHA_CI = 16;

template <bool PBC, int NE, int JPL>
MK_KERNEL(SHA_THREADS) void k_shell_atoms(const float* __restrict__ coords, long long F, const float* __restrict__ box,
                                          const unsigned* __restrict__ sel1, long long n1, const unsigned* __restrict__ sel2, long long n2,
                                          const unsigned* __restrict__ chains, int symmetric, ShellEdges T, int S, int* __restrict__ counts)
{
    const long long NJ = (n2 + WAVE * JPL - 1) / (WAVE * JPL), NI = (n1 + SHA_CI - 1) / SHA_CI, tasks = F * NI * NJ;
    const long long task = (long long)blockIdx.x * (SHA_THREADS / WAVE) + (long long)mk_uniform(threadIdx.x >> 6);
    if (task >= tasks) return;                                       // (the whole wave)
    const int lane = threadIdx.x & (WAVE - 1);
    const long long jblk = task % NJ, ic = (task / NJ) % NI, f = task / (NJ * NI);
    float B[JPL][3];
    unsigned cb[JPL];
    long long jk[JPL];
#pragma unroll
    for (int k = 0; k < JPL; ++k) {
        jk[k] = jblk * WAVE * JPL + WAVE * k + lane;
        const unsigned b = sel2[jk[k] < n2 ? jk[k] : n2 - 1];       // past the end: the last atom (computed, never counted)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) B[k][ax] = shell_coord(coords, F, b, ax, f);
        cb[k] = PBC ? chains[b] : 0u;
    }
    float bx = 0.f, by = 0.f, bz = 0.f, ibx = 0.f, iby = 0.f, ibz = 0.f;
    if (PBC) {
        bx = box[0 * F + f]; by = box[1 * F + f]; bz = box[2 * F + f];
        ibx = mk_fdiv_rn(1.f, bx); iby = mk_fdiv_rn(1.f, by); ibz = mk_fdiv_rn(1.f, bz);
    }
    const long long i_end = ic * SHA_CI + SHA_CI < n1 ? ic * SHA_CI + SHA_CI : n1;
    for (long long i = ic * SHA_CI; i < i_end; ++i) {
        const unsigned a = sel1[i], ca = PBC ? chains[a] : 0u;
        const float xa = shell_coord(coords, F, a, 0, f), ya = shell_coord(coords, F, a, 1, f), za = shell_coord(coords, F, a, 2, f);
        unsigned cnt[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) cnt[e] = 0u;
#pragma unroll
        for (int k = 0; k < JPL; ++k) {
            const float d2 = dist2_min_image_f32(xa, ya, za, B[k][0], B[k][1], B[k][2], bx, by, bz, ibx, iby, ibz, PBC && cb[k] != ca);
            const bool counted = jk[k] < n2 && !(symmetric && jk[k] == i);
#pragma unroll
            for (int e = 0; e < NE; ++e) cnt[e] += (unsigned)mk_popc64(mk_ballot(counted && d2 <= T.t[e]));
        }
        if (lane == 0) shell_add(cnt, S, counts, n1, f, i);
    }
}

}  // namespace mkamd
