// wrap_kernels.h -- HIP kernels of the rectangular periodic wrap (moleculekit wrapping/wrapping.pyx::wrap_box, called from
// Molecule.wrap) on MI355X (gfx950): every bonded group of every frame is moved by whole box lengths, axis by axis, back to within
// half a box of the frame's box centre.
//
// Layout: coordinates frame-major float32 [F, N, 3] (the XTC decoder's, the alignment's); box float32 [3, F]; groups are contiguous
// runs of atoms given by their starts uint32 [G + 1] (starts[G] = N); the centre selection uint32 [n_c] in the caller's order.
//
// The arithmetic is the reference's to the bit, every operation rounded on its own (mk_f*_rn; nothing contracted, no reciprocal):
//   centre of a list of atoms   c = 0;  c = c + (x_n - c) / float(n + 1)  for n = 0, 1, ...  in float32: a SERIAL chain -- a centre
//                               that differs in the last bit moves a group on the boundary by a whole box
//   per axis i                  half = box_i / 2;  diff = group_centre_i - box_centre_i;  if (fabs(diff) > half):
//                               translation = float(double(box_i) * round(double(diff / box_i)))   (float32 quotient; C's round, half
//                               away from zero)  and  x_i = x_i - translation  for every atom of the group
// A zero box length, a NaN, an infinity give whatever this arithmetic gives; nothing is special-cased.
//
//   k_wrap_centre   a wave per frame: the running mean of the centre selection in the UNWRAPPED frame -> centre [F, 3].  A launch of
//                   its own, complete before any group of the frame is written (the selection lies inside groups that move).
//   k_wrap_lanes    a lane per (frame, group) for groups of at most `small_max` atoms (waters, ions): the chain from global memory,
//                   then -- only where an axis moves, or out of place -- the atoms again, shifted.  Larger groups are skipped.
//   k_wrap_waves    a wave per (frame, listed group) for the others (lipids, chains): the wave loads WRAP_CHUNK atoms at a time into
//                   LDS coalesced, lanes 0..2 run the three axes' chains out of LDS (the chain is latency: about n dependent float
//                   divisions, which no number of lanes shortens), then the whole wave applies the shift coalesced.
// A group that does not move is not written when the call is in place.  No atomics of any kind: the same bits on every run.
// An index past the arrays never faults: group bounds are clamped to N, a centre index >= N reads as NaN.
#pragma once
#ifndef MK_DEVICE_API_PROVIDED
#include "mk_device.h"
#endif

namespace mkamd {

constexpr int WRAP_BLOCK = 256;          // k_wrap_lanes
constexpr int WRAP_CHUNK = 256;          // atoms per LDS chunk of a wave: 3 KB (a CU's 160 KB hold every wave it can run), 12 floats a lane
constexpr int WRAP_SMALL_MAX = 16;       // groups up to this size take k_wrap_lanes (the default; the pipeline's `avoid` moves it)

// one step of the reference's numerically stable average
MK_DEV float wrap_mean_step(float c, float x, float n_plus_1) { return mk_fadd_rn(c, mk_fdiv_rn(mk_fsub_rn(x, c), n_plus_1)); }

// does the axis move, and by how much
MK_DEV bool wrap_decide(float grp_centre, float box_centre, float box, float& translation)
{
    const float half = mk_fdiv_rn(box, 2.0f);
    const float diff = mk_fsub_rn(grp_centre, box_centre);
    translation = 0.0f;
    if (!(mk_abs(diff) > half)) return false;
    const double r = __builtin_round((double)mk_fdiv_rn(diff, box));
    translation = (float)mk_dmul_rn((double)box, r);
    return true;
}

// The wave's running mean of n atoms of frame P: atom k is idx[k] (GATHER) or first + k.  Lanes 0, 1, 2 return the mean of their axis
// (the other lanes 0).  lds: 3 * WRAP_CHUNK floats of this wave.  Every lane of the wave must call it.
template <bool GATHER>
MK_DEV float wrap_wave_mean(const float* P, const unsigned* __restrict__ idx, long long first, long long n, long long N,
                            float* lds, int lane)
{
    float c = 0.0f;
    for (long long k0 = 0; k0 < n; k0 += WRAP_CHUNK) {
        const int m = (int)(n - k0 < WRAP_CHUNK ? n - k0 : WRAP_CHUNK);
        if constexpr (GATHER) {
            for (int a = lane; a < m; a += WAVE) {
                const unsigned i = idx[k0 + a];
                const bool ok = (long long)i < N;
                const float* p = P + 3 * (size_t)(ok ? i : 0u);
                const float nan = mk_uint_as_float(0x7fc00000u);
                lds[3 * a] = ok ? p[0] : nan;
                lds[3 * a + 1] = ok ? p[1] : nan;
                lds[3 * a + 2] = ok ? p[2] : nan;
            }
        } else {
            const float* p = P + 3 * (size_t)(first + k0);
            for (int t = lane; t < 3 * m; t += WAVE) lds[t] = p[t];
        }
        mk_wave_sync();
        if (lane < 3) {
            // (the divisor is exact while n < 2^24; beyond it it rounds as the reference's int -> float does)
            for (int k = 0; k < m; ++k) c = wrap_mean_step(c, lds[3 * k + lane], (float)(k0 + k + 1));
        }
        mk_wave_sync();
    }
    return c;
}

// centre [F, 3]: the running mean of the atoms sel[0 .. n_c) of every frame.  Grid: F blocks of one wave.
MK_KERNEL(64) void k_wrap_centre(const float* __restrict__ xyz, long long n_atoms, const unsigned* __restrict__ sel, long long n_c,
                                 float* __restrict__ centre)
{
    __shared__ float lds[3 * WRAP_CHUNK];
    const long long f = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const float c = wrap_wave_mean<true>(xyz + (size_t)f * 3 * (size_t)n_atoms, sel, 0, n_c, n_atoms, lds, lane);
    if (lane < 3) centre[3 * f + lane] = c;
}

// the box centre of frame f: the centre kernel's, or the three floats given
MK_DEV float wrap_box_centre(const float* __restrict__ centre, long long f, int axis, float cx, float cy, float cz)
{
    return centre ? centre[3 * f + axis] : axis == 0 ? cx : axis == 1 ? cy : cz;
}

// Item i: frame i / G, group i % G (neighbouring lanes: neighbouring groups of one frame -- their atoms are neighbours in memory).
// out == xyz: in place.
MK_KERNEL(WRAP_BLOCK) void k_wrap_lanes(const float* xyz, long long n_atoms, const float* __restrict__ box, long long F,
                                        const unsigned* __restrict__ starts, long long G, int small_max,
                                        const float* __restrict__ centre, float cx, float cy, float cz, float* out)
{
    const long long item = (long long)blockIdx.x * WRAP_BLOCK + threadIdx.x;
    if (item >= F * G) return;
    const long long f = item / G, g = item - f * G;
    long long b = starts[g], e = starts[g + 1];
    b = b < n_atoms ? b : n_atoms;
    e = e < n_atoms ? e : n_atoms;
    const long long n = e - b;
    if (n <= 0 || n > small_max) return;
    const size_t base = ((size_t)f * (size_t)n_atoms + (size_t)b) * 3;
    const float* p = xyz + base;                                          // (no __restrict__: out may be xyz)
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    for (int k = 0; k < (int)n; ++k) {
        const float d = (float)(k + 1);
        c0 = wrap_mean_step(c0, p[3 * k], d);
        c1 = wrap_mean_step(c1, p[3 * k + 1], d);
        c2 = wrap_mean_step(c2, p[3 * k + 2], d);
    }
    float t0, t1, t2;
    const bool m0 = wrap_decide(c0, wrap_box_centre(centre, f, 0, cx, cy, cz), box[f], t0);
    const bool m1 = wrap_decide(c1, wrap_box_centre(centre, f, 1, cx, cy, cz), box[F + f], t1);
    const bool m2 = wrap_decide(c2, wrap_box_centre(centre, f, 2, cx, cy, cz), box[2 * F + f], t2);
    const bool in_place = out == xyz;
    if (in_place && !(m0 || m1 || m2)) return;
    float* o = out + base;
    for (int k = 0; k < (int)n; ++k) {
        const float x = p[3 * k], y = p[3 * k + 1], z = p[3 * k + 2];
        if (m0 || !in_place) o[3 * k] = m0 ? mk_fsub_rn(x, t0) : x;
        if (m1 || !in_place) o[3 * k + 1] = m1 ? mk_fsub_rn(y, t1) : y;
        if (m2 || !in_place) o[3 * k + 2] = m2 ? mk_fsub_rn(z, t2) : z;
    }
}

// Block i (one wave): frame i / n_list, group list[i % n_list]; groups of at most small_max atoms are k_wrap_lanes' and skipped.
MK_KERNEL(64) void k_wrap_waves(const float* xyz, long long n_atoms, const float* __restrict__ box, long long F,
                                const unsigned* __restrict__ starts, long long G, const unsigned* __restrict__ list, long long n_list,
                                int small_max, const float* __restrict__ centre, float cx, float cy, float cz, float* out)
{
    __shared__ float lds[3 * WRAP_CHUNK];
    const long long i = blockIdx.x;
    const long long f = i / n_list;
    const long long g = list[i - f * n_list];
    const int lane = (int)threadIdx.x;
    if (g >= G) return;                                                   // (wave-uniform, as every return below)
    long long b = starts[g], e = starts[g + 1];
    b = b < n_atoms ? b : n_atoms;
    e = e < n_atoms ? e : n_atoms;
    const long long n = e - b;
    if (n <= small_max) return;
    const float* P = xyz + (size_t)f * 3 * (size_t)n_atoms;
    const float c = wrap_wave_mean<false>(P, nullptr, b, n, n_atoms, lds, lane);
    float t = 0.0f;
    bool m = false;
    if (lane < 3) m = wrap_decide(c, wrap_box_centre(centre, f, lane, cx, cy, cz), box[(long long)lane * F + f], t);
    float tr[3];
    unsigned mv[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        tr[a] = mk_uint_as_float(mk_readlane(mk_float_bits(t), a));
        mv[a] = mk_readlane(m ? 1u : 0u, a);
    }
    const bool in_place = out == xyz;
    if (in_place && !(mv[0] | mv[1] | mv[2])) return;
    const float* p = P + 3 * (size_t)b;
    float* o = out + (size_t)f * 3 * (size_t)n_atoms + 3 * (size_t)b;
    int axis = lane % 3;                                                  // of float t = lane + 64 j: (lane + j) % 3, as 64 % 3 == 1
    for (long long k = lane; k < 3 * n; k += WAVE) {
        const float x = p[k];
        const float ta = axis == 0 ? tr[0] : axis == 1 ? tr[1] : tr[2];
        const unsigned ma = axis == 0 ? mv[0] : axis == 1 ? mv[1] : mv[2];
        o[k] = ma ? mk_fsub_rn(x, ta) : x;
        axis = axis == 2 ? 0 : axis + 1;
    }
}

}  // namespace mkamd
