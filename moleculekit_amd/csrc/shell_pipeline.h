// shell_pipeline.h -- launch plan of the shell-count kernels (shell_kernels.h), written against the backend concept of pipeline.h so
// that the product (capi.hip) and the test emulator (tests/emu/emu_shell.cpp) run the same plan.
#pragma once
#include "shell_kernels.h"
#include "pipeline.h"

#include <algorithm>
#include <string>
#include <type_traits>

namespace mkamd {

enum { SHELL_AVOID_FRAMES = 1, SHELL_AVOID_ATOMS = 2 };   // `avoid`: the tests walk both lane assignments over the same shapes

// second atoms per lane of k_shell_atoms: four where that keeps >= 80 % of the lanes on real atoms, else one
inline int shell_atoms_jpl(long long n2) { return (double)n2 / (double)((n2 + 255) / 256 * 256) >= 0.8 ? 4 : 1; }

// Lanes along the second atoms instead of the frames?  Only calls of fewer than 64 frames leave lanes of the frame kernel idle; they
// go to the atom kernel when that fills its lanes better.
inline bool shell_takes_atoms(long long F, long long n2)
{
    if (F >= WAVE) return false;
    const long long w = (long long)WAVE * shell_atoms_jpl(n2);
    return (double)n2 / (double)((n2 + w - 1) / w * w) > (double)F / (double)WAVE;
}

// counts int32 [F, n1, n_edges - 1] (cleared here) = how many atoms j of sel2 have T[s] < d2(i, j) <= T[s + 1], per frame and centre i
// of sel1; `d2_thresholds` is HOST memory (it travels as a kernel argument), everything else the device's.  symmetric: sel1 and sel2
// are the same list and the pair (i, i) does not count.  No workspace: nothing here is proportional to n1 * n2.
template <class BE>
int run_shell_counts(BE& be, const float* coords, long long F, const float* box, const unsigned* sel1, long long n1, const unsigned* sel2,
                     long long n2, const unsigned* chains, int symmetric, int pbc, const float* d2_thresholds, long long n_edges,
                     int* counts, std::string& err, int avoid = 0)
{
    if (F < 0 || n1 < 0 || n2 < 0) { err = "negative size"; return ST_EINVAL; }
    if (n_edges < 2 || n_edges > SH_MAX_EDGES) { err = "numshells must be between 1 and 32 (n_edges between 2 and 33)"; return ST_EINVAL; }
    if (!d2_thresholds) { err = "NULL pointer"; return ST_EINVAL; }
    if (symmetric && n1 != n2) { err = "symmetric: both selections must be the same list"; return ST_EINVAL; }
    if (F > 0x3fffffffLL) { err = "too many frames (>= 2^30)"; return ST_EINVAL; }
    ShellEdges T;
    for (int e = 0; e < SH_MAX_EDGES; ++e) T.t[e] = -1.0f;
    for (long long e = 0; e < n_edges; ++e) {
        // (the shells are differences of running counts: the thresholds must not decrease -- and a NaN compares false both ways)
        if (!(d2_thresholds[e] >= (e ? d2_thresholds[e - 1] : d2_thresholds[0]))) { err = "d2_thresholds must be non-decreasing numbers"; return ST_EINVAL; }
        T.t[e] = d2_thresholds[e];
    }
    const int S = (int)n_edges - 1;
    if (F == 0 || n1 == 0) return ST_OK;
    if ((double)F * (double)n1 * (double)S >= 4.0e18) { err = "result too large"; return ST_EINVAL; }
    int st;
    if ((st = be.fill(counts, 0, (size_t)F * (size_t)n1 * (size_t)S * sizeof(int)))) return st;
    if (n2 == 0) return ST_OK;
    const int ne = n_edges <= 5 ? 5 : n_edges <= 9 ? 9 : n_edges <= 17 ? 17 : 33;       // edges the kernel is compiled for
    const bool atoms = (avoid & SHELL_AVOID_FRAMES) || (!(avoid & SHELL_AVOID_ATOMS) && shell_takes_atoms(F, n2));
    if (atoms) {
        const int jpl = shell_atoms_jpl(n2);
        const long long tasks = F * ((n1 + SHA_CI - 1) / SHA_CI) * ((n2 + WAVE * jpl - 1) / (WAVE * jpl));
        if (tasks / 4 + 1 > 0x7ffffff0LL) { err = "too many (frame, centre, atom) blocks for one call; split the frames"; return ST_EINVAL; }
        const dim3 grid((unsigned)((tasks + 3) / 4)), block(SHA_THREADS);
        be.note_dist_kernel(pbc ? "mkamd::k_shell_atoms<true>" : "mkamd::k_shell_atoms<false>");
        auto go = [&](auto kern) { return be.launch(kern, grid, block, coords, F, box, sel1, n1, sel2, n2, chains, symmetric, T, S, counts); };
        auto by_jpl = [&](auto pbc_, auto ne_) {
            constexpr bool P = decltype(pbc_)::value;
            constexpr int E = decltype(ne_)::value;
            return jpl == 4 ? go(k_shell_atoms<P, E, 4>) : go(k_shell_atoms<P, E, 1>);
        };
        auto by_ne = [&](auto pbc_) {
            return ne == 5 ? by_jpl(pbc_, std::integral_constant<int, 5>{}) : ne == 9 ? by_jpl(pbc_, std::integral_constant<int, 9>{})
                 : ne == 17 ? by_jpl(pbc_, std::integral_constant<int, 17>{}) : by_jpl(pbc_, std::integral_constant<int, 33>{});
        };
        return pbc ? by_ne(DistFlag<true>{}) : by_ne(DistFlag<false>{});
    }
    // centres per lane: what the running counts leave room for in the registers (C * NE counters)
    const int C = ne == 5 ? 4 : ne == 9 ? 2 : 1;
    const long long base = ((F + WAVE - 1) / WAVE) * ((n1 + C - 1) / C);
    // slices of the second selection, of at least 64 atoms, until ~4 waves per SIMD exist (256 CUs x 4 SIMDs)
    long long splits = (4 * 4 * (long long)std::max(1, be.compute_units()) + base - 1) / base;
    splits = std::max<long long>(1, std::min<long long>(splits, (n2 + WAVE - 1) / WAVE));
    const long long per_split = ((n2 + splits - 1) / splits + WAVE - 1) / WAVE * WAVE;
    splits = (n2 + per_split - 1) / per_split;                       // (every slice starts inside the selection)
    const long long tasks = base * splits;
    if (tasks / 4 + 1 > 0x7ffffff0LL) { err = "too many (frame, centre) blocks for one call; split the frames"; return ST_EINVAL; }
    const dim3 grid((unsigned)((tasks + 3) / 4)), block(SHF_THREADS);
    be.note_dist_kernel(pbc ? "mkamd::k_shell_frames<true>" : "mkamd::k_shell_frames<false>");
    auto go = [&](auto kern) {
        return be.launch(kern, grid, block, coords, F, box, sel1, n1, sel2, n2, chains, symmetric, T, S, splits, per_split, counts);
    };
    if (pbc) return ne == 5 ? go(k_shell_frames<true, 5, 4>) : ne == 9 ? go(k_shell_frames<true, 9, 2>) : ne == 17 ? go(k_shell_frames<true, 17, 1>)
                                                                                                                 : go(k_shell_frames<true, 33, 1>);
    return ne == 5 ? go(k_shell_frames<false, 5, 4>) : ne == 9 ? go(k_shell_frames<false, 9, 2>) : ne == 17 ? go(k_shell_frames<false, 17, 1>)
                                                                                                             : go(k_shell_frames<false, 33, 1>);
}

}  // namespace mkamd
