// moments_pipeline.h -- launch plans of the group-moment kernels (moments_kernels.h), written against the backend concept of pipeline.h
// so that the product (capi.hip) and the test emulator (tests/emu/emu_moments.cpp) run the same plans.
#pragma once
#include "moments_kernels.h"
#include "pipeline.h"

#include <algorithm>
#include <cstdio>
#include <string>
#include <type_traits>

namespace mkamd {

// `avoid`: the tests walk both forms over the same shapes.  OWNED: a lane group owns the whole (frame, group) and finishes it in the
// same launch; SEGMENTED: the group's atoms are cut into segments over many waves and k_mom_fold finishes.
enum { MOM_AVOID_OWNED = 1, MOM_AVOID_SEGMENTED = 2 };

// How k_mom_sums covers n_items (frame, group) pairs: L = 2^glog2 lanes per item from the MEAN group size (the smallest power of two
// >= it, 8..64: residues share a wave), and -- when the items alone cannot fill the chip (about 8 waves per CU) -- the LARGEST group
// cut into `segs` segments of seg_len atoms, each at least 4 atoms per lane (align_plan's rule).
struct MomPlan {
    int glog2 = 3;
    int segs = 1;
    int seg_len = 1;
    unsigned blocks_x = 1;
};

inline MomPlan moments_plan(long long n_mean, long long n_max, long long n_items, int cus, int avoid)
{
    MomPlan p;
    while (p.glog2 < 6 && (1LL << p.glog2) < n_mean) ++p.glog2;
    const long long L = 1LL << p.glog2, per_wave = WAVE / L;
    const long long waves = (n_items + per_wave - 1) / per_wave;
    const long long want = 8LL * (cus > 0 ? cus : 256);
    const long long max_segs = std::max(1LL, (n_max + 4 * L - 1) / (4 * L));
    long long segs = std::min(max_segs, std::max(1LL, (want + waves - 1) / std::max(1LL, waves)));
    segs = std::min(segs, 4096LL);
    if (avoid & MOM_AVOID_SEGMENTED) segs = 1;
    else if ((avoid & MOM_AVOID_OWNED) && segs == 1) segs = std::min(std::max(1LL, (n_max + L - 1) / L), 2LL);   // (two where a group allows it)
    long long seg_len = std::max(1LL, (n_max + segs - 1) / segs);
    seg_len = (seg_len + L - 1) / L * L;
    segs = std::max(1LL, (n_max + seg_len - 1) / seg_len);
    p.segs = (int)segs;
    p.seg_len = (int)seg_len;
    p.blocks_x = (unsigned)((n_items + (MOM_BLOCK / L) - 1) / (MOM_BLOCK / L));
    return p;
}

struct MomArgs {
    const float* xyz = nullptr;          // [F, N, 3]
    long long n_atoms = 0, n_frames = 0;
    const double* affine = nullptr;      // [F, 12] or NULL
    const unsigned* atoms = nullptr;     // [n_sel]
    const unsigned* offsets = nullptr;   // [G + 1]
    const float* weights = nullptr;      // [n_sel] or NULL
    long long n_groups = 0, n_sel = 0;
    long long max_group = 0;             // the largest group's size (the plan's; an understated value costs balance, not atoms)
};

inline const char* moments_check(const MomArgs& a)
{
    if (a.n_atoms < 0 || a.n_frames < 0 || a.n_groups < 0 || a.n_sel < 0 || a.max_group < 0) return "negative size";
    if (a.n_frames > 0x3fffffffLL) return "too many frames (>= 2^30)";
    // (n_sel < 2^30: seg_len, a group's size rounded up to a multiple of 64 lanes, then fits the kernels' int)
    if (a.n_groups > 0x3fffffffLL || a.n_sel > 0x3fffffffLL) return "too many groups or group atoms (>= 2^30)";
    return nullptr;
}

template <int MODE, class BE>
int run_moments_mode(BE& be, const MomArgs& a, const double* ref, void* out, std::string& err, int avoid, const char* first = "")
{
    const long long n_items = MODE == MOM_SPHERICAL ? a.n_frames : a.n_frames * a.n_groups;
    const long long n_max = MODE == MOM_SPHERICAL ? a.n_sel : std::max(1LL, a.max_group);
    const long long n_mean = MODE == MOM_SPHERICAL ? a.n_sel : (a.n_sel + a.n_groups - 1) / a.n_groups;
    const MomPlan p = moments_plan(n_mean, n_max, n_items, be.compute_units(), avoid);
    if ((long long)p.blocks_x < 1 || n_items / (MOM_BLOCK >> p.glog2) + 1 > 0x7ffffff0LL) { err = "too many (frame, group) pairs for one call; split the frames"; return ST_EINVAL; }
    const bool seg = p.segs > 1 || (avoid & MOM_AVOID_OWNED);
    char name[96];
    if (seg) snprintf(name, sizeof name, "%smkamd::k_mom_sums<%d, true> + mkamd::k_mom_fold<%d>", first, MODE, MODE);
    else snprintf(name, sizeof name, "%smkamd::k_mom_sums<%d, false>", first, MODE);
    be.note_dist_kernel(name);
    const long long ff = 3 * a.n_atoms;
    if (!seg)
        return be.launch(k_mom_sums<MODE, false>, dim3(p.blocks_x), dim3(MOM_BLOCK), a.xyz, ff, a.affine, a.atoms, a.offsets, a.weights, ref,
                         a.n_groups, n_items, p.glog2, p.seg_len, out, (double*)nullptr);
    if (n_items > 0x7fffffffLL) { err = "too many (frame, group) pairs for the segmented form; split the frames"; return ST_EINVAL; }
    void* w = nullptr;
    int st;
    if ((st = be.ensure(WS_M_PART, (size_t)n_items * p.segs * mom_rec(MODE) * sizeof(double), &w, 0))) return st;
    if ((st = be.launch(k_mom_sums<MODE, true>, dim3(p.blocks_x, (unsigned)p.segs), dim3(MOM_BLOCK), a.xyz, ff, a.affine, a.atoms, a.offsets,
                        a.weights, ref, a.n_groups, n_items, p.glog2, p.seg_len, (void*)nullptr, (double*)w)))
        return st;
    return be.launch(k_mom_fold<MODE>, dim3((unsigned)n_items), dim3(WAVE), (const double*)w, p.segs, a.offsets, a.n_groups, out);
}

// out: float32 [F, 3 G] (MOM_CENTER), [F, G, 4] (MOM_GYRATION), [F, 3] (MOM_SPHERICAL: n_groups == 2, no weights) -- the device's, as
// every pointer of `a`.  No group may be empty (the caller's check where the offsets live).  Workspace: the segment records only.
template <class BE>
int run_group_moments(BE& be, const MomArgs& a, int mode, float* out, std::string& err, int avoid = 0)
{
    if (const char* e = moments_check(a)) { err = e; return ST_EINVAL; }
    if (mode < MOM_CENTER || mode > MOM_SPHERICAL) { err = "mode must be 0 (center), 1 (gyration) or 2 (spherical)"; return ST_EINVAL; }
    if (mode == MOM_SPHERICAL && (a.n_groups != 2 || a.weights)) { err = "the spherical mode takes exactly two unweighted groups (target, reference)"; return ST_EINVAL; }
    if (a.n_frames == 0 || a.n_groups == 0) return ST_OK;
    if (a.n_sel < a.n_groups) { err = "an empty group"; return ST_EINVAL; }
    if (!a.xyz || !a.atoms || !a.offsets || !out) { err = "NULL pointer"; return ST_EINVAL; }
    return mode == MOM_CENTER ? run_moments_mode<MOM_CENTER>(be, a, nullptr, out, err, avoid)
         : mode == MOM_GYRATION ? run_moments_mode<MOM_GYRATION>(be, a, nullptr, out, err, avoid)
                                : run_moments_mode<MOM_SPHERICAL>(be, a, nullptr, out, err, avoid);
}

// out float64 [F, n_sel] (a.offsets == NULL: per atom) or [F, G] (the mean over each group's atoms) of sum_c (x_c - ref_c)^2;
// ref float64 [n_sel, 3] on the device, or NULL: the per-atom mean over all frames (k_mom_mean, into the workspace first).
template <class BE>
int run_fluctuation(BE& be, const MomArgs& a, const double* ref, double* out, std::string& err, int avoid = 0)
{
    if (const char* e = moments_check(a)) { err = e; return ST_EINVAL; }
    if (a.weights) { err = "the fluctuation takes no weights"; return ST_EINVAL; }
    if (a.n_frames == 0 || a.n_sel == 0 || (a.offsets && a.n_groups == 0)) return ST_OK;
    if (a.offsets && a.n_sel < a.n_groups) { err = "an empty group"; return ST_EINVAL; }
    if (!a.xyz || !a.atoms || !out) { err = "NULL pointer"; return ST_EINVAL; }
    const long long ff = 3 * a.n_atoms;
    int st;
    const char* first = "";
    if (!ref) {
        int glog2 = 3;
        while (glog2 < 6 && (1LL << glog2) < a.n_frames) ++glog2;
        void* w = nullptr;
        if ((st = be.ensure(WS_M_REF, (size_t)a.n_sel * 3 * sizeof(double), &w, 0))) return st;
        const long long per = MOM_BLOCK >> glog2;
        if ((st = be.launch(k_mom_mean, dim3((unsigned)((a.n_sel + per - 1) / per)), dim3(MOM_BLOCK), a.xyz, ff, a.n_frames, a.affine, a.atoms,
                            a.n_sel, glog2, (double*)w)))
            return st;
        ref = (const double*)w;
        first = "mkamd::k_mom_mean + ";
    }
    if (a.offsets) return run_moments_mode<MOM_FLUCT>(be, a, ref, out, err, avoid, first);
    const long long n_items = a.n_frames * a.n_sel;
    if (n_items / MOM_BLOCK + 1 > 0x7ffffff0LL) { err = "too many (frame, atom) pairs for one call; split the frames"; return ST_EINVAL; }
    be.note_dist_kernel((std::string(first) + "mkamd::k_mom_fluct_atoms").c_str());
    return be.launch(k_mom_fluct_atoms, dim3((unsigned)((n_items + MOM_BLOCK - 1) / MOM_BLOCK)), dim3(MOM_BLOCK), a.xyz, ff, a.affine, a.atoms,
                     ref, a.n_sel, n_items, out);
}

}  // namespace mkamd
