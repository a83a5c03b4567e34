// align_pipeline.h -- launch sequences of the alignment kernels (align_kernels.h), written against the backend concept of
// pipeline.h so that the product (capi.hip) and the test emulator (tests/emu/emu_align.cpp) run the same plans.
#pragma once
#include "align_kernels.h"
#include "pipeline.h"

#include <cstdio>
#include <string>

namespace mkamd {

// How k_align_sums covers `n_items` frames x `n` selected atoms: G = 2^glog2 lanes per frame (the smallest power of two >= n,
// 8..64: up to 8 frames per wave), and the selection cut into `segs` segments when there are too few frames to fill the chip
// (about 8 waves per CU), each segment at least 4 atoms per lane.
struct AlignPlan {
    int glog2 = 3;
    int segs = 1;
    int seg_len = 1;
    unsigned blocks_x = 1;
};

inline AlignPlan align_plan(long long n, long long n_items, int cus)
{
    AlignPlan p;
    while (p.glog2 < 6 && (1LL << p.glog2) < n) ++p.glog2;
    const long long G = 1LL << p.glog2;
    const long long per_wave = WAVE / G;
    const long long waves = (n_items + per_wave - 1) / per_wave;
    const long long want = 8LL * (cus > 0 ? cus : 256);
    const long long max_segs = std::max(1LL, (n + 4 * G - 1) / (4 * G));
    long long segs = std::min(max_segs, std::max(1LL, (want + waves - 1) / std::max(1LL, waves)));
    segs = std::min(segs, 4096LL);
    long long seg_len = std::max(1LL, (n + segs - 1) / segs);
    seg_len = (seg_len + G - 1) / G * G;
    segs = std::max(1LL, (n + seg_len - 1) / seg_len);
    p.segs = (int)segs;
    p.seg_len = (int)seg_len;
    p.blocks_x = (unsigned)((n_items + (AL_BLOCK / G) - 1) / (AL_BLOCK / G));
    return p;
}

// What a call launched for its frames, for mkamd_ctx_last_dist_kernel: the k_align_sums instantiation, the lane-group width, and the
// fold exactly when the frames' records were cut into segments (the reference's own pass of AL_SINGLE is not named).  A backend that
// keeps no note (it has no note_dist_kernel) runs the same plans without one.
template <class BE>
auto align_note_to(BE& be, const char* name, int) -> decltype(be.note_dist_kernel(name), void()) { be.note_dist_kernel(name); }
template <class BE>
void align_note_to(BE&, const char*, long) {}

template <class BE>
void align_note(BE& be, const char* mode, const AlignPlan& p, const char* fold)
{
    static_assert(AL_SHP == 17 && AL_NS == 24, "the fold's name below spells these out");
    char name[96];
    snprintf(name, sizeof name, "mkamd::k_align_sums<%s> G=%d segs=%d%s%s", mode, 1 << p.glog2, p.segs, p.segs > 1 ? " + mkamd::" : "",
             p.segs > 1 ? fold : "");
    align_note_to(be, name, 0);
}

struct AlignArgs {
    const float* xyz = nullptr;          // [F, N, 3]
    long long n_atoms = 0, n_frames = 0;
    const float* ref = nullptr;          // [Fr, Nr, 3]
    long long n_ref_atoms = 0, n_ref_frames = 0;
    const unsigned* sel = nullptr;       // [n] atoms of a frame
    const unsigned* refsel = nullptr;    // [n] atoms of the reference
    long long n = 0;
    const long long* frames = nullptr;   // [n_list] (nullptr: 0 .. n_list - 1)
    long long n_list = 0;
    long long refframe = 0;
    bool matching = false;               // reference frame = the frame itself
};

inline const char* align_check(const AlignArgs& a)
{
    if (a.n_atoms < 0 || a.n_frames < 0 || a.n_ref_atoms < 0 || a.n_ref_frames < 0 || a.n < 0 || a.n_list < 0) return "negative size";
    if (a.n_list > 0x7fffffffLL || a.n > 0x7fffffffLL) return "more than 2^31 - 1 frames or selected atoms";
    if (a.matching && a.n_ref_frames != a.n_frames) return "matchingframes needs a reference with as many frames as the trajectory";
    if (!a.matching && a.n_list > 0 && (a.refframe < 0 || a.refframe >= a.n_ref_frames)) return "refframe out of range";
    if (!a.frames && a.n_list > a.n_frames) return "n_list > n_frames without a list of frames";
    return nullptr;
}

// affine [n_list, 12] and fit_rmsd [n_list] (nullable) of every listed frame: the sums, the solve (+ the reference's sums when it is one
// frame; + a fold of the segments where the selection was split)
template <class BE>
int run_align_transforms(BE& be, const AlignArgs& a, double* affine, double* fit_rmsd, std::string& err)
{
    if (const char* e = align_check(a)) { err = e; return ST_EINVAL; }
    if (a.n_list == 0) return ST_OK;
    const long long ff = 3 * a.n_atoms, rff = 3 * a.n_ref_atoms;
    int st;
    const double* refpart = nullptr;
    int ref_segs = 0;
    if (!a.matching) {                               // the reference's centroid and spread: once
        const AlignPlan rp = align_plan(a.n, 1, be.compute_units());
        void* w = nullptr;
        if ((st = be.ensure(WS_A_REFPART, (size_t)rp.segs * AL_NS * sizeof(double), &w, 0))) return st;
        if ((st = be.launch(k_align_sums<AL_REF>, dim3(rp.blocks_x, (unsigned)rp.segs), dim3(AL_BLOCK), a.xyz, ff, a.ref, rff, a.sel,
                            a.refsel, (int)a.n, a.frames, 1, a.refframe, rp.glog2, rp.seg_len, (const double*)nullptr, (double*)w)))
            return st;
        refpart = (const double*)w;
        ref_segs = rp.segs;
        if (ref_segs > 1) {                          // (a lane per frame would walk them one after the other)
            void* f = nullptr;
            if ((st = be.ensure(WS_A_REFFOLD, AL_NS * sizeof(double), &f, 0))) return st;
            if ((st = be.launch(k_align_fold<AL_SHP, AL_NS>, dim3(1), dim3(WAVE), refpart, ref_segs, (double*)f))) return st;
            refpart = (const double*)f;
            ref_segs = 1;
        }
    }
    const AlignPlan p = align_plan(a.n, a.n_list, be.compute_units());
    align_note(be, a.matching ? "AL_MATCH" : "AL_SINGLE", p, "k_align_fold<17, 24>");
    void* w = nullptr;
    if ((st = be.ensure(WS_A_PART, (size_t)a.n_list * p.segs * AL_NS * sizeof(double), &w, 0))) return st;
    const dim3 grid(p.blocks_x, (unsigned)p.segs);
    const unsigned solve_blocks = (unsigned)((a.n_list + 63) / 64);
    if ((st = a.matching ? be.launch(k_align_sums<AL_MATCH>, grid, dim3(AL_BLOCK), a.xyz, ff, a.ref, rff, a.sel, a.refsel, (int)a.n,
                                     a.frames, (int)a.n_list, a.refframe, p.glog2, p.seg_len, (const double*)nullptr, (double*)w)
                         : be.launch(k_align_sums<AL_SINGLE>, grid, dim3(AL_BLOCK), a.xyz, ff, a.ref, rff, a.sel, a.refsel, (int)a.n,
                                     a.frames, (int)a.n_list, a.refframe, p.glog2, p.seg_len, (const double*)nullptr, (double*)w)))
        return st;
    const double* part = (const double*)w;
    int segs = p.segs;
    if (segs > 1) {
        void* f = nullptr;
        if ((st = be.ensure(WS_A_FOLD, (size_t)a.n_list * AL_NS * sizeof(double), &f, 0))) return st;
        if ((st = be.launch(k_align_fold<AL_SHP, AL_NS>, dim3((unsigned)a.n_list), dim3(WAVE), part, segs, (double*)f))) return st;
        part = (const double*)f;
        segs = 1;
    }
    if (a.matching)
        return be.launch(k_align_solve<AL_MATCH>, dim3(solve_blocks), dim3(WAVE), part, segs, refpart, ref_segs, (int)a.n, (int)a.n_list,
                         affine, fit_rmsd);
    return be.launch(k_align_solve<AL_SINGLE>, dim3(solve_blocks), dim3(WAVE), part, segs, refpart, ref_segs, (int)a.n, (int)a.n_list,
                     affine, fit_rmsd);
}

// out[frames[i]] = float32(M_i x + t_i) for every atom of each listed frame (out may be xyz)
template <class BE>
int run_align_apply(BE& be, const float* xyz, long long n_atoms, const long long* frames, long long n_list, const double* affine,
                    float* out, std::string& err)
{
    if (n_atoms < 0 || n_list < 0) { err = "negative size"; return ST_EINVAL; }
    if (n_atoms == 0 || n_list == 0) return ST_OK;
    const long long segs = (n_atoms + AL_APPLY_ATOMS - 1) / AL_APPLY_ATOMS;
    if (segs * n_list > 0x7fffffffLL) { err = "too many frames x atoms for one call (> 2^31 blocks of 1 024 atoms)"; return ST_EINVAL; }
    return be.launch(k_align_apply, dim3((unsigned)(segs * n_list)), dim3(AL_BLOCK), xyz, 3 * n_atoms, frames, (int)segs, affine, out);
}

// rmsd [n_list] float32: sqrt(mean |float32(M p + t) - q|^2) over (sel, refsel) -- util.molRMSD after the alignment, no copy of the
// coordinates.
template <class BE>
int run_align_rmsd(BE& be, const AlignArgs& a, const double* affine, float* rmsd, std::string& err)
{
    if (const char* e = align_check(a)) { err = e; return ST_EINVAL; }
    if (a.n_list == 0) return ST_OK;
    if (!affine) { err = "NULL affine"; return ST_EINVAL; }
    int st;
    const AlignPlan p = align_plan(a.n, a.n_list, be.compute_units());
    align_note(be, "AL_RMSD", p, "k_align_fold<1, 1>");
    void* w = nullptr;
    if ((st = be.ensure(WS_A_RPART, (size_t)a.n_list * p.segs * sizeof(double), &w, 0))) return st;
    if ((st = be.launch(k_align_sums<AL_RMSD>, dim3(p.blocks_x, (unsigned)p.segs), dim3(AL_BLOCK), a.xyz, 3 * a.n_atoms, a.ref,
                        3 * a.n_ref_atoms, a.sel, a.refsel, (int)a.n, a.frames, (int)a.n_list, a.matching ? -1LL : a.refframe, p.glog2,
                        p.seg_len, affine, (double*)w)))
        return st;
    const double* part = (const double*)w;
    int segs = p.segs;
    if (segs > 1) {
        void* f = nullptr;
        if ((st = be.ensure(WS_A_FOLD, (size_t)a.n_list * sizeof(double), &f, 0))) return st;
        if ((st = be.launch(k_align_fold<1, 1>, dim3((unsigned)a.n_list), dim3(WAVE), part, segs, (double*)f))) return st;
        part = (const double*)f;
        segs = 1;
    }
    return be.launch(k_align_rmsd_finish, dim3((unsigned)((a.n_list + 63) / 64)), dim3(WAVE), part, segs, (int)a.n, (int)a.n_list, rmsd);
}

}  // namespace mkamd
