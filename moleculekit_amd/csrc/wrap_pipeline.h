// wrap_pipeline.h -- launch plan of the periodic-wrap kernels (wrap_kernels.h), written against the backend concept of pipeline.h so
// that the product (capi.hip) and the test emulator (tests/emu/emu_wrap.cpp) run the same plan.
//
// The plan: [k_wrap_centre] -> k_wrap_lanes -> [k_wrap_waves], three launches in stream order.  The centre kernel is a launch of its
// own because, in place, a frame's box centre must be complete before any group of that frame is written.  The two group kernels
// share the groups by size: at most `small_max` atoms a lane, more a wave (the caller lists those groups: they are few).
#pragma once
#include "wrap_kernels.h"
#include "pipeline.h"

#include <string>

namespace mkamd {

// `avoid`: the tests walk both group kernels over the same shapes.  LANES: every group takes the wave kernel (small_max = 0, so the
// caller lists them all); WAVES: every group takes the lane kernel, whatever its size (nothing is listed).
enum { WRAP_AVOID_LANES = 1, WRAP_AVOID_WAVES = 2 };

inline long long wrap_small_max(int avoid)
{
    return (avoid & WRAP_AVOID_LANES) ? 0LL : (avoid & WRAP_AVOID_WAVES) ? 0x7fffffffLL : (long long)WRAP_SMALL_MAX;
}

struct WrapArgs {
    const float* xyz = nullptr;          // [F, N, 3]
    long long n_atoms = 0, n_frames = 0;
    const float* box = nullptr;          // [3, F]
    const unsigned* starts = nullptr;    // [G + 1], starts[0] = 0, increasing, starts[G] = N
    long long n_groups = 0;
    const unsigned* large = nullptr;     // [n_large]: the groups of more than wrap_small_max(avoid) atoms (a group listed that is not one is skipped)
    long long n_large = 0;
    const unsigned* centersel = nullptr; // [n_centersel] (in order), or none: `center`
    long long n_centersel = 0;
    float center[3] = {0.0f, 0.0f, 0.0f};
    float* out = nullptr;                // [F, N, 3]; == xyz: in place
};

// Everything of `a` but `center` is the device's.  Workspace: the frames' centres, 12 B a frame.
template <class BE>
int run_wrap_box(BE& be, const WrapArgs& a, std::string& err, int avoid = 0)
{
    if (a.n_atoms < 0 || a.n_frames < 0 || a.n_groups < 0 || a.n_large < 0 || a.n_centersel < 0) { err = "negative size"; return ST_EINVAL; }
    if (a.n_atoms > 0x3fffffffLL || a.n_frames > 0x3fffffffLL) { err = "too many atoms or frames (>= 2^30)"; return ST_EINVAL; }
    if (a.n_groups > a.n_atoms || a.n_large > a.n_groups) { err = "more groups than atoms (or more listed groups than groups)"; return ST_EINVAL; }
    if ((avoid & WRAP_AVOID_LANES) && (avoid & WRAP_AVOID_WAVES)) { err = "both group kernels avoided"; return ST_EINVAL; }
    if (a.n_frames == 0 || a.n_atoms == 0 || a.n_groups == 0) return ST_OK;
    if (!a.xyz || !a.box || !a.starts || !a.out || (a.n_large > 0 && !a.large) || (a.n_centersel > 0 && !a.centersel)) { err = "NULL pointer"; return ST_EINVAL; }
    const long long small_max = wrap_small_max(avoid);
    const long long lane_blocks = (a.n_frames * a.n_groups + WRAP_BLOCK - 1) / WRAP_BLOCK;
    if (lane_blocks > 0x7ffffff0LL || a.n_frames * a.n_large > 0x7ffffff0LL) { err = "too many (frame, group) pairs for one call; split the frames"; return ST_EINVAL; }
    int st;
    const float* centre = nullptr;
    std::string name;
    if (a.n_centersel > 0) {
        void* w = nullptr;
        if ((st = be.ensure(WS_W_CENTRE, (size_t)a.n_frames * 3 * sizeof(float), &w, 0))) return st;
        if ((st = be.launch(k_wrap_centre, dim3((unsigned)a.n_frames), dim3(WAVE), a.xyz, a.n_atoms, a.centersel, a.n_centersel, (float*)w))) return st;
        centre = (const float*)w;
        name = "mkamd::k_wrap_centre + ";
    }
    if (small_max > 0) {
        if ((st = be.launch(k_wrap_lanes, dim3((unsigned)lane_blocks), dim3(WRAP_BLOCK), a.xyz, a.n_atoms, a.box, a.n_frames, a.starts, a.n_groups,
                            (int)small_max, centre, a.center[0], a.center[1], a.center[2], a.out)))
            return st;
        name += "mkamd::k_wrap_lanes";
    }
    if (a.n_large > 0) {
        if ((st = be.launch(k_wrap_waves, dim3((unsigned)(a.n_frames * a.n_large)), dim3(WAVE), a.xyz, a.n_atoms, a.box, a.n_frames, a.starts,
                            a.n_groups, a.large, a.n_large, (int)small_max, centre, a.center[0], a.center[1], a.center[2], a.out)))
            return st;
        name += small_max > 0 ? " + mkamd::k_wrap_waves" : "mkamd::k_wrap_waves";
    }
    be.note_dist_kernel(name.c_str());
    return ST_OK;
}

// What a caller that holds the starts on the host checks before anything is launched; NULL: fine
inline const char* wrap_check_starts(const unsigned* starts, long long G, long long N)
{
    if (G < 0 || N < 0) return "negative size";
    if (G == 0) return N == 0 ? nullptr : "no groups for the atoms";
    if (!starts) return "NULL pointer";
    if (starts[0] != 0) return "group starts must begin at 0";
    for (long long g = 0; g < G; ++g)
        if (starts[g + 1] <= starts[g]) return "group starts must increase (no empty group)";
    if ((long long)starts[G] != N) return "the last group start must be the number of atoms";
    return nullptr;
}

}  // namespace mkamd
