// wrap_cell_pipeline.h -- launch plan of the triclinic periodic-wrap kernels (wrap_cell_kernels.h), written against the backend concept
// of pipeline.h so that the product (capi.hip) and the test emulator (tests/emu/emu_wrap_cell.cpp) run the same plan.
//
// The plan: [k_wrap_centre] -> k_wrap_cell_prep -> k_wrap_cell_lanes<MODE> -> [k_wrap_cell_waves<MODE>], in stream order.  The centre
// kernel (wrap_kernels.h's, as it is) is a launch of its own because, in place, a frame's centre must be complete before any group of
// that frame is written; a group reads only its own atoms, so in place (out == xyz) is safe.  The group kernels share the groups by size
// as in wrap_pipeline.h, steered by the same `avoid` bits.  The plan checks sizes and pointers, not the box vectors: a frame whose box
// the reference's loops would not end on is flagged by the prep kernel, copied through and reported in `status` (callers that hold the
// box vectors on the host check them first: wrap_cell_check_boxvectors).
#pragma once
#include "wrap_cell_kernels.h"
#include "wrap_pipeline.h"

namespace mkamd {

struct WrapCellArgs {
    WrapArgs w;                          // everything of the rectangular wrap but `box`, which stays NULL
    const double* boxvectors = nullptr;  // [3, 3, F]
    int mode = WRAP_CELL_RECTANGULAR;    // WRAP_CELL_RECTANGULAR / _COMPACT / _TRICLINIC
    int* status = nullptr;               // [WRAP_CELL_NSTATUS] or NULL; the kernels only ever store 1: the caller clears it
};

template <class BE, int MODE>
int run_wrap_cell_groups(BE& be, const WrapCellArgs& c, const WrapCellFrame* recs, const float* centre, long long small_max, long long lane_blocks,
                         std::string& name)
{
    const WrapArgs& a = c.w;
    int st;
    if (small_max > 0) {
        if ((st = be.launch(k_wrap_cell_lanes<MODE>, dim3((unsigned)lane_blocks), dim3(WRAP_BLOCK), a.xyz, a.n_atoms, recs, a.n_frames, a.starts,
                            a.n_groups, (int)small_max, centre, a.center[0], a.center[1], a.center[2], a.out, c.status)))
            return st;
        name += " + mkamd::k_wrap_cell_lanes";
    }
    if (a.n_large > 0) {
        if ((st = be.launch(k_wrap_cell_waves<MODE>, dim3((unsigned)(a.n_frames * a.n_large)), dim3(WAVE), a.xyz, a.n_atoms, recs, a.n_frames,
                            a.starts, a.n_groups, a.large, a.n_large, (int)small_max, centre, a.center[0], a.center[1], a.center[2], a.out,
                            c.status)))
            return st;
        name += " + mkamd::k_wrap_cell_waves";
    }
    return ST_OK;
}

// Everything of `c` but `w.center` is the device's.  Workspace: the frames' centres (12 B a frame) and records (sizeof(WrapCellFrame)).
template <class BE>
int run_wrap_cell(BE& be, const WrapCellArgs& c, std::string& err, int avoid = 0)
{
    const WrapArgs& a = c.w;
    if (c.mode != WRAP_CELL_RECTANGULAR && c.mode != WRAP_CELL_COMPACT && c.mode != WRAP_CELL_TRICLINIC) { err = "mode must be 0 (rectangular), 1 (compact) or 2 (triclinic)"; return ST_EINVAL; }
    if (a.n_atoms < 0 || a.n_frames < 0 || a.n_groups < 0 || a.n_large < 0 || a.n_centersel < 0) { err = "negative size"; return ST_EINVAL; }
    if (a.n_atoms > 0x3fffffffLL || a.n_frames > 0x3fffffffLL) { err = "too many atoms or frames (>= 2^30)"; return ST_EINVAL; }
    if (a.n_groups > a.n_atoms || a.n_large > a.n_groups) { err = "more groups than atoms (or more listed groups than groups)"; return ST_EINVAL; }
    if ((avoid & WRAP_AVOID_LANES) && (avoid & WRAP_AVOID_WAVES)) { err = "both group kernels avoided"; return ST_EINVAL; }
    if (a.n_frames == 0 || a.n_atoms == 0 || a.n_groups == 0) return ST_OK;
    if (!a.xyz || !c.boxvectors || !a.starts || !a.out || (a.n_large > 0 && !a.large) || (a.n_centersel > 0 && !a.centersel)) { err = "NULL pointer"; return ST_EINVAL; }
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
    void* rw = nullptr;
    if ((st = be.ensure(WS_W_CELL, (size_t)a.n_frames * sizeof(WrapCellFrame), &rw, 0))) return st;
    if ((st = be.launch(k_wrap_cell_prep, dim3((unsigned)((a.n_frames + WAVE - 1) / WAVE)), dim3(WAVE), c.boxvectors, a.n_frames, c.mode,
                        (WrapCellFrame*)rw, c.status)))
        return st;
    name += "mkamd::k_wrap_cell_prep";
    const WrapCellFrame* recs = (const WrapCellFrame*)rw;
    st = c.mode == WRAP_CELL_RECTANGULAR ? run_wrap_cell_groups<BE, WRAP_CELL_RECTANGULAR>(be, c, recs, centre, small_max, lane_blocks, name)
         : c.mode == WRAP_CELL_COMPACT   ? run_wrap_cell_groups<BE, WRAP_CELL_COMPACT>(be, c, recs, centre, small_max, lane_blocks, name)
                                         : run_wrap_cell_groups<BE, WRAP_CELL_TRICLINIC>(be, c, recs, centre, small_max, lane_blocks, name);
    if (st) return st;
    be.note_dist_kernel(name.c_str());
    return ST_OK;
}

// What a caller that holds the box vectors [3, 3, F] on the host checks before anything is launched -- the prep kernel's test; NULL: fine
inline const char* wrap_cell_check_boxvectors(const double* bv, long long F)
{
    if (F < 0) return "negative size";
    if (F == 0) return nullptr;
    if (!bv) return "NULL pointer";
    for (long long f = 0; f < F; ++f) {
        double b[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) b[i][j] = bv[(long long)(3 * i + j) * F + f];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                if (!std::isfinite(b[i][j])) return "box vectors: a component is not finite";
        if (!(b[1][1] > 0.0) || !(b[2][2] > 0.0)) return "box vectors: box[1][1] and box[2][2] must be positive";
        if (b[0][1] != 0.0 || b[0][2] != 0.0 || b[1][2] != 0.0) return "box vectors: not lower triangular (box[0][1], box[0][2], box[1][2] must be 0)";
    }
    return nullptr;
}

// the error a set status word stands for; NULL: none set
inline const char* wrap_cell_status_error(const int* status)
{
    if (status[WRAP_CELL_ST_VECTORS]) return "Too many triclinic vectors!!";
    if (status[WRAP_CELL_ST_FRAME]) return "wrap: a frame's box vectors are degenerate (non-finite, box[1][1] or box[2][2] not positive, or not lower triangular); the frame was copied through unchanged";
    if (status[WRAP_CELL_ST_CAP]) return "wrap: a group did not come into the cell within 4096 steps (an infinite coordinate, or a box length far below the coordinates); it was written with what was reached";
    return nullptr;
}

}  // namespace mkamd
