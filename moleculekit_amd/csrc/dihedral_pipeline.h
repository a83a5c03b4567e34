// dihedral_pipeline.h -- launch plan of the dihedral kernels (dihedral_kernels.h), written against the backend concept of pipeline.h so
// that the product (capi.hip) and the test emulator (tests/emu/emu_dihedral.cpp) run the same plan.
#pragma once
#include "dihedral_kernels.h"
#include "pipeline.h"

#include <string>
#include <type_traits>

namespace mkamd {

enum { DIH_AVOID_FRAMES = 1, DIH_AVOID_ATOMS = 2 };       // `avoid`: the tests walk both lane assignments over the same shapes

// Lanes along the dihedrals instead of the frames?  Calls of fewer than 64 frames leave lanes of the frame kernel idle.
inline bool dihedral_takes_atoms(long long F) { return F < WAVE; }

// out float32, frame-major: [F, D, 2] (mode DIH_TERMS), [F, D] (DIH_RADIANS, DIH_DEGREES), [F, 2 D] (DIH_SINCOS); coords [N, 3, F],
// quads uint32 [D, 4] (every index < N: the caller's check), box [3, F] or NULL -- all the device's.  wrap: the box is given and not
// all zeros (the reference's condition; the caller decides it where the box lives).  No workspace: nothing but the result is
// proportional to F * D.
template <class BE>
int run_dihedrals(BE& be, const float* coords, long long F, const float* box, int wrap, const unsigned* quads, long long D, int mode,
                  float* out, std::string& err, int avoid = 0)
{
    if (F < 0 || D < 0) { err = "negative size"; return ST_EINVAL; }
    if (mode < DIH_TERMS || mode > DIH_SINCOS) { err = "mode must be 0 (terms), 1 (radians), 2 (degrees) or 3 (sincos)"; return ST_EINVAL; }
    if (F > 0x3fffffffLL) { err = "too many frames (>= 2^30)"; return ST_EINVAL; }
    if (D > 0x3fffffffLL) { err = "too many dihedrals (>= 2^30)"; return ST_EINVAL; }
    if (F == 0 || D == 0) return ST_OK;
    if ((double)F * (double)D * (double)dih_width(mode) >= 1.0e18) { err = "result too large"; return ST_EINVAL; }
    if (!coords || !quads || !out || (wrap && !box)) { err = "NULL pointer"; return ST_EINVAL; }
    const bool atoms = (avoid & DIH_AVOID_FRAMES) || (!(avoid & DIH_AVOID_ATOMS) && dihedral_takes_atoms(F));
    const long long tasks = atoms ? F * ((D + WAVE - 1) / WAVE) : ((F + WAVE - 1) / WAVE) * ((D + DHF_D - 1) / DHF_D);
    if (tasks / 4 + 1 > 0x7ffffff0LL) { err = "too many (frame, dihedral) blocks for one call; split the frames"; return ST_EINVAL; }
    const dim3 grid((unsigned)((tasks + 3) / 4)), block(atoms ? DHA_THREADS : DHF_THREADS);
    if (atoms) be.note_dist_kernel(wrap ? "mkamd::k_dihedral_atoms<true>" : "mkamd::k_dihedral_atoms<false>");
    else be.note_dist_kernel(wrap ? "mkamd::k_dihedral_frames<true>" : "mkamd::k_dihedral_frames<false>");
    auto go = [&](auto kern) { return be.launch(kern, grid, block, coords, F, box, quads, D, out); };
    auto by_mode = [&](auto wrap_, auto mode_) {
        constexpr bool Wr = decltype(wrap_)::value;
        constexpr int M = decltype(mode_)::value;
        return atoms ? go(k_dihedral_atoms<Wr, M>) : go(k_dihedral_frames<Wr, M>);
    };
    auto by_wrap = [&](auto wrap_) {
        return mode == DIH_TERMS ? by_mode(wrap_, std::integral_constant<int, DIH_TERMS>{})
             : mode == DIH_RADIANS ? by_mode(wrap_, std::integral_constant<int, DIH_RADIANS>{})
             : mode == DIH_DEGREES ? by_mode(wrap_, std::integral_constant<int, DIH_DEGREES>{})
                                   : by_mode(wrap_, std::integral_constant<int, DIH_SINCOS>{});
    };
    return wrap ? by_wrap(DistFlag<true>{}) : by_wrap(DistFlag<false>{});
}

}  // namespace mkamd
