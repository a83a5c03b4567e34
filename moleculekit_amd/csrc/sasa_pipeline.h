// sasa_pipeline.h -- launch sequence of the surface-area kernels (sasa_kernels.h), written against the backend concept of
// pipeline.h so that the product (capi.hip) and the test emulator (tests/emu/emu_sasa.cpp) run the same plan.
#pragma once
#include "sasa_kernels.h"
#include "pipeline.h"

#include <cmath>
#include <string>
#include <vector>

namespace mkamd {

// The n unit-sphere points of the reference (mdtraj's generate_sphere_points: a golden-section spiral), float32 [n][3].  The C
// expression there mixes float variables and double literals; this is that expression conversion by conversion (DESIGN.md
// section 9 records that this variant reproduces the reference's held areas point for point):
//   float inc = pi (3 - sqrt 5), offset = 2.0 / n;  y = i * offset - 1.0 + (offset / 2.0);  r = sqrt(1.0 - y * y);  phi = i * inc;
//   point = (cos(phi) * r, y, sin(phi) * r)
inline void sasa_sphere_points(int n, std::vector<float>& out)
{
    out.resize((size_t)3 * (size_t)(n > 0 ? n : 0));
    const double pi = 3.14159265358979323846;
    const float inc = (float)(pi * (3.0 - std::sqrt(5.0)));
    const float offset = (float)(2.0 / (double)n);
    for (int i = 0; i < n; ++i) {
        const float io = (float)i * offset;
        const float y = (float)((double)io - 1.0 + (double)offset / 2.0);
        const float yy = y * y;
        const float r = (float)std::sqrt(1.0 - (double)yy);
        const float phi = (float)i * inc;
        out[3 * (size_t)i] = (float)(std::cos((double)phi) * (double)r);
        out[3 * (size_t)i + 1] = y;
        out[3 * (size_t)i + 2] = (float)(std::sin((double)phi) * (double)r);
    }
}

inline float sasa_area_const(int n_points) { return (float)(4.0 * 3.14159265358979323846 / (double)n_points); }

struct SasaArgs {
    const float* xyz = nullptr;          // [F, N, 3]
    long long n_atoms = 0, n_frames = 0;
    const float* radii = nullptr;        // [N], probe included, in the unit of xyz / coord_div
    int n_points = 0;
    const int* mapping = nullptr;        // [N] column of out each atom adds to: inside [0, n_out), non-decreasing
    const int* mask = nullptr;           // [N] non-zero: the atom's area is computed (every atom shields)
    long long n_out = 0;
    float coord_div = 1.0f;              // coordinates are divided by this first (10: Angstrom in, the reference's nanometres inside)
    float* out = nullptr;                // [F, n_out], filled by the caller; areas are added
};

inline const char* sasa_check(const SasaArgs& a)
{
    if (a.n_atoms < 0 || a.n_frames < 0 || a.n_out < 0) return "negative size";
    if (a.n_points < 1) return "n_points must be at least 1";
    if (a.n_points > (1 << 24)) return "more than 2^24 sphere points (the count is carried in float32)";
    if (a.n_atoms > 0x3fffffffLL) return "more than 2^30 - 1 atoms";
    if (!(a.coord_div > 0.0f)) return "coord_div must be positive";
    if (a.n_atoms > 0 && a.n_out < 1) return "n_out must be at least 1";
    if (a.n_atoms > 0 && a.n_frames > (0x7fffffffLL * SA_BLOCK) / a.n_atoms) return "too many frames x atoms for one call";
    return nullptr;
}

inline const char* sasa_error_text(int flags)
{
    if (flags & SA_ERR_MAP_RANGE) return "atom_mapping has a value outside [0, n_out)";
    if (flags & SA_ERR_MAP_ORDER) return "atom_mapping must be non-decreasing (the atoms of an output column contiguous)";
    if (flags & SA_ERR_COINCIDENT) return "two atoms are virtually on top of one another (r^2 < 1e-10): the surface is not defined";
    return "";
}

// out[f, mapping[i]] += area of atom i in frame f, for every selected atom.  Ends with a read of the refusal flags (it waits
// for the stream): on a refusal nothing has been added to `out`.
template <class BE>
int run_sasa(BE& be, const SasaArgs& a, std::string& err)
{
    if (const char* e = sasa_check(a)) { err = e; return ST_EINVAL; }
    if (a.n_atoms == 0 || a.n_frames == 0) return ST_OK;
    const long long N = a.n_atoms, F = a.n_frames;
    int st;
    void *dpts = nullptr, *dpack = nullptr, *darea = nullptr, *derr = nullptr;
    std::vector<float> pts;
    sasa_sphere_points(a.n_points, pts);
    // frames per launch of the count kernel: a workgroup per (frame, atom), at most 2^30 of them and 2^24 packed atoms (256 MB)
    const long long chunk = std::max(1LL, std::min(F, (1LL << 24) / N));
    if ((st = be.ensure(WS_S_POINTS, pts.size() * sizeof(float), &dpts, 0))) return st;
    if ((st = be.ensure(WS_S_PACK, (size_t)chunk * N * sizeof(float4), &dpack, 0))) return st;
    if ((st = be.ensure(WS_S_AREA, (size_t)F * N * sizeof(float), &darea, 0))) return st;
    if ((st = be.ensure(WS_S_ERR, sizeof(int), &derr, 0))) return st;
    if ((st = be.to_device(dpts, pts.data(), pts.size() * sizeof(float)))) return st;
    if ((st = be.fill(derr, 0, sizeof(int)))) return st;
    const float area_const = sasa_area_const(a.n_points);
    for (long long f0 = 0; f0 < F; f0 += chunk) {
        const long long nf = std::min(chunk, F - f0), items = nf * N;
        if ((st = be.launch(k_sasa_pack, dim3((unsigned)((items + SA_BLOCK - 1) / SA_BLOCK)), dim3(SA_BLOCK), a.xyz + 3 * f0 * N, a.radii, N,
                            items, a.coord_div, a.mapping, a.n_out, (int)(f0 == 0), (float4*)dpack, (int*)derr)))
            return st;
        if ((st = be.launch(k_sasa_count, dim3((unsigned)items), dim3(SA_BLOCK), (const float4*)dpack, (int)N, a.mask, (const float*)dpts,
                            a.n_points, area_const, (float*)darea + f0 * N, (int*)derr)))
            return st;
    }
    const long long items = F * N;
    if ((st = be.launch(k_sasa_scatter, dim3((unsigned)((items + SA_BLOCK - 1) / SA_BLOCK)), dim3(SA_BLOCK), (const float*)darea, N, items,
                        a.mapping, a.mask, a.n_out, a.out, (const int*)derr)))
        return st;
    int flags = 0;
    if ((st = be.to_host(&flags, derr, sizeof(int)))) return st;        // (waits: `pts` is read by the copy until here)
    if (flags) { err = sasa_error_text(flags); return ST_EINVAL; }
    return ST_OK;
}

}  // namespace mkamd
