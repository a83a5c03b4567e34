// tests/emu/emu_moments.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the group-moment kernels (moleculekit_amd/csrc/moments_kernels.h) through their launch plans (moments_pipeline.h) on the host
// SIMT emulation of emu_device.h: the product's kernel source, host memory instead of HBM.  Built into
// tests/emu/libmkamd_emu_moments.so by tests/emu_moments_build.py (-ffp-contract=off).
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/moments_pipeline.h"

#include <cstdlib>
#include <cstring>
#include <string>

using namespace mkamd;

namespace {

struct MomentsEmuBackend {
    void* bufs[WS_NSLOTS] = {};
    size_t caps[WS_NSLOTS] = {};
    size_t workspace = 0;                  // bytes of workspace the plan asked for (the tests bound it)
    std::string kernel;
    int cus = 256;
    int compute_units() const { return cus; }
    ~MomentsEmuBackend() { for (void* p : bufs) free(p); }
    void note_dist_kernel(const char* name) { kernel = name; }
    int ensure(int slot, size_t bytes, void** ptr, int = 0)
    {
        if (bytes == 0) bytes = 16;
        if (caps[slot] < bytes) {
            free(bufs[slot]);
            bufs[slot] = malloc(bytes);
            memset(bufs[slot], 0xCD, bytes);          // poison: catch reads of unwritten workspace
            workspace += bytes - caps[slot];
            caps[slot] = bytes;
        }
        *ptr = bufs[slot];
        return 0;
    }
    template <class... KA, class... A>
    int launch(void (*kernel)(KA...), dim3 grid, dim3 block, A... args)
    {
        emu::launch(kernel, grid, block, args...);
        return 0;
    }
};

thread_local std::string g_err, g_kernel;
thread_local long long g_workspace = 0;

MomArgs args(const float* xyz, long long N, long long F, const double* affine, const unsigned* atoms, const unsigned* offsets,
             const float* weights, long long G, long long n_sel)
{
    MomArgs a;
    a.xyz = xyz; a.n_atoms = N; a.n_frames = F; a.affine = affine;
    a.atoms = atoms; a.offsets = offsets; a.weights = weights;
    a.n_groups = G; a.n_sel = n_sel;
    a.max_group = 1;
    for (long long g = 0; offsets && g < G; ++g) a.max_group = std::max(a.max_group, (long long)offsets[g + 1] - (long long)offsets[g]);
    return a;
}

}  // namespace

extern "C" {

const char* emu_moments_last_error() { return g_err.c_str(); }
const char* emu_moments_last_kernel() { return g_kernel.c_str(); }
long long emu_moments_last_workspace() { return g_workspace; }

// xyz [F, N, 3]; cus: the compute-unit count the launch plan assumes
int emu_group_moments(int cus, const float* xyz, long long N, long long F, const double* affine, const unsigned* atoms, const unsigned* offsets,
                      const float* weights, long long G, long long n_sel, int mode, float* out, int avoid)
{
    MomentsEmuBackend be;
    be.cus = cus;
    g_err.clear();
    const int st = run_group_moments(be, args(xyz, N, F, affine, atoms, offsets, weights, G, n_sel), mode, out, g_err, avoid);
    g_kernel = be.kernel;
    g_workspace = (long long)be.workspace;
    return st;
}

int emu_fluctuation(int cus, const float* xyz, long long N, long long F, const double* affine, const unsigned* atoms, long long n_sel,
                    const unsigned* offsets, long long G, const double* ref, double* out, int avoid)
{
    MomentsEmuBackend be;
    be.cus = cus;
    g_err.clear();
    const int st = run_fluctuation(be, args(xyz, N, F, affine, atoms, offsets, nullptr, offsets ? G : 0, n_sel), ref, out, g_err, avoid);
    g_kernel = be.kernel;
    g_workspace = (long long)be.workspace;
    return st;
}

int emu_moments_plan(long long n_mean, long long n_max, long long n_items, int cus, int avoid, int* out4)
{
    const MomPlan p = moments_plan(n_mean, n_max, n_items, cus, avoid);
    out4[0] = p.glog2; out4[1] = p.segs; out4[2] = p.seg_len; out4[3] = (int)p.blocks_x;
    return 0;
}

}  // extern "C"
