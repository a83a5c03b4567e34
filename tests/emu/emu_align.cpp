// tests/emu/emu_align.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the alignment kernels (moleculekit_amd/csrc/align_kernels.h) through their launch plans (align_pipeline.h) on the host
// SIMT emulation of emu_device.h: the product's kernel source, host memory instead of HBM.  Built into
// tests/emu/libmkamd_emu_align.so by tests/emu_align_build.py.
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/align_pipeline.h"

#include <cstdlib>
#include <cstring>
#include <string>

using namespace mkamd;

namespace {

struct AlignEmuBackend {
    void* bufs[WS_NSLOTS] = {};
    size_t caps[WS_NSLOTS] = {};
    int compute_units() const { return cus; }
    int cus = 256;
    std::string kernel;
    void note_dist_kernel(const char* name) { kernel = name; }
    ~AlignEmuBackend() { for (void* p : bufs) free(p); }
    int ensure(int slot, size_t bytes, void** ptr, int = 0)
    {
        if (bytes == 0) bytes = 16;
        if (caps[slot] < bytes) {
            free(bufs[slot]);
            bufs[slot] = malloc(bytes);
            memset(bufs[slot], 0xCD, bytes);          // poison: catch reads of unwritten workspace
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

AlignArgs args(const float* xyz, long long N, long long F, const float* ref, long long Nr, long long Fr, const unsigned* sel,
               const unsigned* refsel, long long n, const long long* frames, long long K, long long refframe, int matching)
{
    AlignArgs a;
    a.xyz = xyz; a.n_atoms = N; a.n_frames = F;
    a.ref = ref; a.n_ref_atoms = Nr; a.n_ref_frames = Fr;
    a.sel = sel; a.refsel = refsel; a.n = n;
    a.frames = frames; a.n_list = K;
    a.refframe = refframe; a.matching = matching != 0;
    return a;
}

}  // namespace

extern "C" {

const char* emu_align_last_error() { return g_err.c_str(); }

// run_align_transforms' / run_align_rmsd's note of the last call (what mkamd_ctx_last_dist_kernel reports on the device)
const char* emu_align_last_kernel() { return g_kernel.c_str(); }

// cus: the compute-unit count the launch plan assumes (segments of the selection: few frames are split over many waves)
int emu_align_transforms(int cus, const float* xyz, long long N, long long F, const float* ref, long long Nr, long long Fr,
                         const unsigned* sel, const unsigned* refsel, long long n, const long long* frames, long long K,
                         long long refframe, int matching, double* affine, double* fit_rmsd)
{
    AlignEmuBackend be;
    be.cus = cus;
    g_err.clear();
    const int st = run_align_transforms(be, args(xyz, N, F, ref, Nr, Fr, sel, refsel, n, frames, K, refframe, matching), affine, fit_rmsd, g_err);
    g_kernel = be.kernel;
    return st;
}

int emu_align_apply(const float* xyz, long long N, const long long* frames, long long K, const double* affine, float* out)
{
    AlignEmuBackend be;
    g_err.clear();
    return run_align_apply(be, xyz, N, frames, K, affine, out, g_err);
}

int emu_align_rmsd(int cus, const float* xyz, long long N, long long F, const float* ref, long long Nr, long long Fr, const unsigned* sel,
                   const unsigned* refsel, long long n, const long long* frames, long long K, long long refframe, int matching,
                   const double* affine, float* rmsd)
{
    AlignEmuBackend be;
    be.cus = cus;
    g_err.clear();
    const int st = run_align_rmsd(be, args(xyz, N, F, ref, Nr, Fr, sel, refsel, n, frames, K, refframe, matching), affine, rmsd, g_err);
    g_kernel = be.kernel;
    return st;
}

int emu_align_plan(long long n, long long n_items, int cus, int* out4)
{
    const AlignPlan p = align_plan(n, n_items, cus);
    out4[0] = p.glog2; out4[1] = p.segs; out4[2] = p.seg_len; out4[3] = (int)p.blocks_x;
    return 0;
}

}  // extern "C"
