// tests/emu/emu_wrap_cell.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the triclinic periodic-wrap kernels (moleculekit_amd/csrc/wrap_cell_kernels.h) through their launch plan
// (wrap_cell_pipeline.h) on the host SIMT emulation of emu_device.h: the product's kernel source, host memory instead of HBM.  Built
// into tests/emu/libmkamd_emu_wrap_cell.so by tests/emu_wrap_cell_build.py (-ffp-contract=off).
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/wrap_cell_pipeline.h"

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace mkamd;

namespace {

struct WrapCellEmuBackend {
    void* bufs[WS_NSLOTS] = {};
    size_t caps[WS_NSLOTS] = {};
    std::string kernel;
    int compute_units() const { return 256; }
    ~WrapCellEmuBackend() { for (void* p : bufs) free(p); }
    void note_dist_kernel(const char* name) { kernel = name; }
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

}  // namespace

extern "C" {

const char* emu_wrap_cell_last_error() { return g_err.c_str(); }
const char* emu_wrap_cell_last_kernel() { return g_kernel.c_str(); }
int emu_wrap_cell_max_steps() { return WRAP_CELL_MAX_STEPS; }
const char* emu_wrap_cell_check_boxvectors(const double* bv, long long F) { return wrap_cell_check_boxvectors(bv, F); }
const char* emu_wrap_cell_status_error(const int* status) { return wrap_cell_status_error(status); }

// xyz, out [F, N, 3] (out == xyz: in place); boxvectors [3, 3, F]; status [3], cleared here; the list of large groups is derived here
// as the product's callers derive it.  The plan itself: nothing checks the box vectors first.
int emu_wrap_cell(const float* xyz, long long N, long long F, const double* boxvectors, const unsigned* starts, long long G,
                  const unsigned* centersel, long long n_c, const float* center, int mode, float* out, int* status, int avoid)
{
    WrapCellEmuBackend be;
    g_err.clear();
    std::vector<unsigned> large;
    const long long small_max = wrap_small_max(avoid);
    for (long long g = 0; starts && g < G; ++g)
        if ((long long)starts[g + 1] - (long long)starts[g] > small_max) large.push_back((unsigned)g);
    WrapCellArgs c;
    WrapArgs& a = c.w;
    a.xyz = xyz; a.n_atoms = N; a.n_frames = F; a.starts = starts; a.n_groups = G;
    a.large = large.empty() ? nullptr : large.data(); a.n_large = (long long)large.size();
    a.centersel = centersel; a.n_centersel = n_c; a.out = out;
    if (center) { a.center[0] = center[0]; a.center[1] = center[1]; a.center[2] = center[2]; }
    c.boxvectors = boxvectors; c.mode = mode; c.status = status;
    if (status) memset(status, 0, WRAP_CELL_NSTATUS * sizeof(int));
    const int st = run_wrap_cell(be, c, g_err, avoid);
    g_kernel = be.kernel;
    return st;
}

}  // extern "C"
