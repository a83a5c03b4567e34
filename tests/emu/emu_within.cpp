// tests/emu/emu_within.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the proximity-selection kernels (moleculekit_amd/csrc/within_kernels.h, and the bond guesser's cell-list kernels under them)
// through their launch plan (within_pipeline.h) on the host SIMT emulation of emu_device.h: the product's kernel source, host memory
// instead of HBM.  Built into tests/emu/libmkamd_emu_within.so by tests/emu_within_build.py (-ffp-contract=off).
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/within_pipeline.h"

#include <cstdlib>
#include <cstring>
#include <string>

using namespace mkamd;

namespace {

struct WithinEmuBackend {
    void* bufs[WS_NSLOTS] = {};
    size_t caps[WS_NSLOTS] = {};
    std::string kernel;
    ~WithinEmuBackend() { for (void* p : bufs) free(p); }
    void note_dist_kernel(const char* name) { kernel = name; }
    int ensure(int slot, size_t bytes, void** ptr, int = 0)
    {
        if (bytes == 0) bytes = 16;
        if (caps[slot] < bytes) {
            free(bufs[slot]);
            bufs[slot] = aligned_alloc(16, (bytes + 15) / 16 * 16);
            memset(bufs[slot], 0xCD, bytes);          // poison: catch reads of unwritten workspace
            caps[slot] = bytes;
        }
        *ptr = bufs[slot];
        return 0;
    }
    int fill(void* p, int byte, size_t bytes) { memset(p, byte, bytes); return 0; }
    int to_host(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
    int to_device(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
    template <class... KA, class... A>
    int launch(void (*kernel)(KA...), dim3 grid, dim3 block, A... args)
    {
        emu::launch(kernel, grid, block, args...);
        return 0;
    }
};

thread_local std::string g_err, g_kernel, g_left;

}  // namespace

extern "C" {

const char* emu_within_last_error() { return g_err.c_str(); }
const char* emu_within_last_kernel() { return g_kernel.c_str(); }
const char* emu_within_left() { return g_left.c_str(); }              // why the cell path was left ("" where it was not)

// coords float32 [F][N][3]; gate float32 [F][2][3] or NULL; out uint8 [F][n1], poisoned by the caller.  no_cull: the diagnostics
// switch of within_pipeline.h.  info double [8]: boxes per axis, the box side, the largest occupancy, 1 where the cell path ran.
int emu_within(const float* coords, long long n_atoms, long long n_frames, const unsigned* sel1, long long n1, const unsigned* sel2, long long n2,
               float cutoff, const float* gate, int avoid, int no_cull, unsigned char* out, double* info)
{
    WithinEmuBackend be;
    g_err.clear();
    WithinArgs a;
    a.coords = coords; a.n_atoms = n_atoms; a.n_frames = n_frames;
    a.sel1 = sel1; a.n1 = n1; a.sel2 = sel2; a.n2 = n2;
    a.cutoff = cutoff; a.gate = gate; a.out = out; a.no_cull = no_cull;
    WithinResult R;
    const int st = run_within(be, a, R, g_err, avoid);
    for (int ax = 0; ax < 3; ++ax) info[ax] = (double)R.boxes[ax];
    info[3] = R.side;
    info[4] = (double)R.max_occ;
    info[5] = (double)R.cells;
    info[6] = info[7] = 0.0;
    g_kernel = be.kernel;
    g_left = R.left;
    return st;
}

}  // extern "C"
