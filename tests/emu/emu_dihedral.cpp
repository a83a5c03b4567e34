// tests/emu/emu_dihedral.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the dihedral kernels (moleculekit_amd/csrc/dihedral_kernels.h) through their launch plan (dihedral_pipeline.h) on the host
// SIMT emulation of emu_device.h: the product's kernel source, host memory instead of HBM.  Built into
// tests/emu/libmkamd_emu_dihedral.so by tests/emu_dihedral_build.py (-ffp-contract=off).
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/dihedral_pipeline.h"

#include <cstdlib>
#include <cstring>
#include <string>

using namespace mkamd;

namespace {

struct DihedralEmuBackend {
    void* bufs[WS_NSLOTS] = {};
    size_t caps[WS_NSLOTS] = {};
    size_t workspace = 0;                  // bytes of workspace the plan asked for (the tests bound it)
    std::string kernel;
    int compute_units() const { return 256; }
    ~DihedralEmuBackend() { for (void* p : bufs) free(p); }
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

thread_local std::string g_err, g_kernel;
thread_local long long g_workspace = 0;

}  // namespace

extern "C" {

const char* emu_dihedral_last_error() { return g_err.c_str(); }
const char* emu_dihedral_last_kernel() { return g_kernel.c_str(); }
long long emu_dihedral_last_workspace() { return g_workspace; }

// box: NULL or [3, F]; wrap as the library's host entry decides it (a box that is not all zeros)
int emu_dihedrals(const float* coords, long long F, const float* box, const unsigned* quads, long long D, int mode, float* out, int avoid)
{
    DihedralEmuBackend be;
    g_err.clear();
    bool wrap = false;
    if (box) for (long long i = 0; i < 3 * F && !wrap; ++i) wrap = !(box[i] == 0.0f);
    const int st = run_dihedrals(be, coords, F, wrap ? box : nullptr, wrap, quads, D, mode, out, g_err, avoid);
    g_kernel = be.kernel;
    g_workspace = (long long)be.workspace;
    return st;
}

}  // extern "C"
