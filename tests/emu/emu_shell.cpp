// tests/emu/emu_shell.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the shell-count kernels (moleculekit_amd/csrc/shell_kernels.h) through their launch plan (shell_pipeline.h) on the host
// SIMT emulation of emu_device.h: the product's kernel source, host memory instead of HBM.  Built into
// tests/emu/libmkamd_emu_shell.so by tests/emu_shell_build.py (-ffp-contract=off).
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/shell_pipeline.h"

#include <cstdlib>
#include <cstring>
#include <string>

using namespace mkamd;

namespace {

struct ShellEmuBackend {
    void* bufs[WS_NSLOTS] = {};
    size_t caps[WS_NSLOTS] = {};
    size_t workspace = 0;                  // bytes of workspace the plan asked for (the tests bound it)
    std::string kernel;
    int compute_units() const { return 256; }
    ~ShellEmuBackend() { for (void* p : bufs) free(p); }
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

const char* emu_shell_last_error() { return g_err.c_str(); }
const char* emu_shell_last_kernel() { return g_kernel.c_str(); }
long long emu_shell_last_workspace() { return g_workspace; }

int emu_shell_counts(const float* coords, long long F, const float* box, const unsigned* sel1, long long n1, const unsigned* sel2, long long n2,
                     const unsigned* chains, int symmetric, int pbc, const float* thresholds, long long n_edges, int* counts, int avoid)
{
    ShellEmuBackend be;
    g_err.clear();
    const int st = run_shell_counts(be, coords, F, box, sel1, n1, sel2, n2, chains, symmetric, pbc, thresholds, n_edges, counts, g_err, avoid);
    g_kernel = be.kernel;
    g_workspace = (long long)be.workspace;
    return st;
}

}  // extern "C"
