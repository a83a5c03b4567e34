// tests/emu/emu_dssp.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the secondary-structure kernels (moleculekit_amd/csrc/dssp_kernels.h) through their launch plan (dssp_pipeline.h) on the
// host SIMT emulation of emu_device.h: the product's kernel source, host memory instead of HBM.  Built into
// tests/emu/libmkamd_emu_dssp.so by tests/emu_dssp_build.py (-ffp-contract=off).
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/dssp_pipeline.h"

#include <cstdlib>
#include <cstring>
#include <string>

using namespace mkamd;

namespace {

struct DsspEmuBackend {
    void* bufs[WS_NSLOTS] = {};
    size_t caps[WS_NSLOTS] = {};
    size_t workspace = 0;                  // bytes of workspace the plan asked for (the tests bound it)
    std::string kernel;
    int launches = 0;
    int compute_units() const { return 256; }
    ~DsspEmuBackend() { for (void* p : bufs) free(p); }
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
        ++launches;
        emu::launch(kernel, grid, block, args...);
        return 0;
    }
};

thread_local std::string g_err, g_kernel;
thread_local long long g_workspace = 0, g_chunks = 0;

}  // namespace

extern "C" {

const char* emu_dssp_last_error() { return g_err.c_str(); }
const char* emu_dssp_last_kernel() { return g_kernel.c_str(); }
long long emu_dssp_last_workspace() { return g_workspace; }
long long emu_dssp_last_chunks() { return g_chunks; }
int emu_dssp_takes_atoms(long long F, long long R) { return dssp_takes_atoms(F, R) ? 1 : 0; }

// slot_a int32 [F, R, 2], slot_e float32 [F, R, 2] (NULL: not wanted), out uint8 [F, R]
int emu_dssp(const float* coords, long long F, const unsigned* ca, const unsigned* nco, const int* proline, const int* chain, long long R,
             int simplified, unsigned char* out, int* slot_a, float* slot_e, int avoid)
{
    DsspEmuBackend be;
    g_err.clear();
    g_chunks = 0;
    auto after = [&](const DsspWs& w, long long f0, long long fc) {
        ++g_chunks;
        if (slot_a && slot_e)
            for (long long f = 0; f < fc; ++f)
                for (long long r = 0; r < R; ++r)
                    for (int k = 0; k < 2; ++k) {
                        const size_t at = ((size_t)k * (size_t)R + (size_t)r) * (size_t)fc + (size_t)f;
                        slot_a[((f0 + f) * R + r) * 2 + k] = w.slot_a[at];
                        slot_e[((f0 + f) * R + r) * 2 + k] = w.slot_e[at];
                    }
        return 0;
    };
    const int st = run_dssp(be, coords, F, ca, nco, proline, chain, R, simplified, out, g_err, avoid, after);
    g_kernel = be.kernel;
    g_workspace = (long long)be.workspace;
    return st;
}

}  // extern "C"
