// tests/emu/emu_sasa.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the surface-area kernels (moleculekit_amd/csrc/sasa_kernels.h) through their launch plan (sasa_pipeline.h) on the host
// SIMT emulation of emu_device.h: the product's kernel source, host memory instead of HBM.  Built into
// tests/emu/libmkamd_emu_sasa.so by tests/emu_sasa_build.py (-ffp-contract=off).
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/sasa_pipeline.h"

#include <cstdlib>
#include <cstring>
#include <string>

using namespace mkamd;

namespace {

struct SasaEmuBackend {
    void* bufs[WS_NSLOTS] = {};
    size_t caps[WS_NSLOTS] = {};
    int compute_units() const { return 256; }
    ~SasaEmuBackend() { for (void* p : bufs) free(p); }
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

thread_local std::string g_err;

}  // namespace

extern "C" {

const char* emu_sasa_last_error() { return g_err.c_str(); }

int emu_sasa(const float* xyz, long long N, long long F, const float* radii, int n_points, const int* mapping, const int* mask,
             float coord_div, float* out, long long n_out)
{
    SasaEmuBackend be;
    g_err.clear();
    SasaArgs a;
    a.xyz = xyz; a.n_atoms = N; a.n_frames = F; a.radii = radii; a.n_points = n_points; a.mapping = mapping; a.mask = mask;
    a.n_out = n_out; a.coord_div = coord_div; a.out = out;
    return run_sasa(be, a, g_err);
}

int emu_sasa_sphere_points(int n, float* out3n)
{
    std::vector<float> p;
    sasa_sphere_points(n, p);
    memcpy(out3n, p.data(), p.size() * sizeof(float));
    return 0;
}

int emu_sasa_max_neighbours() { return SA_MAX_NB; }

}  // extern "C"
