// tests/emu/emu_dcd.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the device DCD kernels (moleculekit_amd/csrc/dcd_kernels.h) through their launch plans (run_dcd_decode / run_dcd_encode) on
// the host SIMT emulation of emu_device.h: the product's kernel source, host memory instead of HBM.  Built into
// tests/emu/libmkamd_emu_dcd.so by tests/emu_dcd_build.py.
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/dcd_kernels.h"

#include <cstdint>
#include <cstring>

using namespace mkamd;

namespace {

struct DcdEmuBackend {
    int fill(void* p, int byte, size_t bytes) { memset(p, byte, bytes); return 0; }
    template <class... KA, class... A>
    int launch(void (*kernel)(KA...), dim3 grid, dim3 block, A... args)
    {
        emu::launch(kernel, grid, block, args...);
        return 0;
    }
};

}  // namespace

extern "C" {

// the checks of mkamd_dcd_decode_dev (capi.hip), then the same launches; 22 = a refused argument
int emu_dcd_decode(const unsigned char* bytes, uint64_t n_bytes, const void* desc, long long n_frames, const int* sel, const int* src,
                   long long n_sel, const float* frame0, long long n_atoms, float scale, float* xyz, int* status)
{
    if (n_frames < 0 || n_sel < 0 || n_atoms < 0) return 22;
    if (n_frames == 0) return 0;
    if ((uintptr_t)bytes & 3u) return 22;
    DcdEmuBackend be;
    return run_dcd_decode(be, bytes, (unsigned long long)n_bytes, static_cast<const dcd::FrameDesc*>(desc), n_frames, sel, src, n_sel, frame0, n_atoms,
                          scale, xyz, status);
}

uint64_t emu_dcd_encode_bound(long long n_frames, long long n_atoms, int with_cell)
{
    return (uint64_t)n_frames * dcd_frame_bytes(n_atoms, with_cell != 0);
}

int emu_dcd_encode(const float* xyz, const double* cell, long long n_frames, long long n_atoms, unsigned char* image, uint64_t capacity)
{
    if (n_frames < 0 || n_atoms <= 0) return 22;
    if (n_frames == 0) return 0;
    if (capacity < emu_dcd_encode_bound(n_frames, n_atoms, cell != nullptr) || ((uintptr_t)image & 3u)) return 22;
    DcdEmuBackend be;
    return run_dcd_encode(be, xyz, cell, n_frames, n_atoms, image);
}

}  // extern "C"
