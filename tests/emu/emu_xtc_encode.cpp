// tests/emu/emu_xtc_encode.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the device XTC writer's kernels (moleculekit_amd/csrc/xtc_encode.h) through their launch plan (run_xtc_encode) on the host
// SIMT emulation of emu_device.h: the product's kernel source, host memory instead of HBM.  Built into
// tests/emu/libmkamd_emu_xtc_encode.so by tests/emu_xtc_encode_build.py (-ffp-contract=off); tests/emu/xtc_encode_main.cpp includes this
// file for the same entry points in a program of its own.
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/xtc_encode.h"

#include <cstdint>
#include <cstring>

using namespace mkamd;

namespace {

struct XtcEncodeEmuBackend {
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

uint64_t emu_xtc_encode_work_bytes(long long n_frames, long long n_atoms) { return xtc_encode_layout(n_frames, n_atoms).total; }
uint64_t emu_xtc_encode_bound(long long n_frames, long long n_atoms) { return xtc_encode_bound(n_frames, n_atoms); }

// byte offsets of the integers, the per-frame statistics, the plans and the group records inside the work buffer, and its size
void emu_xtc_encode_layout(long long n_frames, long long n_atoms, uint64_t* out5)
{
    const XtcEncodeLayout L = xtc_encode_layout(n_frames, n_atoms);
    out5[0] = L.ints; out5[1] = L.stats; out5[2] = L.plan; out5[3] = L.groups; out5[4] = L.total;
}

// the checks of mkamd_xtc_encode_dev (capi.hip), then the same launches; 22 = a refused argument
int emu_xtc_encode(const float* xyz, float in_scale, const float* precision, const float* box, const float* time, const int* step,
                   long long n_frames, long long n_atoms, unsigned char* image, uint64_t image_capacity, uint64_t* offsets, int* status,
                   unsigned char* work, uint64_t work_bytes)
{
    if (n_frames < 0 || n_atoms < 0) return 22;
    if (n_frames == 0) return 0;
    if (work_bytes < xtc_encode_layout(n_frames, n_atoms).total || image_capacity < xtc_encode_bound(n_frames, n_atoms)) return 22;
    if (((uintptr_t)work & 7u) || ((uintptr_t)image & 3u)) return 22;
    XtcEncodeEmuBackend be;
    XtcEncodeArgs a;
    a.xyz = xyz; a.in_scale = in_scale; a.precision = precision; a.box = box; a.time = time; a.step = step;
    a.n_frames = n_frames; a.n_atoms = n_atoms;
    a.image = image; a.offsets = reinterpret_cast<unsigned long long*>(offsets); a.status = status; a.work = work;
    return run_xtc_encode(be, a);
}

}  // extern "C"
