// tests/emu/emu_rings.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the ring-interaction kernels (moleculekit_amd/csrc/ring_kernels.h) through their launch plan (ring_pipeline.h) on the host
// SIMT emulation of emu_device.h: the product's kernel source, host memory instead of HBM.  Built into
// tests/emu/libmkamd_emu_rings.so by tests/emu_rings_build.py (-ffp-contract=off).
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/ring_pipeline.h"

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace mkamd;

namespace {

struct RingEmuBackend {
    void* bufs[WS_NSLOTS] = {};
    size_t caps[WS_NSLOTS] = {};
    size_t workspace = 0;                  // bytes of workspace the plan asked for, the lists apart (the tests bound it)
    long long scans = 0;                   // chunks the plan walked
    std::string kernel;
    int compute_units() const { return 256; }
    ~RingEmuBackend() { for (void* p : bufs) free(p); }
    void note_dist_kernel(const char* name) { kernel = name; }
    int ensure(int slot, size_t bytes, void** ptr, int = 0)
    {
        if (bytes == 0) bytes = 16;
        if (caps[slot] < bytes) {
            free(bufs[slot]);
            bufs[slot] = malloc(bytes);
            memset(bufs[slot], 0xCD, bytes);          // poison: catch reads of unwritten workspace
            if (slot != WS_H_OUT && slot != WS_R_OUT2) workspace += bytes - caps[slot];
            caps[slot] = bytes;
        }
        *ptr = bufs[slot];
        return 0;
    }
    int grow_keep(int slot, size_t bytes, size_t keep_bytes, void** ptr)
    {
        if (bytes == 0) bytes = 16;
        if (caps[slot] < bytes) {
            void* fresh = malloc(bytes);               // exactly what was asked for: every chunk moves the list
            memset(fresh, 0xCD, bytes);
            if (bufs[slot] && keep_bytes) memcpy(fresh, bufs[slot], keep_bytes);
            free(bufs[slot]);
            bufs[slot] = fresh;
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
        if ((void*)kernel == (void*)k_contacts_scan) ++scans;
        emu::launch(kernel, grid, block, args...);
        return 0;
    }
};

thread_local std::string g_err, g_kernel;
thread_local long long g_workspace = 0, g_chunks = 0;
thread_local std::vector<unsigned> g_pairs;
thread_local std::vector<float> g_distang;

}  // namespace

extern "C" {

const char* emu_rings_last_error() { return g_err.c_str(); }
const char* emu_rings_last_kernel() { return g_kernel.c_str(); }
long long emu_rings_last_workspace() { return g_workspace; }
long long emu_rings_last_chunks() { return g_chunks; }
const unsigned* emu_rings_pairs() { return g_pairs.data(); }
const float* emu_rings_distang() { return g_distang.data(); }

// device_sink: the lists grow in "device" memory (RingDeviceSink) instead of coming down chunk by chunk
int emu_rings(int kind, const float* coords, long long F, const float* box, const unsigned* ring_atoms, long long n_ring_atoms,
              const unsigned* starts1, long long n1, const unsigned* starts2, const unsigned* partners, long long n2, const float* thr,
              long long budget_bytes, long long chunk_frames, int avoid, int device_sink, long long* frame_offsets)
{
    RingEmuBackend be;
    g_err.clear();
    g_pairs.clear();
    g_distang.clear();
    RingArgs a;
    a.kind = kind;
    a.coords = coords; a.F = F; a.box = box;
    a.ring_atoms = ring_atoms; a.n_ring_atoms = n_ring_atoms;
    a.starts1 = starts1; a.n1 = n1; a.starts2 = starts2; a.partners = partners; a.n2 = n2;
    a.emit = kind == RING_PIPI ? nullptr : partners;
    a.estride = kind == RING_SIGMAHOLE ? 2 : 1;
    for (int i = 0; i < 4; ++i) a.thr[i] = thr[i];
    int st;
    if (device_sink) {
        RingDeviceSink<RingEmuBackend> sink{be};
        st = run_ring_interactions(be, a, (size_t)budget_bytes, chunk_frames, frame_offsets, sink, g_err, avoid);
        if (!st && sink.size) {
            g_pairs.assign((const unsigned*)sink.pairs, (const unsigned*)sink.pairs + 2 * sink.size);
            g_distang.assign((const float*)sink.distang, (const float*)sink.distang + 2 * sink.size);
        }
    } else {
        st = run_ring_interactions(be, a, (size_t)budget_bytes, chunk_frames, frame_offsets, RingHostSink<RingEmuBackend>{be, g_pairs, g_distang}, g_err, avoid);
    }
    g_kernel = be.kernel;
    g_workspace = (long long)be.workspace;
    g_chunks = be.scans;
    return st;
}

}  // extern "C"
