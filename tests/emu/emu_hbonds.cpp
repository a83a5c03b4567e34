// tests/emu/emu_hbonds.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the hydrogen-bond kernels (moleculekit_amd/csrc/hbond_kernels.h) through their launch plan (hbond_pipeline.h) on the host
// SIMT emulation of emu_device.h: the product's kernel source, host memory instead of HBM.  Built into
// tests/emu/libmkamd_emu_hbonds.so by tests/emu_hbonds_build.py (-ffp-contract=off).
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/hbond_pipeline.h"

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace mkamd;

namespace {

struct HbondEmuBackend {
    void* bufs[WS_NSLOTS] = {};
    size_t caps[WS_NSLOTS] = {};
    size_t workspace = 0;                  // bytes of workspace the plan asked for, the list apart (the tests bound it)
    long long scans = 0;                   // chunks the plan walked
    std::string kernel;
    int compute_units() const { return 256; }
    ~HbondEmuBackend() { for (void* p : bufs) free(p); }
    void note_dist_kernel(const char* name) { kernel = name; }
    int ensure(int slot, size_t bytes, void** ptr, int = 0)
    {
        if (bytes == 0) bytes = 16;
        if (caps[slot] < bytes) {
            free(bufs[slot]);
            bufs[slot] = malloc(bytes);
            memset(bufs[slot], 0xCD, bytes);          // poison: catch reads of unwritten workspace
            if (slot != WS_H_OUT) workspace += bytes - caps[slot];
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
thread_local std::vector<int> g_triples;

}  // namespace

extern "C" {

const char* emu_hbonds_last_error() { return g_err.c_str(); }
const char* emu_hbonds_last_kernel() { return g_kernel.c_str(); }
long long emu_hbonds_last_workspace() { return g_workspace; }
long long emu_hbonds_last_chunks() { return g_chunks; }
const int* emu_hbonds_triples() { return g_triples.data(); }

// device_sink: the list grows in "device" memory (HbondDeviceSink) instead of coming down chunk by chunk; names: what the list calls the
// atoms (null: their indices)
int emu_hbonds(const float* coords, long long n_atoms, long long F, const float* box, const unsigned* donors, long long nd,
               const unsigned* acceptors, long long na, const unsigned* sel1, const unsigned* sel2, const unsigned* names, float dist_threshold,
               float angle_threshold, int intra, int ignore_hs, long long budget_bytes, long long chunk_frames, int avoid, int device_sink,
               long long* frame_offsets)
{
    HbondEmuBackend be;
    g_err.clear();
    g_triples.clear();
    HbondArgs a;
    a.coords = coords; a.n_atoms = n_atoms; a.F = F; a.box = box;
    a.donors = donors; a.nd = nd; a.acceptors = acceptors; a.na = na; a.sel1 = sel1; a.sel2 = sel2;
    a.names = names;
    a.dist_threshold = dist_threshold; a.angle_threshold = angle_threshold;
    a.intra = intra != 0; a.ignore_hs = ignore_hs != 0;
    int st;
    if (device_sink) {
        HbondDeviceSink<HbondEmuBackend> sink{be};
        st = run_hbonds(be, a, (size_t)budget_bytes, chunk_frames, frame_offsets, sink, g_err, avoid);
        if (!st && sink.size) g_triples.assign((const int*)sink.triples, (const int*)sink.triples + 3 * sink.size);
    } else {
        st = run_hbonds(be, a, (size_t)budget_bytes, chunk_frames, frame_offsets, HbondHostSink<HbondEmuBackend>{be, g_triples}, g_err, avoid);
    }
    g_kernel = be.kernel;
    g_workspace = (long long)be.workspace;
    g_chunks = be.scans;
    return st;
}

}  // extern "C"
