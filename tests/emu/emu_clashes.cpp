// tests/emu/emu_clashes.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the steric-clash kernels (moleculekit_amd/csrc/clash_kernels.h, and the bond guesser's cell-list kernels under them) through
// their launch plan (clash_pipeline.h) on the host SIMT emulation of emu_device.h: the product's kernel source, host memory instead of
// HBM.  Built into tests/emu/libmkamd_emu_clashes.so by tests/emu_clashes_build.py (-ffp-contract=off).
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/clash_pipeline.h"

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace mkamd;

namespace {

struct ClashEmuBackend {
    void* bufs[WS_NSLOTS] = {};
    size_t caps[WS_NSLOTS] = {};
    std::string kernel;
    ~ClashEmuBackend() { for (void* p : bufs) free(p); }
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

thread_local std::string g_err, g_kernel;
thread_local std::vector<int> g_pairs;
thread_local std::vector<float> g_dist, g_over;

}  // namespace

extern "C" {

const char* emu_clashes_last_error() { return g_err.c_str(); }
const char* emu_clashes_last_kernel() { return g_kernel.c_str(); }
const int* emu_clashes_pairs() { return g_pairs.data(); }
const float* emu_clashes_dist() { return g_dist.data(); }
const float* emu_clashes_over() { return g_over.data(); }

// info double [8]: boxes per axis, the box side, the largest occupancy, the owners, the selected atoms, 0.  Returns the status;
// *n_pairs the rows of emu_clashes_pairs() / _dist() / _over(), in the pair kernels' order.
int emu_find_clashes(const float* coords, const float* radii, const unsigned* sel1, const unsigned* sel2, long long n, int self_mode,
                     const unsigned* ex_start, const unsigned* ex_partner, double overlap, double cutoff, double max_boxes, int avoid,
                     long long* n_pairs, double* info)
{
    ClashEmuBackend be;
    g_err.clear();
    g_pairs.clear(); g_dist.clear(); g_over.clear();
    ClashArgs a;
    a.coords = coords; a.radii = radii; a.sel1 = sel1; a.sel2 = sel2; a.n = n; a.self_mode = self_mode;
    a.ex_start = ex_start; a.ex_partner = ex_partner;
    a.overlap = overlap; a.cutoff = cutoff; a.max_boxes = max_boxes;
    ClashResult R;
    const int st = run_find_clashes(be, a, R, g_err, avoid);
    *n_pairs = st ? 0 : R.n_pairs;
    if (!st && R.n_pairs) {
        g_pairs.assign(R.pairs, R.pairs + 2 * R.n_pairs);
        g_dist.assign(R.dists, R.dists + R.n_pairs);
        g_over.assign(R.overs, R.overs + R.n_pairs);
    }
    for (int ax = 0; ax < 3; ++ax) info[ax] = (double)R.boxes[ax];
    info[3] = R.side;
    info[4] = (double)R.max_occ;
    info[5] = (double)R.n_owners;
    info[6] = (double)R.n_selected;
    info[7] = 0.0;
    g_kernel = be.kernel;
    return st;
}

// the host's box side alone (clash_pipeline.h: clash_grid): info double [4]
int emu_clash_grid(const float* mn, const float* mx, double cutoff, double max_boxes, double* info)
{
    g_err.clear();
    const float lo[3] = {mn[0], mn[1], mn[2]}, hi[3] = {mx[0], mx[1], mx[2]};
    long long boxes[3] = {0, 0, 0};
    double side = 0.0;
    const int st = clash_grid(lo, hi, cutoff, max_boxes, boxes, &side, g_err);
    for (int ax = 0; ax < 3; ++ax) info[ax] = (double)boxes[ax];
    info[3] = side;
    return st;
}

}  // extern "C"
