// tests/emu/emu_bonds.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives the bond-guesser kernels (moleculekit_amd/csrc/bond_kernels.h) through their launch plan (bond_pipeline.h) on the host SIMT
// emulation of emu_device.h: the product's kernel source, host memory instead of HBM.  Built into tests/emu/libmkamd_emu_bonds.so by
// tests/emu_bonds_build.py (-ffp-contract=off).
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/bond_pipeline.h"

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace mkamd;

namespace {

struct BondEmuBackend {
    void* bufs[WS_NSLOTS] = {};
    size_t caps[WS_NSLOTS] = {};
    size_t workspace = 0;                  // bytes of workspace the plan asked for, the list apart
    std::string kernel;
    ~BondEmuBackend() { for (void* p : bufs) free(p); }
    void note_dist_kernel(const char* name) { kernel = name; }
    int ensure(int slot, size_t bytes, void** ptr, int = 0)
    {
        if (bytes == 0) bytes = 16;
        if (caps[slot] < bytes) {
            free(bufs[slot]);
            bufs[slot] = malloc(bytes);
            memset(bufs[slot], 0xCD, bytes);          // poison: catch reads of unwritten workspace
            if (slot != WS_BD_PAIRS) workspace += bytes - caps[slot];
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
thread_local std::vector<int> g_pairs;

}  // namespace

extern "C" {

const char* emu_bonds_last_error() { return g_err.c_str(); }
const char* emu_bonds_last_kernel() { return g_kernel.c_str(); }
long long emu_bonds_last_workspace() { return g_workspace; }
const int* emu_bonds_pairs() { return g_pairs.data(); }

// info double [5]: boxes per axis, pairdist, the largest occupancy.  Returns the status; *n_pairs the rows of emu_bonds_pairs().
int emu_guess_bonds(const float* coords, const float* radii, const unsigned* is_h, long long n, double grid_cutoff, double max_boxes,
                    double cutoff_incr, int avoid, long long* n_pairs, double* info)
{
    BondEmuBackend be;
    g_err.clear();
    g_pairs.clear();
    BondArgs a;
    a.coords = coords; a.radii = radii; a.is_h = is_h; a.n = n;
    a.grid_cutoff = grid_cutoff; a.max_boxes = max_boxes; a.cutoff_incr = cutoff_incr;
    BondResult R;
    const int st = run_guess_bonds(be, a, R, g_err, avoid);
    *n_pairs = st ? 0 : R.n_pairs;
    if (!st && R.n_pairs) g_pairs.assign(R.pairs, R.pairs + 2 * R.n_pairs);
    for (int ax = 0; ax < 3; ++ax) info[ax] = (double)R.boxes[ax];
    info[3] = R.pairdist;
    info[4] = (double)R.max_occ;
    g_kernel = be.kernel;
    g_workspace = (long long)be.workspace;
    return st;
}

// the host's escalation loop alone (bond_pipeline.h: bond_grid): info double [4]
int emu_bond_grid(const float* mn, const float* mx, double grid_cutoff, double max_boxes, double cutoff_incr, double* info)
{
    g_err.clear();
    const float lo[3] = {mn[0], mn[1], mn[2]}, hi[3] = {mx[0], mx[1], mx[2]};
    long long boxes[3] = {0, 0, 0};
    double pd = 0.0;
    const int st = bond_grid(lo, hi, grid_cutoff, max_boxes, cutoff_incr, boxes, &pd, g_err);
    for (int ax = 0; ax < 3; ++ax) info[ax] = (double)boxes[ax];
    info[3] = pd;
    return st;
}

}  // extern "C"
