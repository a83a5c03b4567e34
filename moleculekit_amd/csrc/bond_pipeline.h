// bond_pipeline.h -- launch plan of the bond-guesser kernels (bond_kernels.h), written against the backend concept of pipeline.h so
// that the product (capi.hip) and the test emulator (tests/emu/emu_bonds.cpp) run the same plan.
//
// bounds (7 words to the host) -> the host fixes the grid (bond_grid: the reference's escalation loop) -> cells -> flags -> scan ->
// ranks -> scan -> the largest occupancy reaches the host (the cap; the choice of the pair kernels) -> scatter -> sort -> pair
// count -> scan -> the total reaches the host, which sizes the list -> pair fill.  Three round trips: the call is not asynchronous.
// Workspace: two words per box (<= max_boxes <= 2^28 boxes; 32 MB at the reference's 4e6) and seven per atom, the list apart.
#pragma once
#include "bond_kernels.h"
#include "pipeline.h"

#include <cmath>
#include <cstdio>
#include <string>

namespace mkamd {

enum { BOND_AVOID_THREAD = 1, BOND_AVOID_WAVE = 2 };    // `avoid`: the tests walk both lane assignments over the same shapes
constexpr unsigned BOND_WAVE_FROM = WAVE;               // a box this crowded fills a wave's lanes: the wave-per-owner kernels
constexpr double BOND_MAX_BOXES = 268435456.0;          // 2^28: what max_boxes may ask for (two words a box)

struct BondArgs {
    const float* coords = nullptr;         // device float32 [n][3]
    const float* radii = nullptr;          // device float32 [n]
    const unsigned* is_h = nullptr;        // device uint32 [n]: != 0 a hydrogen
    long long n = 0;
    double grid_cutoff = 0.0, max_boxes = 4e6, cutoff_incr = 1.26;
};

struct BondResult {
    long long n_pairs = 0;
    const int* pairs = nullptr;            // device int32 [n_pairs][2], the backend's WS_BD_PAIRS
    long long boxes[3] = {0, 0, 0};        // the grid the call settled on
    double pairdist = 0.0;
    unsigned max_occ = 0;                  // atoms of the most crowded box
};

// The reference's grid: boxes per axis floor(range / float32(pairdist)) + 1 with range = max - min in float32, pairdist multiplied
// by cutoff_incr in double while the product of the counts exceeds max_boxes.  A quotient that is not finite or does not fit an
// integer counts as "exceeds".
inline int bond_grid(const float (&mn)[3], const float (&mx)[3], double grid_cutoff, double max_boxes, double cutoff_incr, long long (&boxes)[3],
                     double* pairdist, std::string& err)
{
    if (!(grid_cutoff > 0.0) || !std::isfinite(grid_cutoff)) { err = "grid_cutoff must be positive and finite"; return ST_EINVAL; }
    if (!(max_boxes >= 1.0) || !(max_boxes <= BOND_MAX_BOXES)) { err = "max_boxes must lie in [1, 2^28]"; return ST_EINVAL; }
    if (!(cutoff_incr > 1.0) || !std::isfinite(cutoff_incr)) { err = "cutoff_incr must be a finite number greater than 1"; return ST_EINVAL; }
    double pd = grid_cutoff;
    for (int round = 0; round < 100000; ++round) {
        const float pdf = (float)pd;
        bool over = false;
        double product = 1.0;
        for (int ax = 0; ax < 3; ++ax) {
            const volatile float range = mx[ax] - mn[ax];
            const volatile float q = range / pdf;
            const float fl = std::floor((float)q);
            if (!(fl >= 0.0f) || !(fl < 4.0e18f)) { over = true; break; }
            boxes[ax] = (long long)fl + 1;
            product *= (double)boxes[ax];
        }
        if (!over && !(product > max_boxes)) { *pairdist = pd; return ST_OK; }
        pd *= cutoff_incr;
        if (!std::isfinite(pd)) break;
    }
    err = "grid_cutoff: no box side keeps the grid within max_boxes";
    return ST_EINVAL;
}

template <class BE>
int bond_scan(BE& be, unsigned* counts /* zeroed once read */, size_t n, unsigned* starts /* n + 1 */)
{
    const size_t nchunks = (n + 1 + SCAN_CHUNK - 1) / SCAN_CHUNK;
    void* chunks = nullptr;
    int st = be.ensure(WS_BD_CHUNKS, nchunks * sizeof(unsigned), &chunks, 0);
    if (st) return st;
    if ((st = be.launch(k_scan_chunk_sums, dim3((unsigned)nchunks), dim3(SCAN_THREADS), (const unsigned*)counts, n, (unsigned*)chunks))) return st;
    if ((st = be.launch(k_scan_sums_inplace, dim3(1), dim3(SCAN_THREADS), (unsigned*)chunks, (unsigned)nchunks))) return st;
    return be.launch(k_scan_finish, dim3((unsigned)nchunks), dim3(SCAN_THREADS), counts, n, (const unsigned*)chunks, starts, (const unsigned*)nullptr);
}

// The list is the backend's WS_BD_PAIRS buffer: valid until the next bond call on it.
template <class BE>
int run_guess_bonds(BE& be, const BondArgs& a, BondResult& R, std::string& err, int avoid = 0)
{
    R = BondResult{};
    const long long n = a.n;
    if (n < 0) { err = "negative size"; return ST_EINVAL; }
    if (n >= 0x80000000LL) { err = "too many atoms (>= 2^31)"; return ST_EINVAL; }
    if (!(a.grid_cutoff > 0.0) || !std::isfinite(a.grid_cutoff)) { err = "grid_cutoff must be positive and finite"; return ST_EINVAL; }
    if (n == 0) return ST_OK;
    if (!a.coords || !a.radii || !a.is_h) { err = "NULL pointer"; return ST_EINVAL; }
    int st;
    char buf[256];
    const size_t N = (size_t)n;
    const unsigned blocks = (unsigned)((N + BD_THREADS - 1) / BD_THREADS);

    // bounds
    void* dstat = nullptr;
    if ((st = be.ensure(WS_BD_STAT, BD_WORDS * 4, &dstat, 0))) return st;
    unsigned* stat = (unsigned*)dstat;
    unsigned h[BD_WORDS] = {};
    for (int ax = 0; ax < 3; ++ax) h[BD_MIN + ax] = 0xffffffffu;
    h[BD_CROWDED] = 0xffffffffu;
    if ((st = be.to_device(stat, h, sizeof h))) return st;
    if ((st = be.launch(k_bond_bounds, dim3(blocks < 1024u ? blocks : 1024u), dim3(BD_THREADS), a.coords, n, stat))) return st;
    if ((st = be.to_host(h, stat, sizeof h))) return st;
    if (h[BD_NONFINITE]) { err = "non-finite coordinates (NaN or inf): coordinates must be finite"; return ST_EINVAL; }
    BondGrid g;
    float mn[3], mx[3];
    for (int ax = 0; ax < 3; ++ax) { mn[ax] = bond_unkey(h[BD_MIN + ax]); mx[ax] = bond_unkey(h[BD_MAX + ax]); g.mn[ax] = mn[ax]; }
    if ((st = bond_grid(mn, mx, a.grid_cutoff, a.max_boxes, a.cutoff_incr, R.boxes, &R.pairdist, err))) return st;
    g.nx = (int)R.boxes[0]; g.ny = (int)R.boxes[1]; g.nz = (int)R.boxes[2];
    g.pd = (float)R.pairdist;
    { const volatile float c2 = g.pd * g.pd; g.cutoff2 = c2; }
    const size_t nb = (size_t)R.boxes[0] * (size_t)R.boxes[1] * (size_t)R.boxes[2];              // <= 2^28

    // cells -> the boxes' ranks and starts
    void *box_cnt, *box_low, *atom_box, *wa, *wb, *start, *tmp, *order;
    if ((st = be.ensure(WS_BD_BOXCNT, nb * 4, &box_cnt, 0)) || (st = be.ensure(WS_BD_BOXLOW, nb * 4, &box_low, 0)) ||
        (st = be.ensure(WS_BD_ATOMBOX, N * 4, &atom_box, 0)) || (st = be.ensure(WS_BD_A, N * 4, &wa, 0)) ||
        (st = be.ensure(WS_BD_B, (N + 1) * 4, &wb, 0)) || (st = be.ensure(WS_BD_START, (N + 1) * 4, &start, 0)) ||
        (st = be.ensure(WS_BD_TMP, N * 4, &tmp, 0)) || (st = be.ensure(WS_BD_ORDER, N * 4, &order, 0)))
        return st;
    if ((st = be.fill(box_cnt, 0, nb * 4)) || (st = be.fill(box_low, 0xff, nb * 4))) return st;
    const dim3 grid(blocks), block(BD_THREADS);
    if ((st = be.launch(k_bond_cells, grid, block, a.coords, n, g, (unsigned*)atom_box, (unsigned*)box_cnt, (unsigned*)box_low))) return st;
    if ((st = be.launch(k_bond_flags, grid, block, n, (const unsigned*)atom_box, (const unsigned*)box_low, (unsigned*)wa))) return st;
    if ((st = bond_scan(be, (unsigned*)wa, N, (unsigned*)wb))) return st;                        // wb: the ranks; wa is zero again
    if ((st = be.launch(k_bond_ranks, grid, block, n, (const unsigned*)atom_box, (const unsigned*)wb, (const unsigned*)box_cnt, (unsigned*)box_low,
                        (unsigned*)wa, stat)))
        return st;
    if ((st = be.to_host(h, stat, sizeof h))) return st;
    R.max_occ = h[BD_MAXOCC];
    const size_t M = h[BD_NBOXES];                                                               // occupied boxes, 1 <= M <= n
    if (M == 0 || M > N) { err = "internal: the cell list lost its boxes"; return ST_EHIP; }
    if (R.max_occ > BOND_BOX_CAP) {
        const unsigned b = h[BD_CROWDED], per = (unsigned)(g.nx * g.ny);
        snprintf(buf, sizeof buf, "crowded box: box %u (x %u, y %u, z %u of %d x %d x %d, side %.6g) holds %u atoms, more than the %u a box may hold",
                 b, b % per % (unsigned)g.nx, b % per / (unsigned)g.nx, b / per, g.nx, g.ny, g.nz, R.pairdist, R.max_occ, BOND_BOX_CAP);
        err = buf;
        return ST_EINVAL;
    }
    if ((st = bond_scan(be, (unsigned*)wa, M, (unsigned*)start))) return st;                     // the boxes' starts by rank; wa is zero again
    if ((st = be.launch(k_bond_scatter, grid, block, n, (const unsigned*)atom_box, (const unsigned*)box_low, (const unsigned*)start, (unsigned*)box_cnt,
                        (unsigned*)tmp)))
        return st;
    if ((st = be.launch(k_bond_sort, grid, block, n, (const unsigned*)atom_box, (const unsigned*)box_low, (const unsigned*)start, (const unsigned*)tmp,
                        (unsigned*)order)))
        return st;

    // pairs: count -> scan -> fill
    const bool wave = (avoid & BOND_AVOID_THREAD) || (!(avoid & BOND_AVOID_WAVE) && R.max_occ >= BOND_WAVE_FROM);
    be.note_dist_kernel(wave ? "mkamd::k_bond_pairs_wave" : "mkamd::k_bond_pairs_thread");
    const dim3 pgrid(wave ? (unsigned)((N + 3) / 4) : blocks);
    unsigned long long* total = (unsigned long long*)(stat + BD_TOTAL);
    auto pairs = [&](auto kern, int* out) {
        return be.launch(kern, pgrid, block, a.coords, a.radii, a.is_h, n, g, (const unsigned*)atom_box, (const unsigned*)box_low, (const unsigned*)start,
                         (const unsigned*)order, (unsigned*)wa, (const unsigned*)wb, total, out);
    };
    if ((st = wave ? pairs(k_bond_pairs_wave<false>, nullptr) : pairs(k_bond_pairs_thread<false>, nullptr))) return st;
    if ((st = be.to_host(h, stat, sizeof h))) return st;
    unsigned long long found;
    memcpy(&found, h + BD_TOTAL, 8);
    if (found > 0x7fffffffull) { err = "more than 2^31 bonds: the coordinates are not a molecule's"; return ST_EINVAL; }
    if (found == 0) return ST_OK;
    if ((st = bond_scan(be, (unsigned*)wa, N, (unsigned*)wb))) return st;                        // wb: every owner's first row
    void* out = nullptr;
    if ((st = be.ensure(WS_BD_PAIRS, (size_t)found * 8, &out, 0))) return st;
    if ((st = wave ? pairs(k_bond_pairs_wave<true>, (int*)out) : pairs(k_bond_pairs_thread<true>, (int*)out))) return st;
    R.n_pairs = (long long)found;
    R.pairs = (const int*)out;
    return ST_OK;
}

}  // namespace mkamd
