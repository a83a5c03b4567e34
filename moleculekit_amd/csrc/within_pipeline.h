// within_pipeline.h -- launch plan of the proximity-selection kernels (within_kernels.h), written against the backend concept of
// pipeline.h so that the product (capi.hip) and the test emulator (tests/emu/emu_within.cpp) run the same plan.
//
// gather the sources -> their bounding box per frame (the cull) -> ONE of
//   all pairs   k_within_pairs over frames x queries: the whole trajectory path, no round trip, asynchronous
//   cells       one large frame: the bond guesser's cell list over the sources (bounds -> the host fixes the grid -> cells -> flags ->
//               scan -> ranks -> scan -> the cap -> scatter -> sort) -> pack -> k_within_cells.  Two round trips
// The cell path is left for the all-pairs kernel, at the same results and never with an error, where a box holds more than
// BOND_BOX_CAP sources, where a source coordinate is not finite, where sq_cutoff is not finite, where the grid is one box or cannot
// be fixed at all.  Workspace: three words per source and frame, eight per frame; on the cell path the bond guesser's besides.
#pragma once
#include "clash_pipeline.h"
#include "within_kernels.h"

namespace mkamd {

enum { WITHIN_AVOID_PAIRS = 1, WITHIN_AVOID_CELLS = 2 };   // `avoid`: the tests walk both paths over the same shapes
// MEASURED (tools/bench_within.py, the plan sweep): what the all-pairs kernel costs on one frame follows the
// number of SOURCES, not the pair count -- every wave walks all of them, one scalar load after the other, and with one frame there
// are too few waves to hide that -- while the cell list costs its dozen launches and two round trips (0.30 ms) whatever the sizes.
// With 1 024 sources the all-pairs kernel is ahead or level from 4 096 to 1 000 000 queries (0.24 .. 0.33 ms against 0.30 .. 0.33);
// with 4 096 it is behind everywhere (0.46 .. 1.02 ms against 0.31 .. 0.36).  So the rule is the source count alone, at the middle.
constexpr long long WITHIN_CELLS_FROM_SOURCES = 2048;

struct WithinArgs {
    const float* coords = nullptr;         // device float32 [F][N][3]
    long long n_atoms = 0, n_frames = 0;
    const unsigned* sel1 = nullptr;        // device uint32 [n1]: the queries, every index < N
    long long n1 = 0;
    const unsigned* sel2 = nullptr;        // device uint32 [n2]: the sources, every index < N
    long long n2 = 0;
    float cutoff = 0.0f;
    const float* gate = nullptr;           // device float32 [F][2][3] (min, max), or NULL: no gate
    unsigned char* out = nullptr;          // device uint8 [F][n1]
    int no_cull = 0;                       // diagnostics (the emulator's tests): never apply the bounding-box cull
};

struct WithinResult {
    int cells = 0;                         // 1: the cell path ran
    const char* left = "";                 // why the cell path was left, where the plan had taken it
    long long boxes[3] = {0, 0, 0};
    double side = 0.0;
    unsigned max_occ = 0;
};

template <class BE>
int run_within(BE& be, const WithinArgs& a, WithinResult& R, std::string& err, int avoid = 0)
{
    R = WithinResult{};
    const long long F = a.n_frames, N = a.n_atoms, n1 = a.n1, n2 = a.n2;
    if (F < 0 || N < 0 || n1 < 0 || n2 < 0) { err = "negative size"; return ST_EINVAL; }
    if (N >= 0x80000000LL || n1 >= 0x80000000LL || n2 >= 0x80000000LL) { err = "too many atoms (>= 2^31)"; return ST_EINVAL; }
    be.note_dist_kernel("");
    if (F == 0 || n1 == 0) return ST_OK;
    if (!a.out || !a.sel1 || (n2 > 0 && !a.sel2) || !a.coords) { err = "NULL pointer"; return ST_EINVAL; }
    int st;
    if (n2 == 0) return be.fill(a.out, 0, (size_t)F * (size_t)n1);
    const unsigned long long qblocks = (unsigned long long)((n1 + WI_THREADS - 1) / WI_THREADS), sblocks = (unsigned long long)((n2 + WI_THREADS - 1) / WI_THREADS);
    const unsigned bblocks = (unsigned)(sblocks < 64 ? sblocks : 64);
    if (qblocks * (unsigned long long)F >= 0x80000000ULL || sblocks * (unsigned long long)F >= 0x80000000ULL) { err = "too many frames x atoms for one call"; return ST_EINVAL; }

    WithinParams P;
    P.cutoff = a.cutoff;
    { const volatile float sq = a.cutoff * a.cutoff; P.sq_cutoff = sq; }
    P.acut = std::fabs(a.cutoff);
    P.cull = (std::isfinite(P.sq_cutoff) && !a.no_cull) ? 1 : 0;

    void *src, *box;
    if ((st = be.ensure(WS_WI_SRC, (size_t)F * (size_t)n2 * 12, &src, 0)) || (st = be.ensure(WS_WI_BOX, (size_t)F * WI_WORDS * 4, &box, 0))) return st;
    if ((st = be.launch(k_within_gather, dim3((unsigned)(sblocks * (unsigned long long)F)), dim3(WI_THREADS), a.coords, N, a.sel2, n2, (unsigned)sblocks, (float*)src)))
        return st;
    if (P.cull) {
        if ((st = be.fill(box, 0xff, (size_t)F * WI_WORDS * 4))) return st;
        if ((st = be.launch(k_within_bounds, dim3(bblocks * (unsigned)F), dim3(WI_THREADS), (const float*)src, n2, bblocks, (unsigned*)box))) return st;
    }

    auto pairs = [&]() {
        be.note_dist_kernel("mkamd::k_within_pairs");
        return be.launch(k_within_pairs, dim3((unsigned)(qblocks * (unsigned long long)F)), dim3(WI_THREADS), a.coords, N, a.sel1, n1, (const float*)src, n2,
                         a.gate, (const unsigned*)box, P, (unsigned)qblocks, a.out);
    };
    const bool want_cells = F == 1 && ((avoid & WITHIN_AVOID_PAIRS) || (!(avoid & WITHIN_AVOID_CELLS) && n2 >= WITHIN_CELLS_FROM_SOURCES));
    if (!want_cells) return pairs();
    if (!std::isfinite(P.sq_cutoff)) { R.left = "sq_cutoff is not finite"; return pairs(); }

    // the bond guesser's cell list over the sources (clash_pipeline.h: run_find_clashes), the box side from |cutoff|
    const size_t M = (size_t)n2;
    const unsigned blocks = (unsigned)sblocks;
    void* dstat = nullptr;
    if ((st = be.ensure(WS_BD_STAT, BD_WORDS * 4, &dstat, 0))) return st;
    unsigned* stat = (unsigned*)dstat;
    unsigned h[BD_WORDS] = {};
    for (int ax = 0; ax < 3; ++ax) h[BD_MIN + ax] = 0xffffffffu;
    h[BD_CROWDED] = 0xffffffffu;
    if ((st = be.to_device(stat, h, sizeof h))) return st;
    if ((st = be.launch(k_bond_bounds, dim3(blocks < 1024u ? blocks : 1024u), dim3(BD_THREADS), (const float*)src, n2, stat))) return st;
    if ((st = be.to_host(h, stat, sizeof h))) return st;
    if (h[BD_NONFINITE]) { R.left = "a source coordinate is not finite"; return pairs(); }
    BondGrid g;
    float mn[3], mx[3];
    for (int ax = 0; ax < 3; ++ax) { mn[ax] = bond_unkey(h[BD_MIN + ax]); mx[ax] = bond_unkey(h[BD_MAX + ax]); g.mn[ax] = mn[ax]; }
    std::string grid_err;
    if (clash_grid(mn, mx, (double)P.acut, 4e6, R.boxes, &R.side, grid_err)) { R.left = "no grid"; return pairs(); }
    g.nx = (int)R.boxes[0]; g.ny = (int)R.boxes[1]; g.nz = (int)R.boxes[2];
    g.pd = (float)R.side;
    g.cutoff2 = 0.0f;                                                                            // (the bond pair test's: not used here)
    const size_t nb = (size_t)R.boxes[0] * (size_t)R.boxes[1] * (size_t)R.boxes[2];
    if (nb <= 1) { R.left = "the grid is one box"; return pairs(); }
    void *box_cnt, *box_low, *atom_box, *wa, *wb, *start, *tmp, *order, *rec;
    if ((st = be.ensure(WS_BD_BOXCNT, nb * 4, &box_cnt, 0)) || (st = be.ensure(WS_BD_BOXLOW, nb * 4, &box_low, 0)) ||
        (st = be.ensure(WS_BD_ATOMBOX, M * 4, &atom_box, 0)) || (st = be.ensure(WS_BD_A, M * 4, &wa, 0)) ||
        (st = be.ensure(WS_BD_B, (M + 1) * 4, &wb, 0)) || (st = be.ensure(WS_BD_START, (M + 1) * 4, &start, 0)) ||
        (st = be.ensure(WS_BD_TMP, M * 4, &tmp, 0)) || (st = be.ensure(WS_BD_ORDER, M * 4, &order, 0)) || (st = be.ensure(WS_WI_REC, M * 16, &rec, 0)))
        return st;
    if ((st = be.fill(box_cnt, 0, nb * 4)) || (st = be.fill(box_low, 0xff, nb * 4))) return st;
    const dim3 grid(blocks), bblock(BD_THREADS);
    if ((st = be.launch(k_bond_cells, grid, bblock, (const float*)src, n2, g, (unsigned*)atom_box, (unsigned*)box_cnt, (unsigned*)box_low))) return st;
    if ((st = be.launch(k_bond_flags, grid, bblock, n2, (const unsigned*)atom_box, (const unsigned*)box_low, (unsigned*)wa))) return st;
    if ((st = bond_scan(be, (unsigned*)wa, M, (unsigned*)wb))) return st;                        // wb: the ranks; wa is zero again
    if ((st = be.launch(k_bond_ranks, grid, bblock, n2, (const unsigned*)atom_box, (const unsigned*)wb, (const unsigned*)box_cnt, (unsigned*)box_low,
                        (unsigned*)wa, stat)))
        return st;
    if ((st = be.to_host(h, stat, sizeof h))) return st;
    R.max_occ = h[BD_MAXOCC];
    const size_t NB = h[BD_NBOXES];                                                              // occupied boxes, 1 <= NB <= M
    if (NB == 0 || NB > M) { err = "internal: the cell list lost its boxes"; return ST_EHIP; }
    if (R.max_occ > BOND_BOX_CAP) { R.left = "a box holds more sources than the cap"; return pairs(); }
    if ((st = bond_scan(be, (unsigned*)wa, NB, (unsigned*)start))) return st;                    // the boxes' starts by rank
    if ((st = be.launch(k_bond_scatter, grid, bblock, n2, (const unsigned*)atom_box, (const unsigned*)box_low, (const unsigned*)start, (unsigned*)box_cnt,
                        (unsigned*)tmp)))
        return st;
    if ((st = be.launch(k_bond_sort, grid, bblock, n2, (const unsigned*)atom_box, (const unsigned*)box_low, (const unsigned*)start, (const unsigned*)tmp,
                        (unsigned*)order)))
        return st;
    if ((st = be.launch(k_within_pack, grid, dim3(WI_THREADS), n2, (const unsigned*)order, (const float*)src, (float4*)rec))) return st;
    R.cells = 1;
    be.note_dist_kernel("mkamd::k_within_cells");
    return be.launch(k_within_cells, dim3((unsigned)qblocks), dim3(WI_THREADS), a.coords, N, a.sel1, n1, (const float4*)rec, g, (const unsigned*)box_low,
                     (const unsigned*)start, a.gate, (const unsigned*)box, P, a.out);
}

}  // namespace mkamd
