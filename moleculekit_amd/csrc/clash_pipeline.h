// clash_pipeline.h -- launch plan of the steric-clash kernels (clash_kernels.h), written against the backend concept of pipeline.h so
// that the product (capi.hip) and the test emulator (tests/emu/emu_clashes.cpp) run the same plan.
//
// select -> scan -> the number of selected atoms reaches the host -> compact -> the bond guesser's cell list over them (bounds -> the
// host fixes the grid -> cells -> flags -> scan -> ranks -> scan -> the cap -> scatter -> sort) -> pack -> scan -> the number of owners
// reaches the host (the choice of the pair kernels) -> owners -> pair count -> scan -> the total reaches the host, which sizes the
// lists -> pair fill.  Five round trips: the call is not asynchronous.  The rows leave in the fill's order; the caller sorts them.
// Workspace: the bond guesser's (two words per box, seven per selected atom) plus twelve words per selected atom, the lists apart.
#pragma once
#include "bond_pipeline.h"
#include "clash_kernels.h"

#include <algorithm>

namespace mkamd {

enum { CLASH_AVOID_THREAD = 1, CLASH_AVOID_WAVE = 2 };  // `avoid`: the tests walk both lane assignments over the same shapes
// MEASURED (tools/bench_clashes.py, the plan sweep): with few owners a thread per owner leaves most CUs without a
// wave, and the wave-per-owner kernels are faster up to 8 192 owners (a tie there) and slower from 16 384 on; above the count they
// take the call only where a box fills a wave's lanes
constexpr long long CLASH_WAVE_UPTO = 8192;
constexpr unsigned CLASH_WAVE_FROM = WAVE;

struct ClashArgs {
    const float* coords = nullptr;         // device float32 [n][3]
    const float* radii = nullptr;          // device float32 [n]
    const unsigned* sel1 = nullptr;        // device uint32 [n]: != 0 in the first selection
    const unsigned* sel2 = nullptr;        // device uint32 [n]: != 0 in the second (not read in self mode)
    long long n = 0;
    int self_mode = 0;
    const unsigned* ex_start = nullptr;    // device uint32 [n + 1], or NULL: no exclusions
    const unsigned* ex_partner = nullptr;  // device uint32 [ex_start[n]], every row ascending
    double overlap = 0.6, cutoff = 0.0, max_boxes = 4e6;
};

struct ClashResult {
    long long n_pairs = 0;
    const int* pairs = nullptr;            // device int32 [n_pairs][2], the backend's WS_CL_PAIRS
    const float* dists = nullptr;          // device float32 [n_pairs], WS_CL_DIST
    const float* overs = nullptr;          // device float32 [n_pairs], WS_CL_OVER
    long long boxes[3] = {0, 0, 0};        // the grid the call settled on
    double side = 0.0;
    unsigned max_occ = 0;                  // atoms of the most crowded box
    long long n_selected = 0, n_owners = 0;
};

// The box side: at least |cutoff| (the reference's kd-tree squares its radius, so a negative cutoff searches like its absolute value),
// widened by a margin that covers the float32 box arithmetic.  Two atoms no further apart than |cutoff| along an axis must land in
// the same or in adjacent boxes: their quotients (x - min) / side carry a relative error of 2^-23 each, so with q boxes along the axis
// the computed quotients differ by at most |cutoff| / side + q 2^-22, which has to stay <= 1: side >= |cutoff| (1 + margin) with
// margin >= q 2^-21 does it with room.  The margin starts at 2^-10 (good for 2 048 boxes an axis) and grows with the grid.  A side
// below 1 A buys nothing (no radius sum is that small) and costs boxes.
inline int clash_grid(const float (&mn)[3], const float (&mx)[3], double cutoff, double max_boxes, long long (&boxes)[3], double* side, std::string& err)
{
    if (!std::isfinite(cutoff)) { err = "cutoff must be finite"; return ST_EINVAL; }
    const double base = std::fabs(cutoff) > 1.0 ? std::fabs(cutoff) : 1.0;
    double margin = 1.0 / 1024.0;
    for (int round = 0; round < 64; ++round) {
        int st = bond_grid(mn, mx, base * (1.0 + margin), max_boxes, 1.26, boxes, side, err);
        if (st) return st;
        const long long q = std::max(boxes[0], std::max(boxes[1], boxes[2]));
        const double need = (double)q / 2097152.0;
        if (need <= margin) return ST_OK;
        margin = need;
    }
    err = "cutoff: no box side covers the float32 box arithmetic";
    return ST_EINVAL;
}

// The lists are the backend's WS_CL_PAIRS / WS_CL_DIST / WS_CL_OVER buffers: valid until the next clash call on it.
template <class BE>
int run_find_clashes(BE& be, const ClashArgs& a, ClashResult& R, std::string& err, int avoid = 0)
{
    R = ClashResult{};
    const long long n = a.n;
    if (n < 0) { err = "negative size"; return ST_EINVAL; }
    if (n >= 0x80000000LL) { err = "too many atoms (>= 2^31)"; return ST_EINVAL; }
    if (!std::isfinite(a.overlap) || !std::isfinite(a.cutoff)) { err = "overlap and cutoff must be finite"; return ST_EINVAL; }
    if (n == 0) return ST_OK;
    if (!a.coords || !a.radii || !a.sel1 || (!a.self_mode && !a.sel2)) { err = "NULL pointer"; return ST_EINVAL; }
    if ((a.ex_start == nullptr) != (a.ex_partner == nullptr)) { err = "exclusions: both arrays or neither"; return ST_EINVAL; }
    int st;
    char buf[256];
    const size_t N = (size_t)n;
    const dim3 block(CL_THREADS);
    const dim3 ngrid((unsigned)((N + CL_THREADS - 1) / CL_THREADS));
    unsigned word = 0;

    // the atoms of either selection, compacted
    void *flag, *pos;
    if ((st = be.ensure(WS_CL_FLAG, N * 4, &flag, 0)) || (st = be.ensure(WS_CL_POS, (N + 1) * 4, &pos, 0))) return st;
    if ((st = be.launch(k_clash_select, ngrid, block, a.sel1, a.sel2, a.self_mode, n, (unsigned*)flag))) return st;
    if ((st = bond_scan(be, (unsigned*)flag, N, (unsigned*)pos))) return st;
    if ((st = be.to_host(&word, (const unsigned*)pos + N, 4))) return st;
    const size_t M = word;                                                                       // selected atoms
    if (M > N) { err = "internal: the selection scan overran"; return ST_EHIP; }
    R.n_selected = (long long)M;
    if (M == 0) return ST_OK;
    void *sub_coords, *sub_atom;
    if ((st = be.ensure(WS_CL_SUBCOORDS, M * 12, &sub_coords, 0)) || (st = be.ensure(WS_CL_SUBATOM, M * 4, &sub_atom, 0))) return st;
    if ((st = be.launch(k_clash_compact, ngrid, block, a.coords, n, (const unsigned*)pos, (float*)sub_coords, (unsigned*)sub_atom))) return st;

    // the bond guesser's cell list over them (bond_pipeline.h: run_guess_bonds), the box side from the clash cutoff
    const long long m = (long long)M;
    const unsigned blocks = (unsigned)((M + BD_THREADS - 1) / BD_THREADS);
    void* dstat = nullptr;
    if ((st = be.ensure(WS_BD_STAT, BD_WORDS * 4, &dstat, 0))) return st;
    unsigned* stat = (unsigned*)dstat;
    unsigned h[BD_WORDS] = {};
    for (int ax = 0; ax < 3; ++ax) h[BD_MIN + ax] = 0xffffffffu;
    h[BD_CROWDED] = 0xffffffffu;
    if ((st = be.to_device(stat, h, sizeof h))) return st;
    if ((st = be.launch(k_bond_bounds, dim3(blocks < 1024u ? blocks : 1024u), dim3(BD_THREADS), (const float*)sub_coords, m, stat))) return st;
    if ((st = be.to_host(h, stat, sizeof h))) return st;
    if (h[BD_NONFINITE]) { err = "non-finite coordinates (NaN or inf) in the selections: coordinates must be finite"; return ST_EINVAL; }
    BondGrid g;
    float mn[3], mx[3];
    for (int ax = 0; ax < 3; ++ax) { mn[ax] = bond_unkey(h[BD_MIN + ax]); mx[ax] = bond_unkey(h[BD_MAX + ax]); g.mn[ax] = mn[ax]; }
    if ((st = clash_grid(mn, mx, a.cutoff, a.max_boxes, R.boxes, &R.side, err))) return st;
    g.nx = (int)R.boxes[0]; g.ny = (int)R.boxes[1]; g.nz = (int)R.boxes[2];
    g.pd = (float)R.side;
    g.cutoff2 = 0.0f;                                                                            // (the bond pair test's: not used here)
    const size_t nb = (size_t)R.boxes[0] * (size_t)R.boxes[1] * (size_t)R.boxes[2];              // <= 2^28
    void *box_cnt, *box_low, *atom_box, *wa, *wb, *start, *tmp, *order;
    if ((st = be.ensure(WS_BD_BOXCNT, nb * 4, &box_cnt, 0)) || (st = be.ensure(WS_BD_BOXLOW, nb * 4, &box_low, 0)) ||
        (st = be.ensure(WS_BD_ATOMBOX, M * 4, &atom_box, 0)) || (st = be.ensure(WS_BD_A, M * 4, &wa, 0)) ||
        (st = be.ensure(WS_BD_B, (M + 1) * 4, &wb, 0)) || (st = be.ensure(WS_BD_START, (M + 1) * 4, &start, 0)) ||
        (st = be.ensure(WS_BD_TMP, M * 4, &tmp, 0)) || (st = be.ensure(WS_BD_ORDER, M * 4, &order, 0)))
        return st;
    if ((st = be.fill(box_cnt, 0, nb * 4)) || (st = be.fill(box_low, 0xff, nb * 4))) return st;
    const dim3 grid(blocks), bblock(BD_THREADS);
    if ((st = be.launch(k_bond_cells, grid, bblock, (const float*)sub_coords, m, g, (unsigned*)atom_box, (unsigned*)box_cnt, (unsigned*)box_low))) return st;
    if ((st = be.launch(k_bond_flags, grid, bblock, m, (const unsigned*)atom_box, (const unsigned*)box_low, (unsigned*)wa))) return st;
    if ((st = bond_scan(be, (unsigned*)wa, M, (unsigned*)wb))) return st;                        // wb: the ranks; wa is zero again
    if ((st = be.launch(k_bond_ranks, grid, bblock, m, (const unsigned*)atom_box, (const unsigned*)wb, (const unsigned*)box_cnt, (unsigned*)box_low,
                        (unsigned*)wa, stat)))
        return st;
    if ((st = be.to_host(h, stat, sizeof h))) return st;
    R.max_occ = h[BD_MAXOCC];
    const size_t NB = h[BD_NBOXES];                                                              // occupied boxes, 1 <= NB <= M
    if (NB == 0 || NB > M) { err = "internal: the cell list lost its boxes"; return ST_EHIP; }
    if (R.max_occ > BOND_BOX_CAP) {
        const unsigned b = h[BD_CROWDED], per = (unsigned)(g.nx * g.ny);
        snprintf(buf, sizeof buf, "crowded box: box %u (x %u, y %u, z %u of %d x %d x %d, side %.6g) holds %u atoms, more than the %u a box may hold",
                 b, b % per % (unsigned)g.nx, b % per / (unsigned)g.nx, b / per, g.nx, g.ny, g.nz, R.side, R.max_occ, BOND_BOX_CAP);
        err = buf;
        return ST_EINVAL;
    }
    if ((st = bond_scan(be, (unsigned*)wa, NB, (unsigned*)start))) return st;                    // the boxes' starts by rank; wa is zero again
    if ((st = be.launch(k_bond_scatter, grid, bblock, m, (const unsigned*)atom_box, (const unsigned*)box_low, (const unsigned*)start, (unsigned*)box_cnt,
                        (unsigned*)tmp)))
        return st;
    if ((st = be.launch(k_bond_sort, grid, bblock, m, (const unsigned*)atom_box, (const unsigned*)box_low, (const unsigned*)start, (const unsigned*)tmp,
                        (unsigned*)order)))
        return st;

    // the cell-ordered records and the owners
    void *rec, *idx, *bits, *box, *owner;
    if ((st = be.ensure(WS_CL_REC, M * 16, &rec, 0)) || (st = be.ensure(WS_CL_IDX, M * 4, &idx, 0)) || (st = be.ensure(WS_CL_BITS, M * 4, &bits, 0)) ||
        (st = be.ensure(WS_CL_BOX, M * 4, &box, 0)) || (st = be.ensure(WS_CL_OWNER, M * 4, &owner, 0)))
        return st;
    if ((st = be.launch(k_clash_pack, grid, block, m, (const unsigned*)order, (const float*)sub_coords, (const unsigned*)sub_atom, (const unsigned*)atom_box,
                        a.radii, a.sel1, a.sel2, a.self_mode, (float4*)rec, (unsigned*)idx, (unsigned*)bits, (unsigned*)box, (unsigned*)wa)))
        return st;
    if ((st = bond_scan(be, (unsigned*)wa, M, (unsigned*)wb))) return st;                        // wb: the owners' numbers; wa is zero again
    if ((st = be.to_host(&word, (const unsigned*)wb + M, 4))) return st;
    const size_t K = word;                                                                       // owners
    if (K > M) { err = "internal: the owner scan overran"; return ST_EHIP; }
    R.n_owners = (long long)K;
    if (K == 0) return ST_OK;
    if ((st = be.launch(k_clash_owners, grid, block, m, (const unsigned*)wb, (unsigned*)owner))) return st;

    // pairs: count -> scan -> fill
    const bool wave = (avoid & CLASH_AVOID_THREAD) ||
                      (!(avoid & CLASH_AVOID_WAVE) && ((long long)K <= CLASH_WAVE_UPTO || R.max_occ >= CLASH_WAVE_FROM));
    be.note_dist_kernel(wave ? "mkamd::k_clash_pairs_wave" : "mkamd::k_clash_pairs_thread");
    const dim3 pgrid((unsigned)(wave ? (K + 3) / 4 : (K + CL_THREADS - 1) / CL_THREADS));
    ClashParams P;
    P.overlap = (float)a.overlap;
    P.cutoff2 = a.cutoff * a.cutoff;
    P.self_mode = a.self_mode;
    unsigned long long* total = (unsigned long long*)(stat + BD_TOTAL);
    auto pairs = [&](auto kern, int* op, float* od, float* oo) {
        return be.launch(kern, pgrid, block, (const float4*)rec, (const unsigned*)idx, (const unsigned*)bits, (const unsigned*)box, (const unsigned*)owner,
                         (long long)K, g, P, (const unsigned*)box_low, (const unsigned*)start, a.ex_start, a.ex_partner, (unsigned*)wa, (const unsigned*)wb,
                         total, op, od, oo);
    };
    if ((st = wave ? pairs(k_clash_pairs_wave<false>, nullptr, nullptr, nullptr) : pairs(k_clash_pairs_thread<false>, nullptr, nullptr, nullptr))) return st;
    if ((st = be.to_host(h, stat, sizeof h))) return st;
    unsigned long long found;
    memcpy(&found, h + BD_TOTAL, 8);
    if (found > 0x7fffffffull) { err = "more than 2^31 clashes: the coordinates are not a molecule's"; return ST_EINVAL; }
    if (found == 0) return ST_OK;
    if ((st = bond_scan(be, (unsigned*)wa, K, (unsigned*)wb))) return st;                        // wb: every owner's first row
    void *op, *od, *oo;
    if ((st = be.ensure(WS_CL_PAIRS, (size_t)found * 8, &op, 0)) || (st = be.ensure(WS_CL_DIST, (size_t)found * 4, &od, 0)) ||
        (st = be.ensure(WS_CL_OVER, (size_t)found * 4, &oo, 0)))
        return st;
    if ((st = wave ? pairs(k_clash_pairs_wave<true>, (int*)op, (float*)od, (float*)oo) : pairs(k_clash_pairs_thread<true>, (int*)op, (float*)od, (float*)oo)))
        return st;
    R.n_pairs = (long long)found;
    R.pairs = (const int*)op;
    R.dists = (const float*)od;
    R.overs = (const float*)oo;
    return ST_OK;
}

}  // namespace mkamd
