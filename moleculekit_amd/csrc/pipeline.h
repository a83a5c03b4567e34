// pipeline.h -- host-side planning and launch sequences for the kernels in kernels.h.
//
// Written against a small "backend" concept so the exact same planning / launch code drives
//   * the HIP backend in capi.hip (the product: MI355X, one stream per context), and
//   * the host-thread SIMT emulation under tests/emu (test infrastructure, CPU-only boxes).
//
// Backend concept:
//   int  ensure(int slot, size_t bytes, void** ptr)     grow-only workspace buffer
//   int  fill(void* p, int byte, size_t bytes)          async memset on the stream
//   bool pipelining_possible()                           big calls may run their pre-pass beside the previous call's tile kernel
//   int  launch(kernel, dim3 grid, dim3 block, args...) async launch on the stream
//   void hot_begin() / hot_end()                        bracket the tile kernel (event timing)
//   int  acquire_set(bool pipelined)                    pick a workspace set (double-buffered); when
//                                                       pipelined, following launches go to an internal
//                                                       stream that may run beside the previous call's
//                                                       tile kernel
//   void prepass_done(int set)                          back to the caller's stream, which waits for the pre-pass
//   void tile_done(int set)                             the set may be reused once the tile kernel has finished
// ensure() takes the workspace set as its last argument.
#pragma once
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <cstdlib>
#include <type_traits>

namespace mkamd {

constexpr int SOLO_CNT_SHIFT = 3;   // k_bin_solo's cell counters 32 bytes apart (GridDesc::cnt_shift); 16 and 128 bytes measured the same

enum Status { ST_OK = 0, ST_EINVAL = 1, ST_EHIP = 2, ST_ENODEV = 3, ST_EOVERFLOW = 4, ST_EBOX = 5 };

enum WsSlot {
    WS_CELL_COUNT = 0, WS_CELL_START, WS_SCAN_CHUNKS, WS_REC_POS, WS_REC_W, WS_REC_CLS, WS_CLS_TABLE, WS_CLS_BLOCKS, WS_CLS_L1, WS_TMP_POS, WS_TMP_IDX, WS_TMP_CLS, WS_DENSE_LIST, WS_ERR, WS_W_EXPLICIT, WS_DENSE_WORDS, WS_DIRECT_COUNT, WS_REDO_LIST,
    // staging for the "_host" entry points
    WS_H_COORDS, WS_H_SIGMAS, WS_H_OFFSETS, WS_H_ORIGINS, WS_H_BOX, WS_H_OUT, WS_H_CENTERS, WS_H_STAGE,
    // distance_utils row (dist_pipeline.h)
    WS_D_PA, WS_D_PB, WS_D_WRAP, WS_D_COM1, WS_D_COM2, WS_D_SEL1, WS_D_SEL2, WS_D_CHAINS, WS_D_CHAINS2, WS_D_G1A, WS_D_G1O,
    WS_D_G2A, WS_D_G2O, WS_D_MASS, WS_D_CNT, WS_D_TOT, WS_D_BASE, WS_D_CONTACTS, WS_D_MASK,
    // alignment (align_pipeline.h) and its host entry point
    WS_A_REFPART, WS_A_PART, WS_A_RPART, WS_A_FOLD, WS_A_REFFOLD, WS_A_SLAB, WS_A_XYZ, WS_A_REF, WS_A_SEL, WS_A_REFSEL, WS_A_FRAMES, WS_A_AFFINE,
    // surface area (sasa_pipeline.h) and its host entry point
    WS_S_POINTS, WS_S_PACK, WS_S_AREA, WS_S_ERR, WS_S_SLAB, WS_S_XYZ, WS_S_RADII, WS_S_MAP, WS_S_MASK, WS_S_OUT,
    // group moments (moments_pipeline.h) and their host entry points
    WS_M_PART, WS_M_REF, WS_M_ATOMS, WS_M_OFFS, WS_M_W, WS_M_REFIN,
    // periodic wrap (wrap_pipeline.h) and its host entry point
    WS_W_CENTRE, WS_W_STARTS, WS_W_LARGE, WS_W_SEL,
    // ... of triclinic boxes (wrap_cell_pipeline.h): the frames' records; the host entry point's box vectors and status words
    WS_W_CELL, WS_W_BOXV, WS_W_STATUS,
    // ring interactions (ring_pipeline.h): the chunk's ring / partner records, masks, counters; the two context-owned result lists; the
    // host entry point's lists and the second half of a chunk on its way down
    WS_R_REC, WS_R_PART, WS_R_MASK, WS_R_CNT, WS_R_TOT, WS_R_BASE, WS_R_PAIRS, WS_R_DISTANG, WS_R_ATOMS, WS_R_STARTS1, WS_R_STARTS2, WS_R_PARTNERS,
    WS_R_EMIT, WS_R_OUT2,
    // hydrogen bonds (hbond_pipeline.h): the call's table (rows, sublists, tile numbering); the chunk's masks and counters; the context-owned list
    WS_HB_TABLE, WS_HB_MASK, WS_HB_CNT, WS_HB_TOT, WS_HB_BASE, WS_HB_TRIPLES,
    // bond guesser (bond_pipeline.h): status words; its scans' chunk sums; two words per box; the per-atom arrays; the context-owned list
    WS_BD_STAT, WS_BD_CHUNKS, WS_BD_BOXCNT, WS_BD_BOXLOW, WS_BD_ATOMBOX, WS_BD_A, WS_BD_B, WS_BD_START, WS_BD_TMP, WS_BD_ORDER, WS_BD_PAIRS,
    // steric clashes (clash_pipeline.h; the cell list is the bond guesser's and uses its slots, WS_BD_PAIRS apart): the selection's flags
    // and numbering; the selected atoms' coordinates and indices; the cell-ordered records; the owners; the three context-owned lists
    WS_CL_FLAG, WS_CL_POS, WS_CL_SUBCOORDS, WS_CL_SUBATOM, WS_CL_REC, WS_CL_IDX, WS_CL_BITS, WS_CL_BOX, WS_CL_OWNER, WS_CL_PAIRS, WS_CL_DIST, WS_CL_OVER,
    // proximity selections (within_pipeline.h; the cell list is the bond guesser's and uses its slots): the compacted sources, their
    // bounding boxes per frame, the cell-ordered source records; the host entry point's frame-major coordinates and gate bounds
    WS_WI_SRC, WS_WI_BOX, WS_WI_REC, WS_WI_XYZ, WS_WI_GATE,
    // secondary structure (dssp_pipeline.h): the chain runs, the chunk's arrays; the host entry point's per-residue arrays
    WS_SS_SEG, WS_SS_WORK, WS_SS_NCO, WS_SS_PROLINE,
    WS_NSLOTS
};

constexpr double CUTOFF_A = 5.0;            // occupancy_utils.pyx:53 (d^2 < 25)

// A molecule's topology (round 5; kernels.h "Topology"): everything the pre-pass derives from the sigmas alone, on the device.
// Built once (run_topology_build); a lattice call that brings it voxelizes items that are each ONE set of coordinates of that
// molecule -- the frames of a trajectory -- without touching sigmas, classes or table look-ups again.
struct TopologyDev {
    long long n = 0;                        // atoms of the molecule
    int C = 0, G = 0, sigmas_f64 = 0;
    double voxelsize = 0.0;                 // w = voxelsize^2 / sigma^2: the handle is for one voxel size
    const unsigned* ids = nullptr;          // [n, G] class ids (8 x 4 bits per word)
    const uint2* cw = nullptr;              // [n, G] compact channel words (what k_tail's fix-up waves look at first)
    const void* sigmas = nullptr;           // [n, C] the library's own copy (the exact fix-up recomputes from it)
    const unsigned* table = nullptr;        // [CLS_TABLE_WORDS] the class table
    bool overflow = false;                  // more than NCLS distinct sigmas: no class ids (creation reports it, calls are refused)
    bool wide = false;                      // some sigma is wide enough for the exact cut-off fix-up (GridDesc::w_exact_max)
    const unsigned* wide_list = nullptr;    // [n_wide] the atoms that have one, ascending (k_tail's fix-up jobs of a topology call: item x wide atom)
    unsigned n_wide = 0;
    // A BATCH handle (round 7): the same contents built over ALL atoms of a resident, ragged batch of different molecules -- n atoms
    // in n_items items -- and indexed by an atom's position in that batch.  A call is a contiguous range of its items
    // (LatticeProblem::topo_first_item); wide_list then holds batch-wide atom indices.
    bool batch = false;
    int n_items = 0;
    const long long* offsets = nullptr;     // [n_items + 1] the atom offsets the handle was built for, on the device (the binning checks the call's against them)
    const long long* h_offsets = nullptr;   // the same on the host (a call's range: its first atom, its atom count)
    const unsigned* h_wide_list = nullptr;  // wide_list on the host (the wide atoms inside a call's range)
    long long max_item = 0;                 // atoms of the longest item (k_exact_redo's slices)
    // cover fold (round 8): the build's violated-class words, [G] on the device (GridDesc::cover_violated; nullptr: a handle built
    // without them -- no fold), and what the host keeps of them: cover[g] = ~violated[g] & 0xfffe, the classes channel 7 of group g
    // covers.  A property of the handle's atoms, so it holds for any item range of a batch handle.
    const unsigned* cover_violated = nullptr;
    const unsigned* h_cover = nullptr;
};

struct LatticeProblem {
    int B = 0;
    long long total_atoms = 0;
    int C = 0;
    int sigmas_f64 = 0;
    int nvox[3] = {0, 0, 0};
    double voxelsize = 1.0;
    int pbc = 0;
    int max_images = 1;
    int tile_k = 0;                         // 0 = auto
    int force_general = 0;                  // 1 = never use the class-sorted path
    int lds_tier = -1;                      // -1 = adaptive (choose_tier), else the ECAP_TIER index to use
    int prepass_mode = -1;                  // -1 = automatic, 0 = multi-kernel chain, 1 = one-launch per-item pre-pass (if it fits)
    int fine_cells = 0;                     // 1 = half-cutoff cells (A-B benchmarking, see plan_lattice)
    double value_tol = 0.0;                 // > 0: entries may be dropped where they are worth less than this (tolerance-aware reach)
    int direct = -1;                        // direct binning (k_bin_direct): 1 = whenever the geometry allows; -1 (automatic) and 0 = the chain
    int cell_cap = 0;                       // record slots per cell of the direct layout (0 = 128; tests shrink it to see cells spill)
    unsigned spill_cap = 0;                 // slots of an item's spill area in the direct layout (0 = max(1024, an eighth of the average item))
    unsigned seq = 0;                       // != 0: k_tail reports this number in the host-visible feedback words as it starts (FB_TILES_DONE)
    int tile_team = -1;                     // -1 = automatic (a team of waves per tile when the launch is tiny), 0 = never, 1 = always (4, 8, 16: with that many waves)
    int tile_items = -1;                    // -1 = automatic (a workgroup per item for batches of ligand-sized items), 0 = never, 1 = always
    int cover_fold = 0;                     // 0 = a call that bins through a handle folds covered channels (GridDesc::cover_violated), -1 = never (A-B, tests)
    int exact_redo_list = 0;                // 0 = a topology call with wide atoms hands its exact cut-off hits to k_exact_redo, -1 = k_tail recomputes them in place;
                                            // n > 0 (tests): as 0 with a list of n hits
    // device pointers
    const float* coords = nullptr;
    const long long* atom_offsets = nullptr;
    const void* sigmas = nullptr;
    const double* origins = nullptr;
    const float* box = nullptr;
    const double* affine = nullptr;        // optional [B,12]: rotation (row-major 3x3) + translation per item
    float* out = nullptr;
    const TopologyDev* topo = nullptr;      // every item is topo->n atoms of that molecule (checked on the device: MK_ERR_TOPOLOGY)
    int topo_first_item = 0;                // a batch handle: the call is its items [topo_first_item, + B) (checked on the device too)
};

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// Fill the GridDesc for a batch; returns ST_OK or ST_EINVAL with a message.
inline int plan_lattice(const LatticeProblem& P, GridDesc& g, std::string& err)
{
    char buf[256];
    if (P.B < 0 || P.total_atoms < 0 || P.C <= 0) { err = "n_items/total_atoms must be >= 0 and n_channels > 0"; return ST_EINVAL; }
    if (!(P.voxelsize > 0.0) || !std::isfinite(P.voxelsize)) { err = "voxelsize must be a positive finite number"; return ST_EINVAL; }
    for (int ax = 0; ax < 3; ++ax)
        if (P.nvox[ax] < 0) { err = "nvoxels must be >= 0"; return ST_EINVAL; }
    g = GridDesc{};
    g.nx = P.nvox[0]; g.ny = P.nvox[1]; g.nz = P.nvox[2];
    g.V = (long long)g.nx * g.ny * g.nz;
    g.C = P.C; g.G = ceil_div(P.C, CHG);
    g.B = P.B; g.pbc = P.pbc ? 1 : 0; g.force_general = P.force_general ? 1 : 0;
    g.inv_res = 1.0 / P.voxelsize;
    g.w_scale = P.voxelsize * P.voxelsize;
    const double R = CUTOFF_A / P.voxelsize;                 // cutoff in voxel units
    g.R2 = (float)(R * R);
    g.R2cull = (float)(R * R * 1.0002 + 1e-3);
    g.res = P.voxelsize;
    // value step at the cutoff = 1-exp(-(1/(R2 w))^6) > 5e-6  <=>  R2 w < (5e-6)^(-1/6) = 7.647  (sigma > 1.81 A)
    g.w_exact_max = (float)(7.647 / (R * R));
    // 1 - exp(-t^-6) < eps beyond t = w d^2 = eps^(-1/6); off (0) unless the caller opted in.  Capped at 1e-5: the parity bound
    g.cell_cap = 0; g.spill_base = 0u; g.spill_cap = 0u; g.direct_words = nullptr; g.cnt_shift = 0;
    g.reach_tau = (P.value_tol > 0.0) ? (float)std::pow(std::min(P.value_tol, 1e-5), -1.0 / 6.0) : 0.f;
    g.Rp = R + 1e-3;
    g.rint = (int)std::ceil(R);
    if (g.rint > 512) { err = "voxelsize too small (cutoff spans > 512 voxels)"; return ST_EINVAL; }
    // cell edge: the power of two >= the cutoff radius in voxels (1 A grid: 8), so that a tile looks at <= 3 x 3 x 3 cells.
    // `fine_cells` halves it (<= 7 x 7 cell columns, one per lane): the candidates of a tile then hug its rounded box
    // better (at 1 A 7 200 A^3 instead of 27 x 8^3 = 13 824 A^3, against the 3 986 A^3 that survive the exact cull) --
    // measured round 2: VALU instructions of the tile kernel -2.4 %, scalar ones +10 %, time +1.5 % on cfg2 and +5 % on
    // cfg3 (eight times the cell counters), so it is not the default
    g.cs_log2 = 3;
    while ((1 << g.cs_log2) < g.rint && g.cs_log2 < 9) ++g.cs_log2;
    if (g.cs_log2 > 2 && P.fine_cells) --g.cs_log2;
    g.cs = 1 << g.cs_log2;
    g.h = ceil_div((long long)g.rint + 1, g.cs);
    g.ncx = ceil_div(g.nx, g.cs) + 2 * g.h;
    g.ncy = ceil_div(g.ny, g.cs) + 2 * g.h;
    g.ncz = ceil_div(g.nz, g.cs) + 2 * g.h;
    if (g.ncx > 1023 || g.ncy > 1023 || g.ncz > 1023) { err = "grid too large (more than 1023 cells per axis)"; return ST_EINVAL; }
    const long long ncell = (long long)g.ncx * g.ncy * g.ncz;
    if ((ncell + 1) * (long long)(P.B > 0 ? P.B : 1) > 0xFFFF0000LL) {
        snprintf(buf, sizeof buf, "batch too large: %lld cells x %d items exceeds 2^32; split the batch", ncell, P.B);
        err = buf; return ST_EINVAL;
    }
    g.ncell = (int)ncell;
    g.cstride = (int)ncell + 1;
    g.cls_per_item = 0;
    g.prepass_hurry = 1;

    // tile depth: K=8 unless the x extent pads badly or the launch would be too small to fill 256 CUs
    int K = P.tile_k;
    if (K != 4 && K != 8) {
        const long long pad8 = (long long)ceil_div(g.nx, 8) * 8, pad4 = (long long)ceil_div(g.nx, 4) * 4;
        const long long tiles8 = (long long)ceil_div(g.nx, 8) * ceil_div(g.ny, 8) * ceil_div(g.nz, 8) * P.B * g.G;
        K = (pad4 < pad8 || tiles8 < 2048) ? 4 : 8;
    }
    g.K = K;
    g.tnx = ceil_div(g.nx, K); g.tny = ceil_div(g.ny, 8); g.tnz = ceil_div(g.nz, 8);
    const long long ntiles = (long long)g.tnx * g.tny * g.tnz;
    if (ntiles * (long long)(P.B > 0 ? P.B : 1) > 0x7FFFFF00LL) { err = "batch too large: more than 2^31 tiles; split the batch"; return ST_EINVAL; }
    g.ntiles = (int)ntiles;

    long long images = 1;
    if (g.pbc) {
        if (P.max_images < 1) { err = "max_images_per_atom must be >= 1 for periodic items"; return ST_EINVAL; }
        images = P.max_images;
    }
    const long long M = P.total_atoms * images;
    if (M > 0xFFFF0000LL) { err = "batch too large: more than 2^32 atom records; split the batch"; return ST_EINVAL; }
    g.M = (unsigned)(M > 0 ? M : 1);
    g.img_cap = (int)images;
    return ST_OK;
}

// upper bound on periodic images of one atom inside grid+halo, from host-known boxes [B,3] (A)
inline int max_images_from_boxes(const float* box, int B, const int* nvox, double voxelsize, std::string& err)
{
    long long worst = 1;
    for (int b = 0; b < B; ++b) {
        long long m = 1;
        for (int ax = 0; ax < 3; ++ax) {
            const double L = (double)box[3 * b + ax];
            if (!(L > 2.0 * CUTOFF_A)) { err = "periodic box edges must be > 10 A (2 x cutoff)"; return -1; }
            const double span = (double)(nvox[ax] > 0 ? nvox[ax] - 1 : 0) * voxelsize + 2.0 * CUTOFF_A + 2e-3 * voxelsize;
            m *= (long long)std::floor(span / L) + 1;
        }
        if (m > worst) worst = m;
    }
    if (worst > 4096) { err = "periodic box much smaller than the grid (more than 4096 images per atom)"; return -1; }
    return (int)worst;
}

template <class BE>
int run_scan(BE& be, unsigned* counts /* cleared by the last kernel */, size_t n, unsigned* starts /* n+1 */, int set = 0)
{
    const size_t nchunks = (n + 1 + SCAN_CHUNK - 1) / SCAN_CHUNK;
    void* chunks = nullptr;
    int st = be.ensure(WS_SCAN_CHUNKS, nchunks * sizeof(unsigned), &chunks, set);
    if (st) return st;
    if ((st = be.launch(k_scan_chunk_sums, dim3((unsigned)nchunks), dim3(SCAN_THREADS), (const unsigned*)counts, n, (unsigned*)chunks))) return st;
    if ((st = be.launch(k_scan_sums_inplace, dim3(1), dim3(SCAN_THREADS), (unsigned*)chunks, (unsigned)nchunks))) return st;
    return be.launch(k_scan_finish, dim3((unsigned)nchunks), dim3(SCAN_THREADS), counts, n, (const unsigned*)chunks, starts, (const unsigned*)nullptr);
}

// LDS tier of the tile kernel: forced (0..NTIER-1), or the leanest tier that at most 5 % of the tiles of
// the most recent finished call overflowed (feedback = {tiles over tier 0, 1, 2, tiles} written by the
// dense kernel into host-visible memory; stale or zero feedback only costs speed, never correctness:
// all tiers and the dense path produce bit-identical values).
inline int choose_tier(int forced, const volatile unsigned* feedback)
{
    if (forced >= 0) return forced < NTIER ? forced : NTIER - 1;
    if (!feedback) return 0;
    const unsigned tiles = feedback[NTIER];
    if (tiles == 0) return 0;
    int tier = 0;
    while (tier < NTIER - 1 && (unsigned long long)feedback[tier] * 20ull > tiles) ++tier;
    return tier;
}

enum TileFlavour { TILES_PLAIN = 0, TILES_LEAN = 1, TILES_TEAM = 2, TILES_ITEMS = 3 };

constexpr unsigned REDO_BLOCKS = 4096;       // waves of k_exact_redo (they share the jobs)
constexpr unsigned SHELL_BLOCKS = 16384;     // waves of k_exact_shells (they share the (item, wide atom) jobs)
constexpr unsigned REDO_CAP = 32768;         // hits the list holds (1 MB); a call with more walks its shells once more and recomputes in place (k_exact_shells<.., true>)
constexpr unsigned CLS_ROWS_PER_BLOCK = 128;         // per-block sigma sets one workgroup of the first merge takes
constexpr long long PIPELINE_MIN_ATOMS = 200000;     // a call this big may run its pre-pass beside the previous call's tile kernel

// The one float / double switch on the sigmas: `launch` is a generic lambda that takes the typed sigma pointer and names
// its kernel instance with sigma_of<decltype(sig)>, so that every argument list is written once.
template <class Ptr> using sigma_of = std::remove_const_t<std::remove_pointer_t<Ptr>>;
template <class F>
inline int with_sigmas(const void* sigmas, int f64, F&& launch) { return f64 ? launch((const double*)sigmas) : launch((const float*)sigmas); }

// What a backend remembers about the cell-counter buffer of one workspace set (run_lattice): which allocation it is and
// how many of its leading bytes are known to be zero between calls.
// The dense words (dense-tile list length, tier statistics, k_tail's done counter) live in a buffer of their own, in TWO
// copies that alternate from call to call: a call's last launch clears the copy the NEXT call will use.
// dptr / dclean: the same for the counters of the one-launch pre-pass (k_bin_solo; k_tail zeroes them again); tptr: the
// class-table buffer that holds a valid table (k_bin_solo keeps its table across calls: a new buffer starts empty).
struct CounterState { void* ptr = nullptr; size_t clean = 0; void* wptr = nullptr; bool wclean = false; unsigned parity = 0;
                      void* dptr = nullptr; size_t dclean = 0; void* tptr = nullptr; };
constexpr int DENSE_SET_WORDS = DENSE_WORDS + 2;     // + the done counter of k_tail's dense blocks + its role tickets

// Which kernels a lattice call runs: decided once, from the problem and its grid alone (choose_lattice_path), and finished
// once the backend has said whether the call is pipelined (settle_lattice_path).  All paths compute the same bits.
struct LatticePath {
    // the pre-pass: the kernel chain (count -> classes + scan -> fill; with a topology its TOPO binning kernels), the
    // one-launch per-item form (k_prepass_items), or the one-launch form of a small call (k_bin_solo)
    enum PrePass { PRE_CHAIN, PRE_CHAIN_TOPO, PRE_ITEMS, PRE_SOLO } prepass = PRE_CHAIN;
    bool pipelined_wanted = false;          // what acquire_set() is asked
    bool team = false;                      // fewer tile waves than the chip has SIMDs: a team of waves per tile
    bool ligand_items = false;              // ligand-sized items (and the caller has not switched the workgroup-per-item kernel off)
    bool direct_geom = false;               // the geometry allows a direct record layout (k_bin_direct, k_bin_solo):
    int direct_cap = 128; unsigned spill = 0; unsigned long long direct_slots = 0;   // its record slots per cell, spill slots PER ITEM, slots in all
    int team_waves = TILE_TEAM;             // waves per tile of the team kernel
    // the exact cut-off fix-up: its jobs (256-atom blocks, items, or (item, wide atom) pairs of a topology call), k_tail's waves that
    // share them, and k_tail's workgroups for the tiles left behind
    unsigned fix_jobs = 0, fix_waves = 0, dense_wgs = 0;
    bool split_exact_fixup = false;         // k_tail + k_exact_shells + k_exact_redo instead of k_tail alone
    unsigned redo_cap = REDO_CAP;           // hits its list holds
    // settled after acquire_set():
    bool direct_layout = false;             // the records go to the direct layout (PRE_SOLO, or direct_first)
    bool direct_first = false;              // k_bin_direct in front of the chain (then the chain is the fall-back)
    bool small_scan = false;                // the chain's classes + scan in one launch (k_prepass_small) instead of three
    int flavour = TILES_PLAIN;              // TileFlavour

    bool topo() const { return prepass == PRE_CHAIN_TOPO; }
    bool solo() const { return prepass == PRE_SOLO; }
    bool per_item() const { return prepass == PRE_ITEMS; }
};

// The exact cut-off fix-up of the path's pre-pass: its jobs, the waves that share them, and whether they run split in three launches.
inline void choose_exact_fixup(LatticePath& L, const LatticeProblem& P, const GridDesc& g)
{
    const bool topo = L.topo();
    const unsigned topo_jobs = !topo ? 0u : P.topo->batch ? g.topo_wide : (unsigned)((long long)g.B * P.topo->n_wide);
    L.fix_jobs = topo ? topo_jobs : L.per_item() ? (unsigned)g.B : P.total_atoms > 0 ? (unsigned)ceil_div(P.total_atoms, 256) : 0u;
    L.fix_waves = L.fix_jobs < 8192u ? L.fix_jobs : 8192u;         // (the fix-up waves share the jobs: see k_tail)
    // a trajectory of a molecule with wide sigmas (ions): the exact recomputes of k_tail's hits are spread over many waves (k_exact_redo)
    L.split_exact_fixup = topo && topo_jobs != 0u && P.seq == 0u && !g.force_general && P.exact_redo_list >= 0;
}

inline LatticePath choose_lattice_path(const LatticeProblem& P, const GridDesc& g, bool pipelining_possible)
{
    LatticePath L;
    // a frame handle takes the chain whatever the call's size; a BATCH handle is honoured where the plain call would take the chain
    // (and no direct pass: settle_lattice_path) -- a call that goes elsewhere is a plain call on the handle's own sigma copy
    const bool topo = P.topo != nullptr && !P.topo->batch, topo_batch = P.topo != nullptr && P.topo->batch;
    const long long B = g.B;
    // Big batches are software-pipelined across calls: the pre-pass (latency / atomic bound) of this call
    // runs on an internal stream beside the tile kernel (VALU bound) of the previous call, on the other
    // workspace set.  Small calls stay in order on the caller's stream (the hand-over costs ~20 us).
    const bool big = P.total_atoms >= PIPELINE_MIN_ATOMS;
    // (when the call can be pipelined -- the caller opted in and the batch is big -- items of more than ~1 000 atoms go to
    //  the kernel chain: its pre-pass then hides behind the previous call's tile kernel, the one-launch one never does;
    //  cfg1 x 4096 = 1 639 atoms per item: 2.00 -> 1.93 ms per step; 60-atom items lose 4 % that way)
    const bool chain_pays = pipelining_possible && big && P.total_atoms > 1024LL * B;
    const unsigned long long tile_waves = (unsigned long long)g.B * (unsigned)g.ntiles * (unsigned)g.G;
    // fewer tile waves than the chip has SIMDs (one or two 64^3 grids, a pocket): a team of waves per tile --
    // four when that fills the chip (a 64^3 grid: 1 024 tiles), more for fewer tiles (a pocket: 54 tiles of K = 4)
    // (the 3PTB pocket, 54 tiles: 30.0 us per call with 4 waves per tile, 27.8 with 8, 28.3 with 16; a cfg2 grid, 1 024 tiles:
    //  39.9 with 4, 46.6 with 8); 8 and 16 waves: K = 4 only
    L.team = P.tile_team > 0 || (P.tile_team < 0 && tile_waves <= 1024ull);
    if (g.K == 4) L.team_waves = (P.tile_team == 8 || P.tile_team == 16) ? P.tile_team : (P.tile_team != 4 && tile_waves <= 256ull) ? 8 : TILE_TEAM;
    // direct layouts (k_bin_direct, k_bin_solo): open boundaries, one channel group, tiles that see at most 63 cells
    auto span = [&](int width) {                     // most cells a tile of `width` voxels (aligned to it) sees along one axis
        int best = 0;
        for (int x0 = 0; x0 < std::max(g.cs, width); x0 += width)
            best = std::max(best, ((x0 + width - 1 + g.rint) >> g.cs_log2) - ((x0 - g.rint) >> g.cs_log2) + 1);
        return best;
    };
    static const int env_cap = [] { const char* e = std::getenv("MKAMD_CELL_CAP"); return e ? std::atoi(e) : 0; }();     // A-B knob
    L.direct_cap = P.cell_cap > 0 ? P.cell_cap : (env_cap > 0 ? env_cap : 128);
    L.direct_geom = !g.pbc && g.G == 1 && !g.force_general && P.total_atoms > 0 && L.direct_cap <= (1 << SURV_OFF_BITS) &&
                    span(g.K) * span(8) * span(8) <= WAVE - 1;
    // many ligand-sized items (cfg3, cfg5): a workgroup per item sorts its entries once for all its tiles
    L.ligand_items = P.tile_items != 0 && P.total_atoms <= 96LL * B && g.ntiles <= 512;
    const bool hist_fits = g.ncell + 1 <= ITEM_HIST;         // the cell grid within the LDS counters of k_prepass_items
    // a SMALL call (the team regime: one molecule per call) takes the one-launch pre-pass k_bin_solo, unless the caller
    // chose a pre-pass (prepass_mode) or it is a ligand-sized call of the workgroup-per-item tile kernel; direct == 2
    // forces it for any size (tests)
    const bool solo = !topo && L.direct_geom && (unsigned long long)P.total_atoms * (unsigned)g.B <= (1ull << 22) &&
                      (P.direct == 2 || (P.direct != 0 && P.prepass_mode < 0 && L.team && !(L.ligand_items && P.tile_team <= 0 && hist_fits)));
    // small items (up to a few thousand atoms, cell grid within the LDS counters): the one-launch per-item pre-pass
    // (short enough that overlapping it with the previous call's tile kernel does not pay: in order, set 0)
    const bool per_item = !topo && !solo && hist_fits && P.prepass_mode != 0 &&
                          (P.prepass_mode == 1 || (P.total_atoms <= 4096LL * B && !chain_pays));
    // a topology call (P.topo): the chain with the TOPO binning kernels
    L.prepass = topo ? LatticePath::PRE_CHAIN_TOPO : solo ? LatticePath::PRE_SOLO : per_item ? LatticePath::PRE_ITEMS
              : topo_batch ? LatticePath::PRE_CHAIN_TOPO : LatticePath::PRE_CHAIN;
    L.pipelined_wanted = big && !per_item && !solo;
    // spill slots PER ITEM (k_bin_solo: every atom of the call, so that it cannot run out)
    L.spill = solo ? (unsigned)P.total_atoms : P.spill_cap > 0 ? P.spill_cap : (unsigned)std::max<long long>(1024, P.total_atoms / (8LL * B));
    L.direct_slots = (unsigned long long)((size_t)g.B * (size_t)g.cstride) * (unsigned)L.direct_cap + (unsigned long long)L.spill * (unsigned)g.B;
    // the exact cut-off fix-up: jobs per 256-atom block, per item, or per (item, WIDE atom of the molecule) -- the handle lists
    // them -- or none at all.  (Round 5: one job per item; a wave then walked all of a 30 000-atom frame 64 atoms at a time and
    // took its wide atoms one after the other.)
    // (a batch handle: per wide atom inside the call's range, GridDesc::topo_wide)
    choose_exact_fixup(L, P, g);
    // (the general path has no dense tiles; its fix-up waves still run, and its statistics stay what they were)
    L.dense_wgs = g.force_general ? 0u : (unsigned)(tile_waves < 4096ull ? tile_waves : 4096ull);
    L.redo_cap = P.exact_redo_list > 0 && (unsigned)P.exact_redo_list < REDO_CAP ? (unsigned)P.exact_redo_list : REDO_CAP;   // (a tiny list: tests of the overflow pass)
    return L;
}

// The part of the path that depends on what acquire_set() gave the call (and GridDesc::prepass_hurry, which does too).
inline void settle_lattice_path(LatticePath& L, const LatticeProblem& P, GridDesc& g, bool set_is_pipelined)
{
    // Issue priority of the binning / fill waves that run beside the previous call's tile kernel.  Raised (s_setprio 3)
    // they take issue slots from the tile waves whenever they are ready; left at 0 they live on the slots the tile
    // kernel leaves idle, which is cheaper (cfg2 +2..4 % at 16..512 grids per step) as long as the chain still
    // finishes inside the tile kernel.  It does when the tile kernel has enough work per atom: measured on cfg2's atoms
    // over smaller grids, the chain is late (-8 %) at 2.2 voxels per atom, in time from 2.8 on; the periodic binning
    // (one wave per SIMD beside the tile kernel, not two) needs the raised priority up to cfg4's 3.7 at least.
    g.prepass_hurry = !(set_is_pipelined && !g.pbc && (double)g.B * (double)g.V >= 4.0 * (double)P.total_atoms) ? 1 : 0;
    // k_bin_direct for a big call: whenever asked for (1), and by itself (-1) when the call is NOT pipelined -- in order
    // the one-pass form is 3 % faster (the class table of the previous call on the workspace serves; the chain behind
    // it leaves at once), beside the previous call's tile kernel it gains nothing
    // (a BATCH handle's call that would take the direct pass IS a plain call: the pass reads sigma rows, the handle's own copy serves)
    const bool chain_or_batch = L.prepass == LatticePath::PRE_CHAIN || (L.topo() && P.topo->batch);
    const bool direct_big = chain_or_batch && L.direct_geom &&
                            (P.direct == 1 || (P.direct < 0 && !set_is_pipelined && P.total_atoms >= PIPELINE_MIN_ATOMS));
    L.direct_layout = (L.solo() || direct_big) && L.direct_slots <= 0xFFFF0000ull;
    L.direct_first = L.direct_layout && !L.solo();
    if (L.direct_first && L.topo()) { L.prepass = LatticePath::PRE_CHAIN; choose_exact_fixup(L, P, g); }
    // a small call (one grid): one launch instead of three dependent ones
    L.small_scan = !L.direct_layout && (size_t)g.B * (size_t)g.cstride <= SMALL_PREPASS_MAX_CELLS &&
                   (unsigned)ceil_div(P.total_atoms > 0 ? P.total_atoms : 1, 256) <= SMALL_PREPASS_MAX_BLOCKS;
    // lean: leave registers for the next call's pre-pass
    L.flavour = L.team ? TILES_TEAM : (set_is_pipelined ? TILES_LEAN : TILES_PLAIN);
    if (P.tile_items > 0 ? !L.team : (L.ligand_items && P.tile_team <= 0 && L.per_item())) L.flavour = TILES_ITEMS;
}

// The workspace of one lattice call, typed: what the kernels' parameters are.
struct LatticeWorkspace {
    size_t ncells = 0, count_bytes = 0, direct_bytes = 0;
    unsigned *dense_count = nullptr, *dense_other = nullptr;     // this call's copy of the dense words, and the next call's
    unsigned *cell_count = nullptr, *cell_start = nullptr, *direct_count = nullptr, *rec_cls = nullptr, *cls_table = nullptr;
    float4 *rec_pos = nullptr, *rec_w = nullptr, *tmp_pos = nullptr;
    uint2 *tmp_idx = nullptr, *tmp_cls = nullptr;
    int* err_flag = nullptr;
    unsigned *cls_blocks = nullptr, *cls_l1 = nullptr;           // per-block sigma sets and their first merge (not PRE_ITEMS)
    unsigned *dense_list = nullptr, *redo_list = nullptr;
    // the counter book-keeping of the set (CounterState): what this call may vouch for once it has been enqueued in full
    CounterState* cs = nullptr; size_t clean_after = 0; void* table_before = nullptr;
};

template <class T, class BE>
int ensure_as(BE& be, int slot, size_t bytes, T*& p, int set)
{
    void* v = nullptr;
    const int st = be.ensure(slot, bytes, &v, set);
    return p = static_cast<T*>(v), st;
}

// The buffers of the pre-pass and what is known to be zero in them; fills in the direct layout's fields of `g`.
template <class BE>
int acquire_lattice_workspace(BE& be, const LatticeProblem& P, const LatticePath& L, GridDesc& g, int set, LatticeWorkspace& W)
{
    int st;
    const size_t ncells = W.ncells = (size_t)g.B * (size_t)g.cstride;
    // (when the counters do need a memset its size is a multiple of 256 bytes: an odd tail costs the runtime a second
    //  fill kernel)
    W.count_bytes = (ncells * sizeof(unsigned) + 255) & ~(size_t)255;
    unsigned* dwords_all = nullptr;
    if ((st = ensure_as(be, WS_DENSE_WORDS, 2 * DENSE_SET_WORDS * sizeof(unsigned), dwords_all, set))) return st;
    if ((st = ensure_as(be, WS_CELL_COUNT, W.count_bytes, W.cell_count, set))) return st;
    if ((st = ensure_as(be, WS_CELL_START, (ncells + 1) * sizeof(unsigned), W.cell_start, set))) return st;
    // direct binning (k_bin_direct: opt-in, big calls, the chain as its fall-back; k_bin_solo: small calls, nothing behind it)
    size_t mrec = (size_t)g.M;
    CounterState& cs = *(W.cs = &be.counter_state(set));
    if (L.direct_layout) {
        g.cell_cap = L.direct_cap; g.spill_base = (unsigned)(ncells * (size_t)L.direct_cap); g.spill_cap = L.spill;
        mrec = std::max<size_t>(mrec, (size_t)L.direct_slots);
        g.cnt_shift = (L.solo() && ncells <= (1u << 16)) ? SOLO_CNT_SHIFT : 0;        // small calls: the counters spread out (see GridDesc)
        W.direct_bytes = (((size_t)DIRECT_HEAD + (ncells << g.cnt_shift)) * sizeof(unsigned) + 255) & ~(size_t)255;
        if ((st = ensure_as(be, WS_DIRECT_COUNT, W.direct_bytes, W.direct_count, set))) return st;
        if (cs.dptr != W.direct_count) { cs.dptr = W.direct_count; cs.dclean = 0; }
        // the direct counters and the control words of this call: zero -- k_tail leaves them so after a solo call
        if (cs.dclean < W.direct_bytes && (st = be.fill(W.direct_count, 0, W.direct_bytes))) return st;
        cs.dclean = 0;                                  // (vouched for again once this call has been enqueued in full)
        g.direct_words = W.direct_count;
    }
    if ((st = ensure_as(be, WS_REC_POS, mrec * sizeof(float4), W.rec_pos, set))) return st;
    if ((st = ensure_as(be, WS_REC_W, (L.solo() ? mrec : (size_t)g.M) * sizeof(float4) * 2 * g.G, W.rec_w, set))) return st;
    if ((st = ensure_as(be, WS_REC_CLS, (g.G == 1 ? mrec : (size_t)g.M) * sizeof(unsigned) * g.G, W.rec_cls, set))) return st;
    if ((st = ensure_as(be, WS_CLS_TABLE, (L.per_item() ? (size_t)g.B : (size_t)1) * CLS_TABLE_WORDS * sizeof(unsigned), W.cls_table, set))) return st;
    if ((st = ensure_as(be, WS_ERR, sizeof(int), W.err_flag, 0))) return st;
    if ((st = ensure_as(be, WS_TMP_POS, (size_t)g.M * sizeof(float4), W.tmp_pos, set))) return st;
    if ((st = ensure_as(be, WS_TMP_IDX, (size_t)g.M * sizeof(uint2), W.tmp_idx, set))) return st;
    if ((st = ensure_as(be, WS_TMP_CLS, (size_t)(P.total_atoms > 0 ? P.total_atoms : 1) * g.G * sizeof(uint2), W.tmp_cls, set))) return st;

    if (L.solo()) {
        g.M = (unsigned)mrec;                       // the record arrays' plane stride (rec_w) is the direct layout's slot count
        // a table buffer nobody has written yet: k_bin_solo starts from an empty table
        if (cs.tptr != W.cls_table && (st = be.fill(W.cls_table, 0xff, CLS_TABLE_WORDS * sizeof(unsigned)))) return st;
    }
    W.table_before = cs.tptr;
    cs.tptr = nullptr;                              // (a call that fails half-way leaves no table behind)
    if (cs.ptr != W.cell_count) { cs.ptr = W.cell_count; cs.clean = 0; }
    W.clean_after = cs.clean;
    cs.clean = 0;                                   // nothing is vouched for until this call has been enqueued in full
    if (cs.wptr != dwords_all || !cs.wclean) {      // new buffer, or a call that failed half-way: both copies from scratch
        if ((st = be.fill(dwords_all, 0, 2 * DENSE_SET_WORDS * sizeof(unsigned)))) return st;
        cs.wptr = dwords_all;
    }
    cs.wclean = false;
    W.dense_count = dwords_all + cs.parity * DENSE_SET_WORDS;
    W.dense_other = dwords_all + (cs.parity ^ 1u) * DENSE_SET_WORDS;
    if (L.per_item()) return ST_OK;
    // The counters are zero when a call starts and every call leaves them zero (the scan kernels clear what they
    // read): the memset -- a launch of its own, 6 us of a one-grid call -- is only
    // needed for bytes no call has vouched for yet (a new or grown buffer, a call that failed half-way).
    if (W.clean_after < W.count_bytes) {
        if ((st = be.fill(W.cell_count, 0, W.count_bytes))) return st;
        W.clean_after = W.count_bytes;
    }
    const unsigned nblk = (unsigned)ceil_div(P.total_atoms > 0 ? P.total_atoms : 1, 256);
    if ((st = ensure_as(be, WS_CLS_BLOCKS, (size_t)nblk * CLS_BLOCK_SET * sizeof(unsigned), W.cls_blocks, set))) return st;
    return ensure_as(be, WS_CLS_L1, (size_t)ceil_div(nblk, CLS_ROWS_PER_BLOCK) * MERGE_SET * sizeof(unsigned), W.cls_l1, set);
}

// PRE_ITEMS: one workgroup per item does the whole pre-pass of its item
template <class BE>
int prepass_items(BE& be, const LatticeProblem& P, const GridDesc& g, const LatticeWorkspace& W)
{
    // few items: big blocks (latency of the one item matters); many items: small blocks (they fill the chip) --
    // down to ONE wave per item for ligand-sized items (a block's time is a chain of latencies whatever its
    // size, and four times as many blocks are resident: cfg3's 32 768 items 343 -> ~90 us)
    const long long avg = P.total_atoms / (long long)g.B;
    const unsigned threads = (g.B < 512 && avg > 256) ? 1024u : (g.B >= 2048 && avg <= 64) ? 64u : (g.B >= 2048 && avg <= 128) ? 128u : 256u;
    return with_sigmas(P.sigmas, P.sigmas_f64, [&](auto* sig) {
        using S = sigma_of<decltype(sig)>;
        auto go = [&](auto kern) {
            return be.launch(kern, dim3((unsigned)g.B), dim3(threads), g, P.coords, P.atom_offsets, P.sigmas, P.origins, P.box, P.affine, W.cell_start,
                             W.tmp_pos, W.tmp_idx, W.tmp_cls, W.rec_pos, W.rec_w, W.rec_cls, W.cls_table, W.dense_count, W.err_flag);
        };
        return g.ncell < 512 ? go(k_prepass_items<S, 512>) : g.ncell < 2048 ? go(k_prepass_items<S, 2048>) : go(k_prepass_items<S, ITEM_HIST>);
    });
}

// PRE_SOLO: a small call binned, classed and filled by one launch (its counters: zeroed again by k_tail)
template <class BE>
int prepass_solo(BE& be, const LatticeProblem& P, const GridDesc& g, const LatticeWorkspace& W)
{
    return with_sigmas(P.sigmas, P.sigmas_f64, [&](auto* sig) {
        return be.launch(k_bin_solo<sigma_of<decltype(sig)>>, dim3((unsigned)ceil_div(P.total_atoms, 256)), dim3(256), g, P.coords, P.atom_offsets,
                         P.total_atoms, sig, P.origins, P.affine, W.direct_count, W.rec_pos, W.rec_w, W.rec_cls, W.tmp_cls, W.cls_table, W.cls_blocks);
    });
}

// PRE_CHAIN, PRE_CHAIN_TOPO: [k_bin_direct ->] k_bin_count -> classes + scan -> k_bin_fill
template <class BE>
int prepass_chain(BE& be, const LatticeProblem& P, const LatticePath& L, const GridDesc& g, const LatticeWorkspace& W, int set)
{
    int st;
    const bool topo = L.topo();
    const dim3 ablk(256), agrid((unsigned)ceil_div(P.total_atoms > 0 ? P.total_atoms : 1, 256));
    const unsigned nblk = agrid.x, nfblk = (unsigned)ceil_div((long long)g.M, 256);
    // behind a direct pass the chain is a fall-back that usually leaves at once: a few thousand workgroups that share
    // the blocks instead of one each (k_bin_count, k_bin_fill)
    const dim3 cgrid(L.direct_first && nblk > 4096u ? 4096u : nblk);
    const dim3 fgrid(L.direct_first && nfblk > 4096u ? 4096u : nfblk);
    const unsigned nl1 = (unsigned)ceil_div(nblk, CLS_ROWS_PER_BLOCK);
    const unsigned* dfail = g.direct_words ? g.direct_words + DIRECT_FAILED : nullptr;
    // the one-pass form first; the chain below is enqueued behind it and returns at once unless the pass gave up
    if (L.direct_first && (st = with_sigmas(P.sigmas, P.sigmas_f64, [&](auto* sig) {
            return be.launch(k_bin_direct<sigma_of<decltype(sig)>>, agrid, ablk, g, P.coords, P.atom_offsets, P.total_atoms, sig, P.origins, P.affine,
                             W.direct_count, W.rec_pos, W.rec_cls, W.tmp_cls, W.cls_table, W.cls_blocks);
        }))) return st;
    if (P.total_atoms > 0) {
        auto bin = [&](auto kern, auto* sig) {
            return be.launch(kern, cgrid, ablk, g, P.coords, P.atom_offsets, P.total_atoms, sig, P.origins, P.box, P.affine, W.cell_count, W.tmp_pos,
                             W.tmp_idx, W.tmp_cls, W.cls_blocks, W.err_flag, nblk);
        };
        if (topo) {
            // the ids stand where the sigmas would (bin_atom<.., TOPO>): the one launch whose argument is not of the buffer's type
            auto* ids = (const float*)P.topo->ids;
            st = g.pbc ? bin(k_bin_count<float, 1, false, true>, ids) : bin(k_bin_count<float, 0, false, true>, ids);
        } else {
            st = with_sigmas(P.sigmas, P.sigmas_f64, [&](auto* sig) {
                using S = sigma_of<decltype(sig)>;             // (open boundaries: the direct layouts have no periodic form)
                return L.direct_first ? bin(k_bin_count<S, 0, true>, sig) : g.pbc ? bin(k_bin_count<S, 1>, sig) : bin(k_bin_count<S, 0>, sig);
            });
        }
        if (st) return st;
    }
    // sigma classes (per-block sets -> class table) and the scan of the cell counts, fused two launches deep
    const bool do_classes = P.total_atoms > 0 && !g.force_general && !topo;
    if (!do_classes && !topo && (st = be.fill(W.cls_table, 0xff, CLS_TABLE_WORDS * sizeof(unsigned)))) return st;   // nothing to register
    if (L.small_scan) {
        if ((st = be.launch(k_prepass_small, dim3(1), dim3(SMALL_PREPASS_THREADS), W.cls_blocks, do_classes ? nblk : 0u, W.cls_table, W.cell_count,
                            (unsigned)W.ncells, W.cell_start))) return st;
    } else {
        const size_t nchunks = (W.ncells + 1 + SCAN_CHUNK - 1) / SCAN_CHUNK;
        unsigned* chunks = nullptr;
        if ((st = ensure_as(be, WS_SCAN_CHUNKS, nchunks * sizeof(unsigned), chunks, set))) return st;
        const unsigned nl1_eff = do_classes ? nl1 : 0u;
        if ((st = be.launch(k_prepass_reduce1, dim3(nl1_eff + (unsigned)nchunks), dim3(256), W.cls_blocks, nblk, (unsigned)CLS_ROWS_PER_BLOCK, nl1_eff, W.cls_l1,
                            W.cell_count, W.ncells, chunks, dfail))) return st;
        if ((st = be.launch(k_prepass_reduce2, dim3(do_classes ? 2u : 1u), dim3(256), W.cls_l1, nl1_eff, W.cls_table, chunks, (unsigned)nchunks, dfail))) return st;
        if ((st = be.launch(k_scan_finish, dim3((unsigned)nchunks), dim3(SCAN_THREADS), W.cell_count, W.ncells, chunks, W.cell_start, dfail))) return st;
    }
    if (P.total_atoms <= 0) return ST_OK;
    // (FOUR temp slots per thread with their loads in flight together -- for calls that run alone on the chip, where the
    //  48-register budget does not apply -- were measured: 261 us against 212, the pass is bound by its scattered
    //  stores, not by the round trips in front of them)
    auto fill = [&](auto kern, auto* sig) {
        return be.launch(kern, fgrid, ablk, g, sig, W.cell_start, W.tmp_pos, W.tmp_idx, W.tmp_cls, W.rec_pos, W.rec_w, W.rec_cls, W.cls_table, nfblk);
    };
    if (topo) return fill(k_bin_fill<float, false, true>, (const float*)nullptr);
    return with_sigmas(P.sigmas, P.sigmas_f64, [&](auto* sig) {
        using S = sigma_of<decltype(sig)>;
        return L.direct_first ? fill(k_bin_fill<S, true>, sig) : fill(k_bin_fill<S>, sig);
    });
}

// The tile kernel of the call's flavour and LDS tier, then the tiles left behind (usually none), the statistics for the
// next call and the exact cut-off fix-up.
template <int K, int T, class BE>
int launch_tiles_tier(BE& be, const LatticeProblem& P, const LatticePath& L, const GridDesc& g, const LatticeWorkspace& W)
{
    constexpr int E = ECAP_TIER[T];
    int st;
    const unsigned total_tiles = (unsigned)g.B * (unsigned)g.ntiles;
    auto tiles = [&](auto kern, unsigned waves) {
        return be.launch(kern, dim3(((total_tiles + 7u) / 8u) * 8u, (unsigned)g.G), dim3(WAVE * waves), g, W.cell_start, W.rec_pos, W.rec_w, W.rec_cls,
                         W.cls_table, P.out, W.dense_count, W.dense_list);
    };
    if (L.flavour == TILES_ITEMS) {     // batches of ligand-sized items: a workgroup per item, its entries sorted once
        // one workgroup per item when there are enough items to fill the chip (4 096 waves), else several per item
        long long nchunk = (1024 + g.B - 1) / g.B;
        const long long max_chunk = (g.ntiles + TILE_TEAM - 1) / TILE_TEAM;
        nchunk = nchunk < 1 ? 1 : (nchunk > max_chunk ? max_chunk : nchunk);
        int tpb = (int)((g.ntiles + nchunk - 1) / nchunk);
        tpb = ((tpb + TILE_TEAM - 1) / TILE_TEAM) * TILE_TEAM;
        const unsigned blocks_per_item = (unsigned)((g.ntiles + tpb - 1) / tpb);
        st = be.launch(k_voxelize_items<K>, dim3((unsigned)g.B * blocks_per_item, (unsigned)g.G), dim3(WAVE * TILE_TEAM), g, W.cell_start, W.rec_pos, W.rec_w,
                       W.rec_cls, W.cls_table, P.out, tpb);
    } else if (L.flavour == TILES_TEAM) {      // a handful of tiles (one grid per call): a team of waves per tile
        if constexpr (K == 4) {
            st = L.team_waves == 16 ? tiles(k_voxelize_tiles_team<K, E, 16>, 16u) : L.team_waves == 8 ? tiles(k_voxelize_tiles_team<K, E, 8>, 8u)
                                                                                                  : tiles(k_voxelize_tiles_team<K, E, TILE_TEAM>, (unsigned)TILE_TEAM);
        } else st = tiles(k_voxelize_tiles_team<K, E, TILE_TEAM>, (unsigned)TILE_TEAM);
    } else if constexpr (T <= 1) {    // the biggest tier is LDS-bound to < 3 waves/SIMD anyway: no lean instance of it
        st = L.flavour == TILES_LEAN ? tiles(k_voxelize_tiles_lean<K, E>, 1u) : tiles(k_voxelize_tiles<K, E>, 1u);
    } else {
        st = tiles(k_voxelize_tiles<K, E>, 1u);
    }
    if (st || L.dense_wgs + L.fix_waves == 0u) return st;
    // a topology call with wide atoms: k_tail keeps its dense tiles and bookkeeping, the shells of the wide atoms run in a launch of
    // their own (k_exact_shells: waves without the dense role's LDS footprint), their hits in a third (k_exact_redo)
    const bool split = L.split_exact_fixup;
    const unsigned tail_fix_waves = split ? 1u : L.fix_waves, tail_fix_jobs = split ? 0u : L.fix_jobs;   // (one wave stays for k_tail's housekeeping)
    const bool topo = L.topo();
    // what a fix-up wave of k_tail looks at first (see exact_fixup_block)
    const unsigned* summary = topo ? P.topo->wide_list : g.force_general ? nullptr : L.per_item() ? W.cls_table : W.cls_blocks;
    const uint2* cw = topo ? P.topo->cw : W.tmp_cls;
    // (a topology call recomputes from the handle's copy of the sigma matrix)
    return with_sigmas(topo ? P.topo->sigmas : P.sigmas, topo ? P.topo->sigmas_f64 : P.sigmas_f64, [&](auto* sig) {
        using S = sigma_of<decltype(sig)>;
        int s = be.launch(k_tail<K, E, S>, dim3(L.dense_wgs + tail_fix_waves), dim3(WAVE), g, L.dense_wgs, W.cell_start, W.rec_pos, W.rec_cls, W.cls_table, P.out,
                          W.dense_count, W.dense_other, W.dense_list, g.force_general ? (unsigned*)nullptr : be.feedback_dev(), W.err_flag,
                          topo ? 2 : L.per_item() ? 1 : 0, summary, P.coords, P.atom_offsets, P.total_atoms, sig, P.origins, P.box, P.affine, cw,
                          L.solo() ? W.direct_count : nullptr, L.solo() ? (unsigned)(DIRECT_HEAD + (W.ncells << g.cnt_shift)) : 0u, W.cls_table,
                          g.force_general ? 0u : P.seq, tail_fix_jobs);
        if (s || !split) return s;
        auto shells = [&](auto kern, unsigned max_blocks) {
            return be.launch(kern, dim3(L.fix_jobs < max_blocks ? L.fix_jobs : max_blocks), dim3(WAVE), g, L.fix_jobs, summary, P.coords, P.atom_offsets,
                             P.total_atoms, sig, P.origins, P.box, P.affine, cw, P.out, W.redo_list, L.redo_cap);
        };
        if ((s = shells(k_exact_shells<S, false>, SHELL_BLOCKS))) return s;
        // the listed hits, a wave per (hit, slice of the item's atoms); blocks that find the list empty leave at once
        if ((s = be.launch(k_exact_redo<S>, dim3(REDO_BLOCKS), dim3(WAVE), g, W.redo_list, L.redo_cap, P.coords, P.atom_offsets, sig, P.origins, P.box,
                           P.affine, P.out))) return s;
        // the list was full (REDO_CAP hits in one call)?  Then every shell once more, recomputed in place; else these blocks leave at once
        return shells(k_exact_shells<S, true>, 8192u);
    });
}

template <int K, class BE>
int launch_tiles(BE& be, int tier, const LatticeProblem& P, const LatticePath& L, const GridDesc& g, const LatticeWorkspace& W)
{
    return tier == 0 ? launch_tiles_tier<K, 0>(be, P, L, g, W) : tier == 1 ? launch_tiles_tier<K, 1>(be, P, L, g, W) : launch_tiles_tier<K, 2>(be, P, L, g, W);
}

// The lattice hot path: bin -> scan -> fill -> tile kernel.  All pointers in P are device pointers.
template <class BE>
int run_lattice(BE& be, const LatticeProblem& P_in, std::string& err)
{
    LatticeProblem P = P_in;                // (a batch handle's call that leaves the chain becomes a plain call: see below)
    GridDesc g;
    int st = plan_lattice(P, g, err);
    if (st) return st;
    if (P.B == 0 || g.V == 0) return ST_OK;
    size_t topo_wide_lo = 0;                // a batch handle: where the range's wide atoms start in its list
    // a topology call: what its binning kernels do not cover -- the general path, the tolerance-aware reach (it needs every
    // atom's smallest w at fill time) -- is refused, not approximated
    if (const TopologyDev* t = P.topo) {
        if (t->overflow || g.force_general || g.reach_tau > 0.f) {
            err = "a topology call takes the class-sorted path only: not with more than 15 distinct sigmas, force_general or a value tolerance (use the plain entry point)";
            return ST_EINVAL;
        }
        if (t->C != P.C || t->voxelsize != P.voxelsize || t->n <= 0 || (!t->batch && P.total_atoms != (long long)P.B * t->n)) {
            err = "the topology was built for another channel count / voxel size, or the call is not n_items x its atom count long";
            return ST_EINVAL;
        }
        if (t->batch) {
            const long long i0 = P.topo_first_item;
            if (i0 < 0 || i0 + P.B > (long long)t->n_items || P.total_atoms != t->h_offsets[i0 + P.B] - t->h_offsets[i0]) {
                err = "the call is not a range of the batch topology's items: first item + n_items beyond its items, or another atom count";
                return ST_EINVAL;
            }
            // the range's first atom, the handle's offsets from its first item on, the wide atoms inside it (the list is ascending)
            g.topo_base = t->h_offsets[i0]; g.topo_offsets = t->offsets + i0; g.topo_n = t->max_item;
            const unsigned* w0 = std::lower_bound(t->h_wide_list, t->h_wide_list + t->n_wide, (unsigned)g.topo_base);
            const unsigned* w1 = std::lower_bound(w0, t->h_wide_list + t->n_wide, (unsigned)(g.topo_base + P.total_atoms));
            topo_wide_lo = (size_t)(w0 - t->h_wide_list); g.topo_wide = (unsigned)(w1 - w0);
        } else {
            if ((unsigned long long)g.B * t->n_wide > 0xffffffffull) { err = "too many (item, wide atom) fix-up jobs (>= 2^32): split the batch"; return ST_EINVAL; }
            g.topo_n = t->n; g.topo_wide = t->n_wide;
        }
    }
    LatticePath L = choose_lattice_path(P, g, be.pipelining_possible());
    g.cls_per_item = L.per_item() ? 1 : 0;
    const int set = be.acquire_set(L.pipelined_wanted);
    settle_lattice_path(L, P, g, be.set_is_pipelined(set));
    TopologyDev range;                      // a batch handle as the call's range sees it: every sigma-side array at the range's first atom
    if (P.topo != nullptr && P.topo->batch) {
        const TopologyDev* t = P.topo;
        const size_t a0 = (size_t)g.topo_base;
        const void* sig0 = (const char*)t->sigmas + a0 * (size_t)t->C * (t->sigmas_f64 ? 8 : 4);
        if (L.topo()) {
            range = *t;
            range.ids = t->ids + a0 * (size_t)t->G; range.cw = t->cw + a0 * (size_t)t->G; range.sigmas = sig0;
            range.wide_list = t->wide_list + topo_wide_lo;
            P.topo = &range;
        } else {
            // not the chain (ligand-sized items, one small call, a direct pass): a plain call on the handle's own copy of the sigmas
            P.topo = nullptr; P.sigmas = sig0; P.sigmas_f64 = t->sigmas_f64;
            g.topo_n = 0; g.topo_wide = 0u; g.topo_offsets = nullptr; g.topo_base = 0;
        }
    }
    if (L.solo() && !L.direct_layout) { err = "internal: the one-launch pre-pass does not fit its record slots"; return ST_EINVAL; }

    LatticeWorkspace W;
    if ((st = acquire_lattice_workspace(be, P, L, g, set, W))) return st;
    st = L.per_item() ? prepass_items(be, P, g, W) : L.solo() ? prepass_solo(be, P, g, W) : prepass_chain(be, P, L, g, W, set);
    if (st) return st;
    be.prepass_done(set);

    const unsigned long long tile_waves = (unsigned long long)g.B * (unsigned)g.ntiles * (unsigned)g.G;
    if (tile_waves > 0xFFFF0000ull) { err = "batch too large: more than 2^32 tiles x channel groups; split the batch"; return ST_EINVAL; }
    if ((st = ensure_as(be, WS_DENSE_LIST, (size_t)tile_waves * sizeof(unsigned), W.dense_list, set))) return st;
    const int tier = choose_tier(P.lds_tier, be.feedback_host());
    // a topology call: the tile kernels read the handle's table (nobody writes through it: k_tail's table is a solo call's)
    if (L.topo()) W.cls_table = const_cast<unsigned*>(P.topo->table);
    // ... and, binning through the handle, leave the atoms channel 7 covers out of its lists (every other route: the full lists)
    g.cover_violated = L.topo() && P.cover_fold >= 0 ? P.topo->cover_violated : nullptr;
    if (L.split_exact_fixup) {
        if ((st = ensure_as(be, WS_REDO_LIST, (size_t)(REDO_HEAD + (size_t)REDO_CAP * REDO_ENTRY) * sizeof(unsigned), W.redo_list, set))) return st;
        // (the list's counter back to zero: queued behind the previous call's k_exact_redo on this stream, in front of this call's hot kernels)
        if ((st = be.launch(k_zero_words, dim3(1), dim3(WAVE), W.redo_list, (unsigned)REDO_HEAD))) return st;
    }
    be.hot_begin(L.flavour, g.K, ECAP_TIER[tier]);
    st = g.K == 8 ? launch_tiles<8>(be, tier, P, L, g, W) : launch_tiles<4>(be, tier, P, L, g, W);
    be.hot_end();
    const bool tail_ran = L.dense_wgs + L.fix_waves != 0u;
    if (!st) {
        CounterState& cs = *W.cs;
        cs.clean = W.clean_after;
        cs.wclean = true;
        cs.tptr = L.topo() ? W.table_before : W.cls_table;       // every pre-pass leaves a whole table in the buffer (a topology call: untouched)
        if (L.solo()) cs.dclean = W.direct_bytes;                // k_tail has zeroed them
        if (tail_ran) cs.parity ^= 1u;                           // k_tail has cleared the other copy: the next call's
    }
    const bool tail_mirrors = !st && !g.force_general && be.feedback_dev() != nullptr;
    be.note_error_flag_mirrored(tail_mirrors && L.dense_wgs != 0u);
    be.note_tail_reports(tail_mirrors && tail_ran && P.seq != 0u);
    be.tile_done(set);
    return st;
}

// Build a molecule's topology into caller-provided device buffers (cw [n, G] uint2, ids [n, G], table [CLS_TABLE_WORDS],
// flags [1] int, zeroed by the caller); `d_sigmas` is the library's own copy.  The caller reads table[CLS_OVERFLOW] and
// flags[0] back once the stream has drained.  Workspace: the class-set slots of set 0.
template <class BE>
int run_topology_build(BE& be, const void* d_sigmas, int sigmas_f64, long long n, int C, double voxelsize, uint2* cw, unsigned* ids,
                       unsigned* table, int* flags /* 2 words, zeroed */, unsigned* wide_list /* [n] */, std::string& err,
                       unsigned* violated = nullptr /* [G] words, zeroed: the cover fold's input (TopologyDev::cover_violated) */)
{
    if (n <= 0 || C <= 0) { err = "a topology needs n_atoms > 0 and n_channels > 0"; return ST_EINVAL; }
    if (!(voxelsize > 0.0) || !std::isfinite(voxelsize)) { err = "voxelsize must be a positive finite number"; return ST_EINVAL; }
    const int G = ceil_div(C, CHG);
    const double w_scale = voxelsize * voxelsize, R = CUTOFF_A / voxelsize;
    const float w_exact_max = (float)(7.647 / (R * R));                     // plan_lattice's rule
    const unsigned nblk = (unsigned)ceil_div(n, 256), nl1 = (unsigned)ceil_div(nblk, CLS_ROWS_PER_BLOCK);
    unsigned *bsets = nullptr, *l1sets = nullptr;
    int st;
    if ((st = ensure_as(be, WS_CLS_BLOCKS, (size_t)nblk * CLS_BLOCK_SET * sizeof(unsigned), bsets, 0))) return st;
    if ((st = ensure_as(be, WS_CLS_L1, (size_t)nl1 * MERGE_SET * sizeof(unsigned), l1sets, 0))) return st;
    return with_sigmas(d_sigmas, sigmas_f64, [&](auto* sig) {
        using S = sigma_of<decltype(sig)>;
        int s;
        if ((s = be.launch(k_topology_classes<S>, dim3(nblk), dim3(256), sig, n, C, G, w_scale, cw, bsets))) return s;
        if ((s = be.launch(k_merge_classes, dim3(nl1), dim3(256), bsets, nblk, (unsigned)CLS_BLOCK_SET, CLS_ROWS_PER_BLOCK, l1sets, (unsigned*)nullptr))) return s;
        if ((s = be.launch(k_merge_classes, dim3(1), dim3(256), l1sets, nl1, (unsigned)MERGE_SET, nl1, (unsigned*)nullptr, table))) return s;
        return be.launch(k_topology_ids<S>, dim3(nblk), dim3(256), sig, cw, table, n, C, G, w_scale, w_exact_max, ids, flags, wide_list, violated);
    });
}

// Explicit centres: sigma -> w, then the brute-force double-precision kernel.
template <class BE>
int run_centers(BE& be, const double* d_centers, long long V, const float* d_coords, long long N,
                const void* d_sigmas, int sigmas_f64, int C, const double* box_host, float* d_out,
                std::string& err)
{
    if (V < 0 || N < 0 || C <= 0) { err = "n_centers/n_atoms must be >= 0 and n_channels > 0"; return ST_EINVAL; }
    if (V == 0) return ST_OK;
    if (box_host)
        for (int ax = 0; ax < 3; ++ax)
            if (!(box_host[ax] > 2.0 * CUTOFF_A)) { err = "periodic box edges must be > 10 A (2 x cutoff)"; return ST_EBOX; }
    // the launch below is dim3(ceil(V / 64), G): refused here, by name, instead of by the runtime at the launch
    if (((long long)C + CHG - 1) / CHG > 65535) { err = "explicit centres: at most 524280 channels (65535 channel groups of 8, the grid's y limit)"; return ST_EINVAL; }
    if ((V - 1) / EXPL_CENTERS + 1 > 0x7fffffffLL) { err = "explicit centres: at most 2^31 - 1 blocks of 64 centres (the grid's x limit)"; return ST_EINVAL; }
    const int G = ceil_div(C, CHG);
    float4* w = nullptr;
    int st = ensure_as(be, WS_W_EXPLICIT, (size_t)(N > 0 ? N : 1) * sizeof(float4) * 2 * G, w, 0);
    if (st) return st;
    if (N > 0) {
        st = with_sigmas(d_sigmas, sigmas_f64, [&](auto* sig) {
            return be.launch(k_sigma_to_w<sigma_of<decltype(sig)>>, dim3((unsigned)ceil_div(N, 256)), dim3(256), sig, N, C, G, 1.0, w);
        });
        if (st) return st;
    }
    // 64 centres per workgroup; its waves split the atoms: as many (4, 8, 16) as it takes to put ~4 waves on every SIMD
    const long long wgs = ceil_div(V, EXPL_CENTERS) * G;
    int waves = 4;
    while (waves < EXPL_MAX_WAVES && wgs * waves < 4096) waves *= 2;
    const dim3 grid((unsigned)ceil_div(V, EXPL_CENTERS), (unsigned)G), blk((unsigned)(waves * WAVE));
    be.note_dist_kernel(("mkamd::k_occupancy_centers, " + std::to_string(waves) + " waves").c_str());   // (the tests: every block size runs)
    return be.launch(k_occupancy_centers, grid, blk, d_centers, V, d_coords, N, w, C,
                     box_host ? 1 : 0, box_host ? box_host[0] : 0.0, box_host ? box_host[1] : 0.0,
                     box_host ? box_host[2] : 0.0, d_out);
}

template <class BE>
int run_grid_centers(BE& be, const double* bb_min, const int* nvox, double voxelsize, double* d_centers,
                     std::string& err)
{
    if (nvox[0] < 0 || nvox[1] < 0 || nvox[2] < 0) { err = "nvoxels must be >= 0"; return ST_EINVAL; }
    const long long V = (long long)nvox[0] * nvox[1] * nvox[2];
    if (V == 0) return ST_OK;
    return be.launch(k_grid_centers, dim3((unsigned)ceil_div(V, 256)), dim3(256), bb_min[0], bb_min[1],
                     bb_min[2], nvox[0], nvox[1], nvox[2], voxelsize, d_centers);
}

// Is this centre list a getCenters lattice (x slowest, z fastest, one positive step)?  The test of
// moleculekit_amd/voxeldescriptors.py::_recognise_lattice_numpy in two passes over the array instead of a dozen numpy
// temporaries: axis lengths from the first place z (then y, at stride nz) stops increasing, one common positive step,
// then every centre against fl64(index * step) + centre 0 with the tolerance 1e-9 * max(1, max |c|).  Host code.
inline bool lattice_from_centers(const double* c, long long V, double* bb_min, int* nvoxels, double* voxelsize)
{
    if (!c || !bb_min || !nvoxels || !voxelsize || V < 2) return false;
    long long nz = V;
    for (long long i = 1; i < V; ++i) if (c[3 * i + 2] <= c[3 * (i - 1) + 2]) { nz = i; break; }
    if (V % nz) return false;
    const long long rows = V / nz;
    long long ny = rows;
    for (long long i = 1; i < rows; ++i) if (c[3 * (i * nz) + 1] <= c[3 * ((i - 1) * nz) + 1]) { ny = i; break; }
    if (rows % ny) return false;
    const long long nx = rows / ny;
    if (nx > 0x7fffffff || ny > 0x7fffffff || nz > 0x7fffffff) return false;
    double steps[3]; int ns = 0;
    if (nz > 1) steps[ns++] = c[3 * 1 + 2] - c[2];
    if (ny > 1) steps[ns++] = c[3 * nz + 1] - c[1];
    if (nx > 1) steps[ns++] = c[3 * (nz * ny) + 0] - c[0];
    if (ns == 0) return false;
    for (int i = 0; i < ns; ++i) if (!(steps[i] > 0.0)) return false;
    const double vs = steps[0];
    const double stol = 1e-9 * std::max(1.0, std::fabs(vs));
    for (int i = 0; i < ns; ++i) if (std::fabs(steps[i] - vs) > stol) return false;
    double maxabs = 0.0;
    for (long long i = 0; i < 3 * V; ++i) {
        const double a = std::fabs(c[i]);
        if (!(a <= maxabs)) { if (a != a) return false; maxabs = a; }           // a NaN centre is no lattice
    }
    const double tol = 1e-9 * std::max(1.0, maxabs);
    const double o[3] = {c[0], c[1], c[2]};
    const double* q = c;
    for (long long ix = 0; ix < nx; ++ix) {
        const double ex = (double)ix * vs + o[0];
        for (long long iy = 0; iy < ny; ++iy) {
            const double ey = (double)iy * vs + o[1];
            for (long long iz = 0; iz < nz; ++iz, q += 3) {
                const double ez = (double)iz * vs + o[2];
                if (std::fabs(ex - q[0]) > tol || std::fabs(ey - q[1]) > tol || std::fabs(ez - q[2]) > tol) return false;
            }
        }
    }
    bb_min[0] = o[0]; bb_min[1] = o[1]; bb_min[2] = o[2];
    nvoxels[0] = (int)nx; nvoxels[1] = (int)ny; nvoxels[2] = (int)nz;
    *voxelsize = vs;
    return true;
}

// mkamd_calculate_occupancy's choice between the tiled lattice kernels and the pairwise double-precision kernel
// (occupancy_utils.pyx:34-61 takes any centre list; its one caller passes a lattice).  Only "not a lattice" and the
// lattice plan's own refusal of a geometry (ST_EINVAL: more than 1023 cells per axis, a cutoff of more than 512 voxels,
// more than 2^31 tiles) reach the pairwise kernel; every other status of the lattice path -- a HIP error, a failed
// allocation -- is the call's status.
template <class Lattice, class Pairwise>
inline int route_calculate_occupancy(bool is_lattice, Lattice&& lattice, Pairwise&& pairwise)
{
    if (is_lattice) {
        const int st = lattice();
        if (st != ST_EINVAL) return st;
    }
    return pairwise();
}

}  // namespace mkamd
