// tests/emu/emu_cover_fold.cpp -- TEST INFRASTRUCTURE: the cover fold (GridDesc::cover_violated, round 8) on the host emulation.
// The emulation library's translation unit, whole, plus one entry point: a handle (frame or batch) built by the product's kernels
// WITH the violated-class words, the masks the host derives from them, and a range of its items through run_lattice with the
// fold on or off.  Built twice by tests/emu_cover_fold_build.py: as it is, and with -DMK_DIAG=128 (the fold compiled out while
// channel 7 still leaves the covered atoms out: the mutation the tests must catch).
#include "emu_capi.cpp"

namespace {
struct CoverHandle {
    std::vector<uint2> cw;
    std::vector<unsigned> ids, table, wide_list, violated, cover;
    TopologyDev T;
};

// mirrors topology_create_impl (capi.hip) with host memory standing in for the device's
int build_cover_handle(EmuBackend& be, CoverHandle& H, const void* sigmas, int sigmas_f64, long long n, const long long* offsets, int n_items, int C,
                       double voxelsize)
{
    const int G = ceil_div(C, CHG);
    H.cw.resize((size_t)n * G);
    H.ids.assign((size_t)n * G, 0xCDCDCDCDu); H.table.assign(CLS_TABLE_WORDS, 0xCDCDCDCDu); H.wide_list.assign((size_t)n, 0xCDCDCDCDu);
    H.violated.assign((size_t)G, 0u);
    int flags2[2] = {0, 0};
    const int st = run_topology_build(be, sigmas, sigmas_f64, n, C, voxelsize, H.cw.data(), H.ids.data(), H.table.data(), flags2, H.wide_list.data(), g_err,
                                      H.violated.data());
    if (st) return st;
    std::sort(H.wide_list.begin(), H.wide_list.begin() + flags2[1]);
    H.cover.resize((size_t)G);
    for (int gq = 0; gq < G; ++gq) H.cover[gq] = ~H.violated[gq] & 0xfffeu;
    TopologyDev& T = H.T;
    T.n = n; T.C = C; T.G = G; T.sigmas_f64 = sigmas_f64; T.voxelsize = voxelsize; T.ids = H.ids.data(); T.cw = H.cw.data(); T.sigmas = sigmas;
    T.table = H.table.data(); T.overflow = H.table[CLS_OVERFLOW] != CLS_EMPTY; T.wide = (flags2[0] & 1) != 0;
    T.wide_list = H.wide_list.data(); T.n_wide = (unsigned)flags2[1];
    T.cover_violated = H.violated.data(); T.h_cover = H.cover.data();
    if (offsets) {
        T.batch = true; T.n_items = n_items; T.offsets = offsets; T.h_offsets = offsets; T.h_wide_list = H.wide_list.data();
        for (int b = 0; b < n_items; ++b) T.max_item = std::max(T.max_item, offsets[b + 1] - offsets[b]);
    }
    return 0;
}
}  // namespace

extern "C" {

// batch_offsets != NULL: a BATCH handle over n_items items (`sigmas` of all their atoms), the call its items [first_item, + B);
// NULL: a FRAME handle of n_atoms atoms, the call B sets of coordinates of it.  coords / call_offsets / origins / box / features are
// the call's.  cover_fold: LatticeProblem::cover_fold (0 on, -1 off).  masks_out [G]: the handle's cover masks; table_out [16]: its
// class table (w bits).  features == NULL: the handle alone.
int emu_cover_fold_voxelize(int n_items, const long long* batch_offsets, long long n_atoms, const void* sigmas, int sigmas_f64, int C, int first_item,
                            int B, const float* coords, const long long* call_offsets, const double* origins, const int* nvox, double voxelsize,
                            const float* box, int max_images, int tile_k, int tile_team, int lds_tier, int cover_fold, float* features,
                            int* err_flag_out, unsigned* masks_out, unsigned* table_out, unsigned* feedback_out)
{
    EmuBackend be;
    void* eflag = nullptr;
    be.ensure(WS_ERR, sizeof(int), &eflag);
    *(int*)eflag = 0;
    CoverHandle H;
    int st = build_cover_handle(be, H, sigmas, sigmas_f64, batch_offsets ? batch_offsets[n_items] : n_atoms, batch_offsets, n_items, C, voxelsize);
    if (st) return st;
    for (int gq = 0; gq < H.T.G; ++gq) masks_out[gq] = H.cover[gq];
    if (table_out) for (int i = 0; i < CLS_TABLE_WORDS; ++i) table_out[i] = H.table[i];
    if (!features) return 0;
    LatticeProblem P;
    P.B = B; P.total_atoms = B > 0 ? call_offsets[B] : 0; P.C = C; P.sigmas_f64 = sigmas_f64;
    P.nvox[0] = nvox[0]; P.nvox[1] = nvox[1]; P.nvox[2] = nvox[2];
    P.voxelsize = voxelsize; P.pbc = box ? 1 : 0; P.tile_k = tile_k; P.max_images = box ? max_images : 1;
    P.prepass_mode = 0; P.tile_team = tile_team; P.tile_items = 0; P.direct = 0; P.lds_tier = lds_tier; P.cover_fold = cover_fold;
    P.coords = coords; P.atom_offsets = call_offsets; P.sigmas = nullptr; P.origins = origins;
    P.box = box; P.out = features; P.topo = &H.T; P.topo_first_item = first_item;
    const size_t nout = (size_t)B * nvox[0] * nvox[1] * nvox[2] * C;
    for (size_t i = 0; i < nout; ++i) features[i] = -123.0f;
    st = run_lattice(be, P, g_err);
    if (err_flag_out) *err_flag_out = *(int*)be.bufs[WS_ERR];
    if (feedback_out) for (int i = 0; i < FEEDBACK_WORDS; ++i) feedback_out[i] = be.feedback[i];
    return st;
}

}  // extern "C"
