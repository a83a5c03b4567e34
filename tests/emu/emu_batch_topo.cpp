// tests/emu/emu_batch_topo.cpp -- TEST INFRASTRUCTURE: the BATCH topology handle (pipeline.h TopologyDev::batch, round 7) on the host
// emulation.  The emulation library's translation unit, whole, plus two entry points of its own: a handle built by the product's
// kernels over all atoms of a ragged batch and a RANGE of its items through run_lattice, and the launch sequence of such a call on
// the recording backend.
#include "emu_capi.cpp"

namespace {
struct BatchHandle {
    std::vector<uint2> cw;
    std::vector<unsigned> ids, table, wide_list;
    TopologyDev T;
};

// mirrors topology_create_impl (capi.hip) with host memory standing in for the device's
int build_batch_handle(EmuBackend& be, BatchHandle& H, const void* sigmas, int sigmas_f64, const long long* offsets, int n_items, int C, double voxelsize)
{
    const long long n = offsets[n_items];
    const int G = ceil_div(C, CHG);
    H.cw.resize((size_t)n * G);
    H.ids.assign((size_t)n * G, 0xCDCDCDCDu); H.table.assign(CLS_TABLE_WORDS, 0xCDCDCDCDu); H.wide_list.assign((size_t)n, 0xCDCDCDCDu);
    int flags2[2] = {0, 0};
    const int st = run_topology_build(be, sigmas, sigmas_f64, n, C, voxelsize, H.cw.data(), H.ids.data(), H.table.data(), flags2, H.wide_list.data(), g_err);
    if (st) return st;
    std::sort(H.wide_list.begin(), H.wide_list.begin() + flags2[1]);
    TopologyDev& T = H.T;
    T.n = n; T.C = C; T.G = G; T.sigmas_f64 = sigmas_f64; T.voxelsize = voxelsize; T.ids = H.ids.data(); T.cw = H.cw.data(); T.sigmas = sigmas;
    T.table = H.table.data(); T.overflow = H.table[CLS_OVERFLOW] != CLS_EMPTY; T.wide = (flags2[0] & 1) != 0;
    T.wide_list = H.wide_list.data(); T.n_wide = (unsigned)flags2[1];
    T.batch = true; T.n_items = n_items; T.offsets = offsets; T.h_offsets = offsets; T.h_wide_list = H.wide_list.data();
    for (int b = 0; b < n_items; ++b) T.max_item = std::max(T.max_item, offsets[b + 1] - offsets[b]);
    return 0;
}
}  // namespace

extern "C" {

// items [first_item, first_item + B) of the batch (`batch_offsets` [n_items + 1], `sigmas` of ALL its atoms) through the handle;
// coords / call_offsets (rebased) / origins / box / affine / features are the RANGE's.  *wide_out: wide atoms in the whole handle.
int emu_voxelize_lattice_batch_topo(int n_items, const long long* batch_offsets, const void* sigmas, int sigmas_f64, int C, int first_item, int B,
                                    const float* coords, const long long* call_offsets, const double* origins, const int* nvox, double voxelsize,
                                    const float* box, int max_images, int tile_k, const double* affine, int prepass_mode, int tile_team, int tile_items,
                                    int direct, int exact_redo, float* features, int* err_flag_out, int* wide_out)
{
    EmuBackend be;
    void* eflag = nullptr;
    be.ensure(WS_ERR, sizeof(int), &eflag);
    *(int*)eflag = 0;
    BatchHandle H;
    int st = build_batch_handle(be, H, sigmas, sigmas_f64, batch_offsets, n_items, C, voxelsize);
    if (st) return st;
    if (wide_out) *wide_out = (int)H.T.n_wide;
    LatticeProblem P;
    P.B = B; P.total_atoms = B > 0 ? call_offsets[B] : 0; P.C = C; P.sigmas_f64 = sigmas_f64;
    P.nvox[0] = nvox[0]; P.nvox[1] = nvox[1]; P.nvox[2] = nvox[2];
    P.voxelsize = voxelsize; P.pbc = box ? 1 : 0; P.tile_k = tile_k; P.max_images = box ? max_images : 1;
    P.prepass_mode = prepass_mode; P.tile_team = tile_team; P.tile_items = tile_items; P.direct = direct; P.exact_redo_list = exact_redo;
    P.coords = coords; P.atom_offsets = call_offsets; P.sigmas = nullptr; P.origins = origins;
    P.box = box; P.affine = affine; P.out = features; P.topo = &H.T; P.topo_first_item = first_item;
    const size_t nout = (size_t)B * nvox[0] * nvox[1] * nvox[2] * C;
    for (size_t i = 0; i < nout; ++i) features[i] = -123.0f;
    st = run_lattice(be, P, g_err);
    if (err_flag_out) *err_flag_out = *(int*)be.bufs[WS_ERR];
    return st;
}

// the launch sequence of a batch-handle call on the recorder: `n_items` items of `item_atoms` atoms each in the handle, the call its
// items [first_item, + B); `wide_every` > 0: every wide_every-th atom of the batch is wide.  Text: emu_trace_text().
int emu_trace_lattice_batch(int n_items, long long item_atoms, int first_item, int B, int C, const int* nvox, int pbc, int max_images, int prepass_mode,
                            int tile_team, int tile_items, int direct, int exact_redo, int wide_every, int pipelining, int calls)
{
    RecBackend be;
    be.can_pipeline = pipelining != 0;
    std::vector<long long> offs((size_t)n_items + 1);
    for (int b = 0; b <= n_items; ++b) offs[b] = (long long)b * item_atoms;
    std::vector<unsigned> wide;
    if (wide_every > 0) for (long long a = 0; a < offs[n_items]; a += wide_every) wide.push_back((unsigned)a);
    const size_t big = (size_t)1 << 40;
    TopologyDev T;
    T.n = offs[n_items]; T.C = C; T.G = ceil_div(C, CHG); T.voxelsize = 1.0;
    T.ids = (const unsigned*)be.range("topo.ids", big); T.cw = (const uint2*)be.range("topo.cw", big); T.sigmas = be.range("topo.sigmas", big);
    T.table = (const unsigned*)be.range("topo.table", big); T.wide_list = (const unsigned*)be.range("topo.wide_list", big);
    T.n_wide = (unsigned)wide.size(); T.wide = !wide.empty();
    T.batch = true; T.n_items = n_items; T.offsets = (const long long*)be.range("topo.offsets", big); T.h_offsets = offs.data();
    T.h_wide_list = wide.data(); T.max_item = item_atoms;
    LatticeProblem P;
    P.B = B; P.total_atoms = (long long)B * item_atoms; P.C = C; P.nvox[0] = nvox[0]; P.nvox[1] = nvox[1]; P.nvox[2] = nvox[2];
    P.pbc = pbc; P.max_images = pbc ? max_images : 1; P.prepass_mode = prepass_mode; P.tile_team = tile_team; P.tile_items = tile_items;
    P.direct = direct; P.exact_redo_list = exact_redo; P.voxelsize = 1.0;
    P.coords = (const float*)be.range("coords", big); P.atom_offsets = (const long long*)be.range("offsets", big);
    P.origins = (const double*)be.range("origins", big); P.box = pbc ? (const float*)be.range("box", big) : nullptr;
    P.out = (float*)be.range("out", big); P.topo = &T; P.topo_first_item = first_item;
    int st = 0;
    for (int c = 0; c < calls && !st; ++c) {
        be.out += "call " + std::to_string(c) + "\n";
        st = run_lattice(be, P, g_err);
        be.out += "  status " + std::to_string(st) + (st ? ": " + g_err : std::string()) + "\n";
    }
    g_trace = be.out;
    return st;
}

}  // extern "C"
