// capi.hip -- extern "C" boundary of libmkamd.so (see include/mkamd_voxel.h) and the HIP backend
// that drives the launch sequences of pipeline.h on an MI355X.  One context = one device, one
// stream, one grow-only workspace.  Without a GPU every context entry point fails with MKAMD_ENODEV / MKAMD_EHIP; the one
// host implementation (mkamd_calculate_occupancy_cpu, cpu_occupancy.h) is a separate, explicit entry point nothing here falls back to.
#include "../../include/mkamd_voxel.h"
#include "../../include/mkamd_distance.h"
#include "../../include/mkamd_xtc.h"
#include "xtc_reader.h"
#include <atomic>
#include "pipeline.h"
#include "dist_pipeline.h"
#include "align_pipeline.h"
#include "sasa_pipeline.h"
#include "shell_pipeline.h"
#include "dihedral_pipeline.h"
#include "moments_pipeline.h"
#include "wrap_pipeline.h"
#include "wrap_cell_pipeline.h"
#include "ring_pipeline.h"
#include "hbond_pipeline.h"
#include "bond_pipeline.h"
#include "clash_pipeline.h"
#include "within_pipeline.h"
#include "dssp_pipeline.h"
#include "arith_probe.h"
#include "host_pack.h"
#include "xtc_gpu.h"
#include "xtc_encode.h"
#include "dcd_kernels.h"
#include "xtc_headers.h"
#include "cpu_occupancy.h"

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

using namespace mkamd;

// The message of the calling thread's last failure: a fixed buffer, so that reporting an error can never throw
// (an std::string here could raise bad_alloc on the way out of an extern "C" function).
static thread_local char g_last_error[512] = "";

static int fail(int code, const char* msg) noexcept
{
    snprintf(g_last_error, sizeof g_last_error, "%s", msg ? msg : "");
    return code;
}
static int fail(int code, const std::string& msg) noexcept { return fail(code, msg.c_str()); }

// what an entry point returns after a run_* of the pipelines: its status, with the message it left (if any) as the last error
static int run_status(int st, const std::string& err) noexcept
{
    if (st) return err.empty() ? st : fail(st, err);
    return MKAMD_OK;
}

static int hip_fail(hipError_t e, const char* what) noexcept
{
    snprintf(g_last_error, sizeof g_last_error, "%s: %s", what, hipGetErrorString(e));
    return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? MKAMD_ENODEV : MKAMD_EHIP;
}

// Every extern "C" entry point is a function-try-block closed by this: nothing C++ (bad_alloc from a vector / string,
// anything a dependency throws) crosses the C boundary; it comes back as a status + message like every other failure.
#define MK_API_CATCH                                                                              \
    catch (const std::bad_alloc&) { return fail(MKAMD_ENOMEM, "out of host memory"); }            \
    catch (const std::exception& e) { return fail(MKAMD_EHIP, e.what()); }                        \
    catch (...) { return fail(MKAMD_EHIP, "unexpected C++ exception"); }

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return hip_fail(_e, #expr); \
    } while (0)

struct mkamd_ctx {
    int device = 0;
    int n_cus = 256;                       // compute units of the device (launch plans that count wave slots: dist_pipeline.h)
    int compute_units() const { return n_cus; }
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;          // stream the launches of the current call go to (main or side)
    hipStream_t main_stream = nullptr;     // the caller-visible stream
    hipStream_t side_stream = nullptr;     // internal: pre-pass of pipelined calls
    hipEvent_t ev_host_done = nullptr;     // end of a small synchronous host call's launches (voxelize_lattice_host_begin_impl)
    hipEvent_t ev_inputs = nullptr;        // main -> side: the call's inputs are ready
    hipEvent_t ev_pre_done[2] = {};        // side -> main: workspace set s is filled
    hipEvent_t ev_tile_done[2] = {};       // main -> side: the tile kernel that read set s has finished
    hipEvent_t inputs_marker = nullptr;    // the event the next pipelined pre-pass waits for (ev_inputs or a timing event)
    hipEvent_t tile_marker[2] = {};        // ditto per workspace set (ev_tile_done[s] or a timing event)
    hipEvent_t last_hot_end = nullptr;
    bool tile_pending[2] = {false, false};
    int next_set = 0;
    bool in_pipelined_prepass = false;
    bool pipelining = false;               // opt-in (mkamd_ctx_set_pipelining)
    bool promise = false;                  // one-shot: the NEXT lattice call's inputs are promised (mkamd_ctx_promise_inputs)
    hipEvent_t promise_event = nullptr;    // ... complete once this event has completed (nullptr: complete already)
    long long n_pipelined = 0;             // lattice calls whose pre-pass went to the side stream (mkamd_ctx_pipelined_calls)
    bool have_pre_tile_event = false;
    void* bufs[2 * WS_NSLOTS] = {};        // two workspace sets (set 1 only used by pipelined calls)
    CounterState counters[2];              // what is known about each set's cell counters between calls
    size_t caps[2 * WS_NSLOTS] = {};
    int tile_k = 0;
    int force_general = 0;
    int lds_tier = -1;                     // -1 = adaptive
    int prepass_mode = -1;                 // -1 = automatic
    int tile_items = -1;                   // -1 = automatic
    int exact_redo = 0;                    // 0 = automatic (mkamd_ctx_set_exact_redo), -1 = never
    int cover_fold = 0;                    // 0 = automatic (mkamd_ctx_set_cover_fold), -1 = never
    int tile_team = -1;                    // -1 = automatic
    int fine_cells = 0;                    // 1 = half-cutoff cells (A-B benchmarking)
    int direct = -1;                       // direct binning: -1 automatic, 0 never, 1 whenever possible (mkamd_ctx_set_direct_binning)
    double value_tol = 0.0;                // tolerance-aware reach (mkamd_ctx_set_value_tolerance); 0 = the hard 5 A cutoff everywhere
    unsigned* fb_host = nullptr;           // pinned, device-visible: tier statistics of the last finished call
    unsigned* fb_dev = nullptr;
    bool err_mirrored = false;             // fb_host[NTIER+1] holds the error flag as of the last lattice call
    void* stage_host = nullptr;            // pinned staging for the inputs of small _host calls (one H2D copy)
    void* stage_host_dev = nullptr;        // device-side address of the same memory (mapped): tiny inputs are read in place
    size_t stage_cap = 0;
    std::vector<uint32_t> contacts_host;   // result of the last mkamd_contacts_trajectory_host call (owned here)
    std::vector<uint32_t> ring_pairs_host; // results of the last mkamd_ring_interactions_host call (owned here)
    std::vector<float> ring_distang_host;
    int ring_avoid = 0;                    // mkamd_ctx_set_ring_plan
    long long ring_chunk = 0;
    std::vector<int> hbond_triples_host;   // result of the last mkamd_hbonds_host call (owned here)
    int hbond_avoid = 0;                   // mkamd_ctx_set_hbond_plan
    long long hbond_chunk = 0;
    std::vector<int> bond_pairs_host;      // result of the last mkamd_guess_bonds_host call (owned here)
    int bond_avoid = 0;                    // mkamd_ctx_set_bond_plan
    std::vector<int> clash_pairs_host;     // results of the last mkamd_find_clashes_host call (owned here)
    std::vector<float> clash_dist_host, clash_over_host;
    int clash_avoid = 0;                   // mkamd_ctx_set_clash_plan
    int within_avoid = 0;                  // mkamd_ctx_set_within_plan
    int dssp_avoid = 0;                    // mkamd_ctx_set_dssp_plan
    std::vector<float> packed_coords;      // the selected atoms' rows of a host distance call (host_pack.h), kept between calls
    std::vector<float> f32_stage;          // host staging of big float64-out results
    struct PendingHostCall { bool active = false; size_t out_bytes = 0; bool mapped_out = false; unsigned seq = 0; void* dout = nullptr; hipEvent_t done = nullptr; };
    PendingHostCall pending;               // a host call between its begin and its end (voxelize_lattice_host_begin_impl)
    void* out_host = nullptr;              // pinned, device-mapped result buffer of small _host calls (no D2H copy)
    void* out_host_dev = nullptr;          // its device-side address
    // tile-kernel timing
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used, ev_free;
    hipEvent_t cur0 = nullptr, cur1 = nullptr;
    int launch_status = 0;

    // ---- backend concept (pipeline.h) ----
    CounterState& counter_state(int set) { return counters[set & 1]; }
    const volatile unsigned* feedback_host() const { return fb_host; }
    unsigned* feedback_dev() const { return fb_dev; }
    void note_error_flag_mirrored(bool yes) { err_mirrored = yes; }
    void note_tail_reports(bool yes) { tail_reports = yes; }
    int dist_avoid = 0;                    // kernels dist_trajectory must not take (mkamd_ctx_set_dist_kernels: tests, A-B timing)
    int reduction_block = 0;               // k_dist_reduction_closest's first-group atoms in registers (mkamd_ctx_set_reduction_block)
    char last_dist_kernel[128] = "";       // what the last dist_trajectory call launched (mkamd_ctx_last_dist_kernel)
    void note_dist_kernel(const char* name) { snprintf(last_dist_kernel, sizeof last_dist_kernel, "%s", name); }
    void note_dist_kernel_append(const char* more) { strncat(last_dist_kernel, more, sizeof last_dist_kernel - strlen(last_dist_kernel) - 1); }
    bool tail_reports = false;             // the last lattice call's k_tail writes FB_TILES_DONE / FB_TAIL_WROTE with seq_next
    unsigned seq_next = 0, seq_counter = 0; // sequence number handed to the next lattice call (0 = none)
    int ensure(int slot, size_t bytes, void** ptr, int set = 0)
    {
        slot += set * WS_NSLOTS;
        if (bytes == 0) bytes = 16;
        if (caps[slot] < bytes) {
            if (bufs[slot]) {
                HIP_TRY(hipStreamSynchronize(main_stream));  // buffer may still be in use
                if (side_stream) HIP_TRY(hipStreamSynchronize(side_stream));
                HIP_TRY(hipFree(bufs[slot]));
                bufs[slot] = nullptr; caps[slot] = 0;
            }
            const size_t want = bytes + bytes / 4 + 256;     // grow-only, 25 % slack
            hipError_t e = hipMalloc(&bufs[slot], want);
            if (e != hipSuccess) return hip_fail(e, "hipMalloc(workspace)");
            caps[slot] = want;
        }
        *ptr = bufs[slot];
        return 0;
    }
    // a workspace buffer that grows WITH its first keep_bytes (the device-resident contact list: chunks are appended)
    int grow_keep(int slot, size_t bytes, size_t keep_bytes, void** ptr)
    {
        if (bytes == 0) bytes = 16;
        if (caps[slot] < bytes) {
            void* fresh = nullptr;
            const size_t want = bytes + bytes / 2 + 256;
            hipError_t e = hipMalloc(&fresh, want);
            if (e != hipSuccess) return hip_fail(e, "hipMalloc(contact list)");
            if (bufs[slot] && keep_bytes) {
                e = hipMemcpyAsync(fresh, bufs[slot], keep_bytes, hipMemcpyDeviceToDevice, stream);
                if (e != hipSuccess) { (void)hipFree(fresh); return hip_fail(e, "hipMemcpyAsync(contact list)"); }
            }
            if (bufs[slot]) {
                HIP_TRY(hipStreamSynchronize(stream));
                HIP_TRY(hipFree(bufs[slot]));
            }
            bufs[slot] = fresh; caps[slot] = want;
        }
        *ptr = bufs[slot];
        return 0;
    }
    int fill(void* p, int byte, size_t bytes)
    {
        HIP_TRY(hipMemsetAsync(p, byte, bytes, stream));
        return 0;
    }
    int to_host(void* dst, const void* src_dev, size_t bytes)
    {
        HIP_TRY(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return 0;
    }
    int to_device(void* dst_dev, const void* src, size_t bytes)
    {
        HIP_TRY(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, stream));
        return 0;
    }
    template <class... KA, class... A>
    int launch(void (*kernel)(KA...), dim3 grid, dim3 block, A... args)
    {
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // ---- cross-call software pipeline (pipeline.h: acquire_set / prepass_done / tile_done) ----
    // Every event record / stream wait below is checked: a failed one would silently remove the ordering the results
    // depend on, so on failure the context drains both streams (which restores a trivially correct order), turns
    // pipelining off for good (`pipeline_broken`) and the call carries on in order on the caller's stream.
    bool pipeline_broken = false;
    bool sync_ok(hipError_t e)
    {
        if (e == hipSuccess) return true;
        (void)hipGetLastError();
        pipeline_broken = true;
        if (side_stream) (void)hipStreamSynchronize(side_stream);
        (void)hipStreamSynchronize(main_stream);
        tile_pending[0] = tile_pending[1] = false;
        have_pre_tile_event = false;
        return false;
    }
    int acquire_set(bool big_enough)
    {
        in_pipelined_prepass = false;
        // a promised call (mkamd_ctx_promise_inputs) waits for the event its inputs come with, on whichever stream runs its
        // pre-pass; should that wait fail, the streams have been drained and the event is awaited on the host
        auto await_promise = [&](hipStream_t s) {
            if (!promise_event) return;
            if (!sync_ok(hipStreamWaitEvent(s, promise_event, 0))) (void)hipEventSynchronize(promise_event);
        };
        if (!big_enough || !(pipelining || promise) || !side_stream || pipeline_broken) {
            // in-order call on the caller's stream, set 0 (any earlier pipelined call has already made the
            // main stream wait for its pre-pass; its tile kernel is ahead of us on the same stream)
            await_promise(main_stream);
            have_pre_tile_event = false;
            return 0;
        }
        const int set = next_set;
        // Inputs must not depend on work enqueued after the PREVIOUS call's tile kernel (the opt-in contract of
        // mkamd_ctx_set_pipelining): the side stream is ordered after everything before that launch only.
        if (!have_pre_tile_event) {
            if (!sync_ok(hipEventRecord(ev_inputs, main_stream))) { await_promise(main_stream); return 0; }
            inputs_marker = ev_inputs;
        }
        if (!sync_ok(hipStreamWaitEvent(side_stream, inputs_marker, 0))) { await_promise(main_stream); return 0; }
        if (tile_pending[set] && !sync_ok(hipStreamWaitEvent(side_stream, tile_marker[set], 0))) { await_promise(main_stream); return 0; }
        if (promise_event && !sync_ok(hipStreamWaitEvent(side_stream, promise_event, 0))) { (void)hipEventSynchronize(promise_event); return 0; }
        next_set ^= 1;
        stream = side_stream;
        in_pipelined_prepass = true;
        ++n_pipelined;
        return set;
    }
    bool set_is_pipelined(int) const { return in_pipelined_prepass; }
    bool pipelining_possible() const { return (pipelining || promise) && side_stream && !pipeline_broken; }
    void prepass_done(int set)
    {
        if (!in_pipelined_prepass) return;
        stream = main_stream;
        // on failure sync_ok() has drained the side stream: the pre-pass is complete, the tile kernel may follow
        if (sync_ok(hipEventRecord(ev_pre_done[set], side_stream)) && sync_ok(hipStreamWaitEvent(main_stream, ev_pre_done[set], 0)))
            have_pre_tile_event = true;                               // hot_begin() records the marker
    }
    void tile_done(int set)
    {
        if (!side_stream) return;
        // Only a PIPELINED call needs the marker (the pre-pass that reuses its workspace set two calls later waits for
        // it).  An in-order call is covered by stream order: the next pipelined pre-pass first waits for a marker recorded
        // on the main stream after everything enqueued so far (acquire_set, !have_pre_tile_event).  The event is a barrier
        // packet of its own -- ~2 us of every one-molecule call on a context that has ever had pipelining switched on.
        const bool piped = in_pipelined_prepass;
        in_pipelined_prepass = false;
        if (pipeline_broken || !piped) { last_hot_end = nullptr; return; }
        if (last_hot_end) { tile_marker[set] = last_hot_end; tile_pending[set] = true; }   // the timing event sits at the same place
        else if (sync_ok(hipEventRecord(ev_tile_done[set], main_stream))) { tile_marker[set] = ev_tile_done[set]; tile_pending[set] = true; }
        last_hot_end = nullptr;
    }
    // Events are barrier packets the command processor takes ~5 us each to retire, and they sit between one
    // call's tile kernel and the next one's: the timing events double as the pipeline's markers when both exist.
    int last_flavour = -1, last_K = 0, last_ecap = 0;      // the tile kernel of the last lattice call (mkamd_ctx_last_tile_kernel)
    void hot_begin(int flavour, int K, int ecap)
    {
        last_flavour = flavour; last_K = K; last_ecap = ecap;
        last_hot_end = nullptr;
        if (timing) {
            std::pair<hipEvent_t, hipEvent_t> ev;
            bool ok = true;
            if (!ev_free.empty()) { ev = ev_free.back(); ev_free.pop_back(); }
            else ok = hipEventCreate(&ev.first) == hipSuccess && hipEventCreate(&ev.second) == hipSuccess;
            if (ok && hipEventRecord(ev.first, stream) == hipSuccess) {
                cur0 = ev.first; cur1 = ev.second;
                if (in_pipelined_prepass) inputs_marker = cur0;       // "everything before this call's tile kernel"
                return;
            }
            (void)hipGetLastError();                                  // no timing for this launch; the marker below still goes in
        }
        if (in_pipelined_prepass) {
            if (sync_ok(hipEventRecord(ev_inputs, main_stream))) inputs_marker = ev_inputs;
        }
    }
    void hot_end()
    {
        if (!timing || !cur0) return;
        if (hipEventRecord(cur1, stream) == hipSuccess) {
            ev_used.emplace_back(cur0, cur1);
            last_hot_end = cur1;
        } else {
            (void)hipGetLastError();
            ev_free.emplace_back(cur0, cur1);
        }
        cur0 = cur1 = nullptr;
    }
};

// A molecule's topology on the device (include/mkamd_voxel.h, mkamd_topology_create_*): one allocation, owned here.
struct mkamd_topology {
    int device = 0;
    void* mem = nullptr;                   // sigmas copy | cw | ids | table | flags + violated-class words | wide list | atom offsets (a batch handle)
    mkamd::TopologyDev dev;
    std::vector<unsigned> h_cover;         // per channel group: the classes its channel 7 covers (dev.h_cover)
    std::vector<long long> h_offsets;      // a batch handle: its atom offsets and its wide list on the host (dev.h_offsets, dev.h_wide_list)
    std::vector<unsigned> h_wide;
};

// `pending_ok`: the entry point may run between the two halves of a host call (mkamd_voxelize_lattice_host_begin / _end): the
// halves themselves, and what touches neither the pending call's result buffer nor the workspace it reads (queries, the
// centre generator, copies out).  Every other entry point would regrow or overwrite what `end` is about to hand back --
// it is refused, not guessed at.
static int check_ctx(mkamd_ctx* ctx, bool pending_ok = false)
{
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (!pending_ok && ctx->pending.active)
        return fail(MKAMD_EINVAL, "a host call begun on this context (mkamd_voxelize_lattice_host_begin) has not been ended: call _end (or mkamd_ctx_abandon_pending) first");
    HIP_TRY(hipSetDevice(ctx->device));
    ctx->stream = ctx->main_stream;           // a failed call may have left the side stream selected
    return 0;
}

// read + clear the device-side error flag (after the stream has been synchronised)
static int collect_async_errors(mkamd_ctx* ctx)
{
    if (!ctx->bufs[WS_ERR]) return 0;
    // the last lattice call's dense kernel mirrored the flag into pinned host memory: no copy on the clean path
    if (ctx->err_mirrored && ctx->fb_host && ((volatile unsigned*)ctx->fb_host)[NTIER + 1] == 0u) return 0;
    int flag = 0;
    HIP_TRY(hipMemcpy(&flag, ctx->bufs[WS_ERR], sizeof(int), hipMemcpyDeviceToHost));
    if (flag == 0) return 0;
    HIP_TRY(hipMemset(ctx->bufs[WS_ERR], 0, sizeof(int)));
    if (flag & MK_ERR_TOPOLOGY) return fail(MKAMD_EINVAL, "a topology call was given an item that is not the topology's atom count long (a batch topology: not the atoms of its item); results are incomplete");
    if (flag & MK_ERR_BAD_BOX) return fail(MKAMD_EBOX, "periodic box edges must be > 10 A (2 x cutoff)");
    if (flag & MK_ERR_TOO_MANY_IMAGES) return fail(MKAMD_EBOX, "periodic box much smaller than the grid (too many images)");
    return fail(MKAMD_EOVERFLOW, "more periodic images than max_images_per_atom allowed; results are incomplete");
}

static int ensure_err_flag(mkamd_ctx* ctx)
{
    if (ctx->bufs[WS_ERR]) return 0;
    void* p = nullptr;
    int st = ctx->ensure(WS_ERR, sizeof(int), &p);
    if (st) return st;
    HIP_TRY(hipMemsetAsync(p, 0, sizeof(int), ctx->stream));
    return 0;
}

// One wave that spins for `ref_ticks` of the fixed-frequency reference counter (s_memrealtime) and reports how far the SHADER clock
// counter (s_memtime) got meanwhile: launched on a stream of the caller's beside the work whose clock is asked for.
__global__ void k_clock_probe(unsigned long long ref_ticks, unsigned long long* __restrict__ out)
{
    if (threadIdx.x != 0) return;
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), t0 = __builtin_readcyclecounter();
    unsigned long long r;
    unsigned spins = 0u;                                             // (bounded whatever the counter does: a probe must not be able to hang a queue)
    do { __builtin_amdgcn_s_sleep(16); r = __builtin_amdgcn_s_memrealtime(); } while (r - r0 < ref_ticks && ++spins < (1u << 25));
    const unsigned long long t1 = __builtin_readcyclecounter();
    out[0] = t1 - t0;
    out[1] = r - r0;
}


extern "C" {

#ifndef MKAMD_SRC_HASH            // _build.py: sha256 over the sources this library was compiled from (first 16 hex digits)
#define MKAMD_SRC_HASH "unstamped"
#endif
// (the hash is what ties a measurement to a build: profiles/*_pmc_counters.json carry it, bench.py refuses counters of another build)
const char* mkamd_version(void) { return "moleculekit_amd 0.4.0 (gfx950, HIP) src " MKAMD_SRC_HASH MKAMD_BUILD_KIND; }

const char* mkamd_last_error(void) { return g_last_error; }

int mkamd_device_count(int* count)
try {
    if (!count) return fail(MKAMD_EINVAL, "count is NULL");
    *count = 0;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    *count = n;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_create(int device, mkamd_ctx** out)
try {
    if (!out) return fail(MKAMD_EINVAL, "ctx out-pointer is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(MKAMD_ENODEV, std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (device < 0 || device >= n) return fail(MKAMD_EINVAL, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    mkamd_ctx* c = new mkamd_ctx();
    c->device = device;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->n_cus = cus; }
    e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return hip_fail(e, "hipStreamCreate"); }
    c->stream = c->main_stream = c->own_stream;
    // the pre-pass kernels are small and latency-bound: give their queue the highest priority so that they
    // get wave slots as the (huge) tile grid of the previous call retires waves, instead of waiting for it to drain
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    bool ok = hipStreamCreateWithPriority(&c->side_stream, hipStreamNonBlocking, prio_greatest) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_inputs, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2 && ok; ++i)
        ok = hipEventCreateWithFlags(&c->ev_pre_done[i], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->ev_tile_done[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) c->side_stream = nullptr;          // fall back to a single in-order stream
    // tier statistics come back through pinned host memory the dense kernel writes directly (no copy, no sync)
    if (hipHostMalloc((void**)&c->fb_host, FEEDBACK_WORDS * sizeof(unsigned), hipHostMallocMapped) == hipSuccess) {
        for (int i = 0; i < FEEDBACK_WORDS; ++i) c->fb_host[i] = 0u;
        if (hipHostGetDevicePointer((void**)&c->fb_dev, c->fb_host, 0) != hipSuccess) c->fb_dev = nullptr;
    } else {
        c->fb_host = nullptr;                   // no feedback: the leanest tier is always used
    }
    if (!c->fb_dev && c->fb_host) { (void)hipHostFree(c->fb_host); c->fb_host = nullptr; }
    *out = c;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_destroy(mkamd_ctx* ctx)
try {
    if (!ctx) return MKAMD_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->side_stream) (void)hipStreamSynchronize(ctx->side_stream);
    for (int i = 0; i < 2 * WS_NSLOTS; ++i)
        if (ctx->bufs[i]) (void)hipFree(ctx->bufs[i]);
    for (auto& ev : ctx->ev_used) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (auto& ev : ctx->ev_free) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (ctx->side_stream) { (void)hipStreamSynchronize(ctx->side_stream); (void)hipStreamDestroy(ctx->side_stream); }
    if (ctx->ev_host_done) (void)hipEventDestroy(ctx->ev_host_done);
    if (ctx->ev_inputs) (void)hipEventDestroy(ctx->ev_inputs);
    for (int i = 0; i < 2; ++i) {
        if (ctx->ev_pre_done[i]) (void)hipEventDestroy(ctx->ev_pre_done[i]);
        if (ctx->ev_tile_done[i]) (void)hipEventDestroy(ctx->ev_tile_done[i]);
    }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    if (ctx->fb_host) (void)hipHostFree(ctx->fb_host);
    if (ctx->stage_host) (void)hipHostFree(ctx->stage_host);
    if (ctx->out_host) (void)hipHostFree(ctx->out_host);
    delete ctx;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_stream(mkamd_ctx* ctx, void* hip_stream)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    // NULL is a real stream (the legacy default stream, which is what torch.cuda.current_stream() usually is);
    // (void*)-1 selects the context's own stream again
    hipStream_t next = hip_stream == (void*)-1 ? ctx->own_stream : (hipStream_t)hip_stream;
    if (next == ctx->main_stream) return MKAMD_OK;
    HIP_TRY(hipStreamSynchronize(ctx->main_stream)); // workspace is shared between the streams
    if (ctx->side_stream) HIP_TRY(hipStreamSynchronize(ctx->side_stream));
    ctx->tile_pending[0] = ctx->tile_pending[1] = false;
    ctx->have_pre_tile_event = false;         // the next pipelined pre-pass takes its marker from the NEW stream
    ctx->stream = ctx->main_stream = next;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_abandon_pending(mkamd_ctx* ctx)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (!ctx->pending.active) return MKAMD_OK;
    // the kernels of the abandoned call still write the result buffer and read the workspace: drained before anything reuses them
    ctx->pending.active = false;
    if (ctx->side_stream) HIP_TRY(hipStreamSynchronize(ctx->side_stream));
    HIP_TRY(hipStreamSynchronize(ctx->main_stream));
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_synchronize(mkamd_ctx* ctx)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (ctx->side_stream) HIP_TRY(hipStreamSynchronize(ctx->side_stream));
    HIP_TRY(hipStreamSynchronize(ctx->main_stream));
    return collect_async_errors(ctx);
} MK_API_CATCH

int mkamd_ctx_poll_errors(mkamd_ctx* ctx)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    // the dense pass of every lattice call mirrors the device-side flag into pinned host memory: reading it costs
    // nothing and needs no synchronisation; only a raised flag pays for the drain + the precise report
    if (!ctx->fb_host || ((volatile unsigned*)ctx->fb_host)[NTIER + 1] == 0u) return MKAMD_OK;
    if (ctx->side_stream) HIP_TRY(hipStreamSynchronize(ctx->side_stream));
    HIP_TRY(hipStreamSynchronize(ctx->main_stream));
    ctx->err_mirrored = false;
    st = collect_async_errors(ctx);
    ((volatile unsigned*)ctx->fb_host)[NTIER + 1] = 0u;
    return st;
} MK_API_CATCH

int mkamd_ctx_device_info(mkamd_ctx* ctx, char* name, size_t len, int* compute_units,
                          uint64_t* hbm_bytes, char* arch, size_t arch_len)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, ctx->device));
    if (name && len) { strncpy(name, p.name, len - 1); name[len - 1] = 0; }
    if (arch && arch_len) { strncpy(arch, p.gcnArchName, arch_len - 1); arch[arch_len - 1] = 0; }
    if (compute_units) *compute_units = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (uint64_t)p.totalGlobalMem;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_tile_k(mkamd_ctx* ctx, int k)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (k != 0 && k != 4 && k != 8) return fail(MKAMD_EINVAL, "tile K must be 0 (auto), 4 or 8");
    ctx->tile_k = k;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_lds_tier(mkamd_ctx* ctx, int tier)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (tier < -1 || tier >= NTIER) return fail(MKAMD_EINVAL, "LDS tier must be -1 (adaptive), 0, 1 or 2");
    ctx->lds_tier = tier;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_prepass_mode(mkamd_ctx* ctx, int mode)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (mode < -1 || mode > 1) return fail(MKAMD_EINVAL, "pre-pass mode must be -1 (automatic), 0 (kernel chain) or 1 (per-item)");
    ctx->prepass_mode = mode;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_tile_team(mkamd_ctx* ctx, int mode)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (mode < -1 || (mode > 1 && mode != 4 && mode != 8 && mode != 16))
        return fail(MKAMD_EINVAL, "tile team mode must be -1 (automatic), 0 (one wave per tile), 1 (a team of waves per tile) or 4 / 8 / 16 (a team of that many waves)");
    ctx->tile_team = mode;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_tile_items(mkamd_ctx* ctx, int mode)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (mode < -1 || mode > 1) return fail(MKAMD_EINVAL, "tile items mode must be -1 (automatic), 0 (tiles on their own) or 1 (a workgroup per item)");
    ctx->tile_items = mode;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_exact_redo(mkamd_ctx* ctx, int mode)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (mode != 0 && mode != -1) return fail(MKAMD_EINVAL, "exact redo mode must be 0 (automatic) or -1 (recompute inside the last launch)");
    ctx->exact_redo = mode;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_cover_fold(mkamd_ctx* ctx, int mode)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (mode != 0 && mode != -1) return fail(MKAMD_EINVAL, "cover fold mode must be 0 (automatic) or -1 (every channel keeps its full lists)");
    ctx->cover_fold = mode;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_fine_cells(mkamd_ctx* ctx, int on)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    ctx->fine_cells = on != 0;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_direct_binning(mkamd_ctx* ctx, int mode)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (mode < -1 || mode > 2) return fail(MKAMD_EINVAL, "direct binning mode must be -1 (automatic), 0 (never), 1 (whenever possible) or 2 (the one-launch pre-pass whenever possible)");
    ctx->direct = mode;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_value_tolerance(mkamd_ctx* ctx, double eps)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (!(eps >= 0.0) || eps > 1e-5) return fail(MKAMD_EINVAL, "value tolerance must be in [0, 1e-5] (0 = off)");
    ctx->value_tol = eps;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_force_general(mkamd_ctx* ctx, int on)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    ctx->force_general = on != 0;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_pipelining(mkamd_ctx* ctx, int on)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    HIP_TRY(hipStreamSynchronize(ctx->main_stream));
    if (ctx->side_stream) HIP_TRY(hipStreamSynchronize(ctx->side_stream));
    ctx->pipelining = on != 0;
    ctx->pipeline_broken = false;             // both streams are drained: a fresh start
    ctx->have_pre_tile_event = false;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_promise_inputs(mkamd_ctx* ctx, void* hip_event)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    ctx->promise = true;
    ctx->promise_event = (hipEvent_t)hip_event;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_pipelined_calls(mkamd_ctx* ctx, int64_t* n)
try {
    if (!ctx || !n) return fail(MKAMD_EINVAL, "ctx / n is NULL");
    *n = (int64_t)ctx->n_pipelined;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_last_tile_kernel(mkamd_ctx* ctx, char* name, size_t name_cap)
try {
    if (!ctx || !name || name_cap == 0) return fail(MKAMD_EINVAL, "ctx / name is NULL");
    static const char* const base[] = {"k_voxelize_tiles", "k_voxelize_tiles_lean", "k_voxelize_tiles_team", "k_voxelize_items"};
    if (ctx->last_flavour < 0 || ctx->last_flavour > 3) snprintf(name, name_cap, "%s", "");
    else if (ctx->last_flavour == 3) snprintf(name, name_cap, "mkamd::%s<%d>", base[3], ctx->last_K);
    else snprintf(name, name_cap, "mkamd::%s<%d, %d>", base[ctx->last_flavour], ctx->last_K, ctx->last_ecap);
    return MKAMD_OK;
} MK_API_CATCH

// the short correctly-rounded square root of the distance kernels against the provable form, over every float it is used for
int mkamd_selftest_sqrt(mkamd_ctx* ctx, uint64_t* mismatches, uint32_t* first_bad_bits)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (!mismatches) return fail(MKAMD_EINVAL, "mismatches pointer is NULL");
    void* w = nullptr;
    if ((st = ctx->ensure(WS_D_TOT, 16, &w, 0))) return st;
    HIP_TRY(hipMemsetAsync(w, 0, 16, ctx->stream));
    const unsigned lo = 0x0F800000u;                                // 2^-96: below it mk_fsqrt_rn takes its scaled branch
    const unsigned long long n = 0x7F800000ull - lo;
    if ((st = ctx->launch(k_selftest_sqrt, dim3(65536), dim3(256), lo, n, (unsigned long long*)w, (unsigned*)((char*)w + 8)))) return st;
    unsigned long long host[2] = {0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(host, w, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *mismatches = (uint64_t)host[0];
    if (first_bad_bits) *first_bad_bits = (uint32_t)(host[1] & 0xffffffffull);
    return MKAMD_OK;
} MK_API_CATCH

// one device function per `op` (arith_probe.h), elementwise over device arrays, on the context's stream: asynchronous
int mkamd_selftest_arith(mkamd_ctx* ctx, int op, long long n, const void* a, const void* b, const void* c, void* out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    const char* err = nullptr;
    st = run_arith_probe(*ctx, op, n, a, b, c, out, err);
    if (err) return fail(MKAMD_EINVAL, err);
    return st;
} MK_API_CATCH

// Every distance kernel takes its roots with mk_fsqrt_rn_ordinary, whose correct rounding is a PROPERTY OF THIS CHIP's v_rsq_f32 (checked
// exhaustively, not proved: mk_device.h).  So the exhaustive comparison runs once per process and device, in front of the first
// distance call (a few milliseconds), and a device -- another stepping, firmware or compiler lowering of the reciprocal square root --
// on which it finds a mismatch gets no distances at all rather than wrong last bits.  -1 unknown, 1 good, 0 bad.
static std::atomic<int> g_sqrt_verdict[64];
static struct SqrtVerdictInit { SqrtVerdictInit() { for (auto& v : g_sqrt_verdict) v.store(-1); } } g_sqrt_verdict_init;

static int dist_entry(mkamd_ctx* ctx)
{
    int st = check_ctx(ctx);
    if (st) return st;
    const int d = ctx->device >= 0 && ctx->device < 64 ? ctx->device : 0;
    int v = g_sqrt_verdict[d].load();
    if (v < 0) {
        uint64_t bad = 0;
        uint32_t first = 0;
        if ((st = mkamd_selftest_sqrt(ctx, &bad, &first))) return st;
        v = bad == 0 ? 1 : 0;
        g_sqrt_verdict[d].store(v);
        if (!v) {
            char msg[200];
            snprintf(msg, sizeof msg, "float32 square-root self-test failed on this device (%llu mismatches, first at bits 0x%08x): "
                     "the distance kernels would not be bit-exact here", (unsigned long long)bad, first);
            return fail(MKAMD_EHIP, msg);
        }
    }
    if (!v) return fail(MKAMD_EHIP, "float32 square-root self-test failed on this device: the distance kernels would not be bit-exact here");
    return MKAMD_OK;
}

int mkamd_clock_probe_dev(mkamd_ctx* ctx, void* hip_stream, int64_t microseconds, uint64_t* d_ticks2)
try {
    if (!ctx || !d_ticks2) return fail(MKAMD_EINVAL, "ctx / result pointer is NULL");
    if (microseconds < 1 || microseconds > 5000000) return fail(MKAMD_EINVAL, "clock probe: 1 us .. 5 s");
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, (unsigned long long)microseconds * 100ull,
                       (unsigned long long*)d_ticks2);
    HIP_TRY(hipGetLastError());
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_dist_kernels(mkamd_ctx* ctx, int avoid_mask)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (avoid_mask < 0 || avoid_mask > 65535) return fail(MKAMD_EINVAL, "avoid mask: bits 1 (block-per-frame kernel), 2 (row kernel), 4 (rectangular tile kernel), 8 (16-byte row stores), 16 (the row kernel wherever it applies), 32 (host calls upload the whole coordinate array), 64 (selfdist calls keep the pair-table kernel), 128 (short-row calls of few frames keep the tile kernel), 256 / 512 (shell counts: not the frame-lane / not the atom-lane kernel), 1024 / 2048 (dihedrals: the same), 4096 / 8192 (group moments: not the form in which a lane group owns a (frame, group) / not the segmented form), 16384 / 32768 (periodic wrap: not the lane-per-group / not the wave-per-group kernel)");
    ctx->dist_avoid = avoid_mask;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_set_reduction_block(mkamd_ctx* ctx, int block)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (block != 0 && block != 4 && block != 8 && block != -1 && block != -2 && block != 104 && block != 108)
        return fail(MKAMD_EINVAL, "reduction block: 0 (choose), 4, 8 (+ 100: blocks of four waves), -1 (the generic kernel) or -2 (the few-frame kernel)");
    ctx->reduction_block = block;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_last_dist_kernel(mkamd_ctx* ctx, char* name, size_t name_cap)
try {
    if (!ctx || !name || name_cap == 0) return fail(MKAMD_EINVAL, "ctx / name is NULL");
    snprintf(name, name_cap, "%s", ctx->last_dist_kernel);
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_withdraw_promise(mkamd_ctx* ctx)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    ctx->promise = false;
    ctx->promise_event = nullptr;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_enable_kernel_timing(mkamd_ctx* ctx, int enable)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    ctx->timing = enable != 0;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_ctx_read_kernel_timing(mkamd_ctx* ctx, double* total_ms, int64_t* launches)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    double tot = 0.0;
    int64_t n = 0;
    for (auto& ev : ctx->ev_used) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) { tot += ms; ++n; }
        ctx->ev_free.push_back(ev);
    }
    ctx->ev_used.clear();
    if (total_ms) *total_ms = tot;
    if (launches) *launches = n;
    return MKAMD_OK;
} MK_API_CATCH

// A big result usually lands in FRESH host memory (np.empty / np.zeros: pages nobody has touched), and the copy out of the
// device then faults them in one by one on one thread (measured: 34 ms for 537 MB against 13 ms into pages that exist).
// Called after the kernels are enqueued and before the copy: host threads touch the destination in contiguous slices
// while the GPU works (xtc_reader.h, prefault_output: it writes zeros, so only for buffers the copy overwrites entirely).
static void prefault_big_result(void* dst, size_t bytes)
{
    if (!dst || bytes < ((size_t)32 << 20)) return;
    const int nt = (int)std::min<unsigned>(32u, std::max(1u, std::thread::hardware_concurrency()));
    mkamd::xtc::prefault_output(static_cast<float*>(dst), bytes / sizeof(float), nt);
}

// ---------------------------------------------------------------------------------------------
// explicit centres
// ---------------------------------------------------------------------------------------------
int mkamd_occupancy_centers_dev(mkamd_ctx* ctx, const double* d_centers, int64_t n_centers,
                                const float* d_coords, int64_t n_atoms, const void* d_sigmas,
                                int sigmas_are_f64, int32_t n_channels, const double* box_host,
                                float* d_features)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (n_centers > 0 && (!d_centers || !d_features)) return fail(MKAMD_EINVAL, "centers/features pointer is NULL");
    if (n_atoms > 0 && (!d_coords || !d_sigmas)) return fail(MKAMD_EINVAL, "coords/sigmas pointer is NULL");
    std::string err;
    st = run_centers(*ctx, d_centers, n_centers, d_coords, n_atoms, d_sigmas, sigmas_are_f64, n_channels,
                     box_host, d_features, err);
    return run_status(st, err);
} MK_API_CATCH

int mkamd_occupancy_centers_host(mkamd_ctx* ctx, const double* centers, int64_t V, const float* coords,
                                 int64_t N, const void* sigmas, int sigmas_are_f64, int32_t C,
                                 const double* box, float* features)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (V < 0 || N < 0 || C <= 0) return fail(MKAMD_EINVAL, "n_centers/n_atoms must be >= 0 and n_channels > 0");
    if (V == 0) return MKAMD_OK;
    if (!centers || !features) return fail(MKAMD_EINVAL, "centers/features pointer is NULL");
    if (N > 0 && (!coords || !sigmas)) return fail(MKAMD_EINVAL, "coords/sigmas pointer is NULL");
    const size_t sz = sigmas_are_f64 ? 8 : 4;
    void *dc = nullptr, *dx = nullptr, *ds = nullptr, *dout = nullptr;
    if ((st = ctx->ensure(WS_H_CENTERS, (size_t)V * 24, &dc))) return st;
    if ((st = ctx->ensure(WS_H_COORDS, (size_t)N * 12, &dx))) return st;
    if ((st = ctx->ensure(WS_H_SIGMAS, (size_t)N * C * sz, &ds))) return st;
    if ((st = ctx->ensure(WS_H_OUT, (size_t)V * C * 4, &dout))) return st;
    HIP_TRY(hipMemcpyAsync(dc, centers, (size_t)V * 24, hipMemcpyHostToDevice, ctx->stream));
    if (N > 0) {
        HIP_TRY(hipMemcpyAsync(dx, coords, (size_t)N * 12, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(ds, sigmas, (size_t)N * C * sz, hipMemcpyHostToDevice, ctx->stream));
    }
    st = mkamd_occupancy_centers_dev(ctx, (const double*)dc, V, (const float*)dx, N, ds, sigmas_are_f64, C, box, (float*)dout);
    if (st) return st;
    prefault_big_result(features, (size_t)V * C * 4);
    HIP_TRY(hipMemcpyAsync(features, dout, (size_t)V * C * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MKAMD_OK;
} MK_API_CATCH

static int voxelize_lattice_host_begin_impl(mkamd_ctx* ctx, int32_t B, const float* coords, const int64_t* atom_offsets,
                                            const void* sigmas, int sigmas_are_f64, int32_t C, const double* origins,
                                            const int32_t* nvoxels, double voxelsize, const float* box, int32_t max_images);
static int voxelize_lattice_host_end_impl(mkamd_ctx* ctx, float* features, double* features64, double* max_into);

int mkamd_calculate_occupancy(mkamd_ctx* ctx, const double* centers, int64_t V, const float* coords,
                              int64_t N, const double* sigmas, int32_t C, double* results)
try {
    if (V < 0 || N < 0 || C <= 0) return fail(MKAMD_EINVAL, "n_centers/n_atoms must be >= 0 and n_channels > 0");
    if (V == 0 || N == 0) return ctx ? MKAMD_OK : fail(MKAMD_EINVAL, "ctx is NULL");
    if (!results) return fail(MKAMD_EINVAL, "results pointer is NULL");
    int st0 = check_ctx(ctx);
    if (st0) return st0;
    std::vector<float>& tmp = ctx->f32_stage;               // context-owned: no fresh pages to fault in on every call
    // The reference's only caller hands this function a getCenters LATTICE (voxeldescriptors.py:356 via _getOccupancyC):
    // recognised (two passes over the centres, host) it takes the tiled lattice kernels -- microseconds where the
    // pairwise kernel below tests N x V pairs in double.
    // A status other than "this geometry is not for the tiled kernels" (MKAMD_EINVAL: every argument has been checked
    // above, so what is left are the capacity limits of the lattice plan) goes back to the caller -- a HIP error or a
    // failed allocation is not retried on a kernel a hundred times slower (route_calculate_occupancy, pipeline.h).
    double bb_min[3], vs = 0.0;
    int32_t nv[3];
    const bool is_lattice = mkamd::lattice_from_centers(centers, (long long)V, bb_min, nv, &vs);
    bool lattice_done = false;
    const int st = mkamd::route_calculate_occupancy(is_lattice,
        [&] { const int64_t offs[2] = {0, N};                  // (the in-place maximum is taken by the call's second half)
              const int s1 = voxelize_lattice_host_begin_impl(ctx, 1, coords, offs, sigmas, 1, C, bb_min, nv, vs, nullptr, 0);
              if (s1) return s1;
              lattice_done = true;
              return voxelize_lattice_host_end_impl(ctx, nullptr, nullptr, results); },
        [&] { tmp.resize((size_t)V * C);
              return mkamd_occupancy_centers_host(ctx, centers, V, coords, N, sigmas, 1, C, nullptr, tmp.data()); });
    if (st) return st;
    if (lattice_done) return MKAMD_OK;
    // in-place max-accumulate, `value > old ? value : old` as occupancy_utils.pyx:61
    const size_t nvals = (size_t)V * C;
    for (size_t i = 0; i < nvals; ++i) {
        const double v = (double)tmp[i];
        if (v > results[i]) results[i] = v;
    }
    return MKAMD_OK;
} MK_API_CATCH

// calculate_occupancy on the HOST: the library's own double-precision implementation (cpu_occupancy.h), no
// context, no device.  Explicit only: nothing in the library or the package takes it on its own.
int mkamd_calculate_occupancy_cpu_threads(const double* centers, int64_t V, const float* coords, int64_t N, const double* sigmas,
                                          int32_t C, double* results, int32_t n_threads)
try {
    if (V < 0 || N < 0 || C <= 0) return fail(MKAMD_EINVAL, "n_centers/n_atoms must be >= 0 and n_channels > 0");
    if (V == 0 || N == 0) return MKAMD_OK;
    if (!centers || !coords || !sigmas || !results) return fail(MKAMD_EINVAL, "centers/coords/sigmas/results pointer is NULL");
    if (N > 0xFFFFFFF0LL) return fail(MKAMD_EINVAL, "more than 2^32 atoms");
    mkamd::cpu::calculate_occupancy(centers, V, coords, N, sigmas, C, results, (int)n_threads);
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_calculate_occupancy_cpu(const double* centers, int64_t V, const float* coords, int64_t N, const double* sigmas,
                                  int32_t C, double* results)
try {
    return mkamd_calculate_occupancy_cpu_threads(centers, V, coords, N, sigmas, C, results, 0);
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// lattice grids (the hot path)
// ---------------------------------------------------------------------------------------------
int mkamd_voxelize_lattice_dev(mkamd_ctx* ctx, int32_t B, const float* d_coords,
                               const int64_t* d_atom_offsets, int64_t total_atoms, const void* d_sigmas,
                               int sigmas_are_f64, int32_t C, const double* d_origins,
                               const int32_t* nvoxels, double voxelsize, const float* d_box,
                               int32_t max_images, float* d_features)
try {
    return mkamd_voxelize_lattice_aug_dev(ctx, B, d_coords, d_atom_offsets, total_atoms, d_sigmas, sigmas_are_f64, C,
                                          d_origins, nvoxels, voxelsize, d_box, max_images, nullptr, d_features);
} MK_API_CATCH

static int voxelize_lattice_dev_impl(mkamd_ctx* ctx, int32_t B, const float* d_coords,
                                     const int64_t* d_atom_offsets, int64_t total_atoms, const void* d_sigmas,
                                     int sigmas_are_f64, int32_t C, const double* d_origins,
                                     const int32_t* nvoxels, double voxelsize, const float* d_box,
                                     int32_t max_images, const double* d_affine, float* d_features, const mkamd_topology* topo,
                                     int32_t topo_first_item = 0)
{
    int st = check_ctx(ctx);
    if (st) return st;
    if (!nvoxels) return fail(MKAMD_EINVAL, "nvoxels pointer is NULL");
    if (B > 0 && (!d_atom_offsets || !d_origins || !d_features)) return fail(MKAMD_EINVAL, "atom_offsets/origins/features pointer is NULL");
    if (total_atoms > 0 && (!d_coords || (!d_sigmas && !topo))) return fail(MKAMD_EINVAL, "coords/sigmas pointer is NULL");
    if (topo && topo->device != ctx->device) return fail(MKAMD_EINVAL, "the topology lives on another device than the context");
    if ((st = ensure_err_flag(ctx))) return st;
    LatticeProblem P;
    P.B = B; P.total_atoms = total_atoms; P.C = C; P.sigmas_f64 = sigmas_are_f64;
    P.nvox[0] = nvoxels[0]; P.nvox[1] = nvoxels[1]; P.nvox[2] = nvoxels[2];
    P.voxelsize = voxelsize; P.pbc = d_box ? 1 : 0; P.max_images = d_box ? max_images : 1;
    P.tile_k = ctx->tile_k; P.force_general = ctx->force_general; P.lds_tier = ctx->lds_tier; P.prepass_mode = ctx->prepass_mode; P.tile_team = ctx->tile_team; P.tile_items = ctx->tile_items; P.exact_redo_list = ctx->exact_redo; P.cover_fold = ctx->cover_fold; P.fine_cells = ctx->fine_cells; P.value_tol = ctx->value_tol; P.direct = ctx->direct; P.seq = ctx->seq_next; ctx->seq_next = 0u;
    P.coords = d_coords; P.atom_offsets = (const long long*)d_atom_offsets; P.sigmas = d_sigmas;
    P.origins = d_origins; P.box = d_box; P.affine = d_affine; P.out = d_features;
    P.topo = topo ? &topo->dev : nullptr;
    P.topo_first_item = topo_first_item;
    std::string err;
    // a promise (mkamd_ctx_promise_inputs) is about the next call of THIS entry point made from outside the library: a host
    // call reaches here through voxelize_lattice_host_begin_impl, which has set the promise aside (its inputs were uploaded
    // on the main stream just now, behind the marker a pipelined pre-pass waits for)
    st = run_lattice(*ctx, P, err);
    ctx->promise = false; ctx->promise_event = nullptr;       // one call's worth
    return run_status(st, err);
}

int mkamd_voxelize_lattice_aug_dev(mkamd_ctx* ctx, int32_t B, const float* d_coords,
                                   const int64_t* d_atom_offsets, int64_t total_atoms, const void* d_sigmas,
                                   int sigmas_are_f64, int32_t C, const double* d_origins,
                                   const int32_t* nvoxels, double voxelsize, const float* d_box,
                                   int32_t max_images, const double* d_affine, float* d_features)
try {
    return voxelize_lattice_dev_impl(ctx, B, d_coords, d_atom_offsets, total_atoms, d_sigmas, sigmas_are_f64, C, d_origins, nvoxels, voxelsize,
                                     d_box, max_images, d_affine, d_features, nullptr);
} MK_API_CATCH

// ---- topology reuse: the frames of a trajectory share everything the pre-pass derives from the sigmas ----
// h_offsets != nullptr: a BATCH handle over the n_items items of those (host) atom offsets, n_atoms = all their atoms
static int topology_create_impl(mkamd_ctx* ctx, const void* d_sigmas, int sigmas_are_f64, int64_t n_atoms, int32_t C, double voxelsize,
                                const int64_t* h_offsets, int32_t n_items, mkamd_topology** out)
{
    if (!out) return fail(MKAMD_EINVAL, "topology out-pointer is NULL");
    *out = nullptr;
    int st = check_ctx(ctx);
    if (st) return st;
    if (n_atoms <= 0 || C <= 0 || !d_sigmas) return fail(MKAMD_EINVAL, "a topology needs n_atoms > 0, n_channels > 0 and the sigmas");
    if (n_atoms > 0x7fffffffLL) return fail(MKAMD_EINVAL, "a topology holds at most 2^31 atoms");
    long long max_item = 0;
    if (h_offsets) {
        if (n_items <= 0 || h_offsets[0] != 0 || h_offsets[n_items] != n_atoms)
            return fail(MKAMD_EINVAL, "a batch topology needs n_items > 0 and atom offsets that start at 0 and end at total_atoms");
        for (int32_t b = 0; b < n_items; ++b) {
            if (h_offsets[b + 1] < h_offsets[b]) return fail(MKAMD_EINVAL, "a batch topology's atom offsets must not decrease");
            max_item = std::max<long long>(max_item, h_offsets[b + 1] - h_offsets[b]);
        }
    }
    const int G = ceil_div(C, CHG);
    const size_t a256 = 255, sig_bytes = (size_t)n_atoms * C * (sigmas_are_f64 ? 8 : 4);
    const size_t o_cw = (sig_bytes + a256) & ~a256, o_ids = (o_cw + (size_t)n_atoms * G * sizeof(uint2) + a256) & ~a256,
                 o_tab = (o_ids + (size_t)n_atoms * G * sizeof(unsigned) + a256) & ~a256, o_flags = o_tab + 256,
                 flag_bytes = (8 + (size_t)G * sizeof(unsigned) + a256) & ~a256,       // flags [2], then the violated-class words [G]
                 o_wide = o_flags + flag_bytes,
                 o_offs = (o_wide + (size_t)n_atoms * sizeof(unsigned) + a256) & ~a256,
                 total = o_offs + (h_offsets ? (size_t)n_items + 1 : 0) * sizeof(long long);
    mkamd_topology* t = new mkamd_topology();
    t->device = ctx->device;
    hipError_t e = hipMalloc(&t->mem, total);
    if (e != hipSuccess) { delete t; return hip_fail(e, "hipMalloc(topology)"); }
    char* m = (char*)t->mem;
    auto drop = [&](int code) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(t->mem); delete t; return code; };
    if ((e = hipMemcpyAsync(m, d_sigmas, sig_bytes, hipMemcpyDeviceToDevice, ctx->stream)) != hipSuccess) return drop(hip_fail(e, "hipMemcpyAsync(topology sigmas)"));
    if ((e = hipMemsetAsync(m + o_flags, 0, flag_bytes, ctx->stream)) != hipSuccess) return drop(hip_fail(e, "hipMemsetAsync(topology flags)"));
    std::string err;
    st = run_topology_build(*ctx, m, sigmas_are_f64, (long long)n_atoms, C, voxelsize, (uint2*)(m + o_cw), (unsigned*)(m + o_ids),
                            (unsigned*)(m + o_tab), (int*)(m + o_flags), (unsigned*)(m + o_wide), err, (unsigned*)(m + o_flags + 8));
    if (st) return drop(run_status(st, err));
    unsigned table[CLS_TABLE_WORDS];
    std::vector<unsigned> fl(2 + (size_t)G, 0u);                     // the flags and the violated-class words: one read-back
    if ((e = hipMemcpyAsync(table, m + o_tab, sizeof table, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(fl.data(), m + o_flags, fl.size() * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return drop(hip_fail(e, "topology read-back"));
    const int flags = (int)fl[0];
    const unsigned n_wide = fl[1];
    t->h_cover.resize((size_t)G);
    for (int gq = 0; gq < G; ++gq) t->h_cover[gq] = ~fl[2 + gq] & 0xfffeu;
    std::vector<unsigned>& wl = t->h_wide;                           // (a batch handle keeps the list on the host too)
    wl.resize(n_wide);
    if (n_wide > 1u || (n_wide != 0u && h_offsets)) {
        // the list arrives in the order the lanes' atomics did: sorted here, once, so that a handle is the same whenever it is built
        if ((e = hipMemcpyAsync(wl.data(), m + o_wide, (size_t)n_wide * 4, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return drop(hip_fail(e, "topology read-back (wide atoms)"));
        std::sort(wl.begin(), wl.end());
        if ((e = hipMemcpyAsync(m + o_wide, wl.data(), (size_t)n_wide * 4, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return drop(hip_fail(e, "topology write-back (wide atoms)"));
    }
    if (table[CLS_OVERFLOW] != CLS_EMPTY)
        return drop(fail(MKAMD_EINVAL, "more than 15 distinct sigma values: no class ids to reuse (use the plain entry point)"));
    t->dev.n = (long long)n_atoms; t->dev.C = C; t->dev.G = G; t->dev.sigmas_f64 = sigmas_are_f64; t->dev.voxelsize = voxelsize;
    t->dev.sigmas = m; t->dev.cw = (const uint2*)(m + o_cw); t->dev.ids = (const unsigned*)(m + o_ids); t->dev.table = (const unsigned*)(m + o_tab);
    t->dev.overflow = false; t->dev.wide = (flags & 1) != 0;
    t->dev.wide_list = (const unsigned*)(m + o_wide); t->dev.n_wide = n_wide;
    t->dev.cover_violated = (const unsigned*)(m + o_flags + 8); t->dev.h_cover = t->h_cover.data();
    if (h_offsets) {
        t->h_offsets.assign(h_offsets, h_offsets + n_items + 1);
        if ((e = hipMemcpyAsync(m + o_offs, t->h_offsets.data(), ((size_t)n_items + 1) * sizeof(long long), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
            (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return drop(hip_fail(e, "topology upload (atom offsets)"));
        t->dev.batch = true; t->dev.n_items = n_items; t->dev.max_item = max_item;
        t->dev.offsets = (const long long*)(m + o_offs); t->dev.h_offsets = t->h_offsets.data(); t->dev.h_wide_list = t->h_wide.data();
    }
    *out = t;
    return MKAMD_OK;
}

int mkamd_topology_create_dev(mkamd_ctx* ctx, const void* d_sigmas, int sigmas_are_f64, int64_t n_atoms, int32_t C, double voxelsize,
                              mkamd_topology** out)
try {
    return topology_create_impl(ctx, d_sigmas, sigmas_are_f64, n_atoms, C, voxelsize, nullptr, 0, out);
} MK_API_CATCH

// ---- a batch handle: the same for a resident, ragged batch of different molecules (include/mkamd_voxel.h (3c)) ----
int mkamd_topology_create_batch_dev(mkamd_ctx* ctx, const void* d_sigmas, int sigmas_are_f64, int64_t total_atoms, int32_t C, double voxelsize,
                                    const int64_t* atom_offsets_host, int32_t n_items, mkamd_topology** out)
try {
    if (!atom_offsets_host) { if (out) *out = nullptr; return fail(MKAMD_EINVAL, "a batch topology needs the batch's atom offsets (host memory)"); }
    return topology_create_impl(ctx, d_sigmas, sigmas_are_f64, total_atoms, C, voxelsize, atom_offsets_host, n_items, out);
} MK_API_CATCH

int mkamd_topology_create_batch_host(mkamd_ctx* ctx, const void* sigmas, int sigmas_are_f64, int64_t total_atoms, int32_t C, double voxelsize,
                                     const int64_t* atom_offsets_host, int32_t n_items, mkamd_topology** out)
try {
    if (!out) return fail(MKAMD_EINVAL, "topology out-pointer is NULL");
    *out = nullptr;
    int st = check_ctx(ctx);
    if (st) return st;
    if (total_atoms <= 0 || C <= 0 || !sigmas) return fail(MKAMD_EINVAL, "a topology needs n_atoms > 0, n_channels > 0 and the sigmas");
    void* ds = nullptr;
    const size_t bytes = (size_t)total_atoms * C * (sigmas_are_f64 ? 8 : 4);
    if ((st = ctx->ensure(WS_H_SIGMAS, bytes, &ds))) return st;
    HIP_TRY(hipMemcpyAsync(ds, sigmas, bytes, hipMemcpyHostToDevice, ctx->stream));
    return mkamd_topology_create_batch_dev(ctx, ds, sigmas_are_f64, total_atoms, C, voxelsize, atom_offsets_host, n_items, out);
} MK_API_CATCH

int mkamd_topology_create_host(mkamd_ctx* ctx, const void* sigmas, int sigmas_are_f64, int64_t n_atoms, int32_t C, double voxelsize,
                               mkamd_topology** out)
try {
    if (!out) return fail(MKAMD_EINVAL, "topology out-pointer is NULL");
    *out = nullptr;
    int st = check_ctx(ctx);
    if (st) return st;
    if (n_atoms <= 0 || C <= 0 || !sigmas) return fail(MKAMD_EINVAL, "a topology needs n_atoms > 0, n_channels > 0 and the sigmas");
    void* ds = nullptr;
    const size_t bytes = (size_t)n_atoms * C * (sigmas_are_f64 ? 8 : 4);
    if ((st = ctx->ensure(WS_H_SIGMAS, bytes, &ds))) return st;
    HIP_TRY(hipMemcpyAsync(ds, sigmas, bytes, hipMemcpyHostToDevice, ctx->stream));
    return mkamd_topology_create_dev(ctx, ds, sigmas_are_f64, n_atoms, C, voxelsize, out);
} MK_API_CATCH

int mkamd_topology_destroy(mkamd_ctx* ctx, mkamd_topology* topo)
try {
    if (!topo) return MKAMD_OK;
    if (ctx) {                                   // calls that read the handle may still be in flight on the context's streams
        (void)hipSetDevice(ctx->device);
        if (ctx->side_stream) (void)hipStreamSynchronize(ctx->side_stream);
        (void)hipStreamSynchronize(ctx->main_stream);
    } else {
        (void)hipSetDevice(topo->device);
        (void)hipDeviceSynchronize();
    }
    if (topo->mem) (void)hipFree(topo->mem);
    delete topo;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_topology_info(const mkamd_topology* topo, int64_t* n_atoms, int32_t* n_channels, double* voxelsize, int32_t* has_wide_sigmas)
try {
    if (!topo) return fail(MKAMD_EINVAL, "topology is NULL");
    if (n_atoms) *n_atoms = (int64_t)topo->dev.n;
    if (n_channels) *n_channels = topo->dev.C;
    if (voxelsize) *voxelsize = topo->dev.voxelsize;
    if (has_wide_sigmas) *has_wide_sigmas = topo->dev.wide ? 1 : 0;
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_voxelize_lattice_topo_dev(mkamd_ctx* ctx, int32_t B, const float* d_coords, const int64_t* d_atom_offsets, int64_t total_atoms,
                                    const mkamd_topology* topo, const double* d_origins, const int32_t* nvoxels, double voxelsize,
                                    const float* d_box, int32_t max_images, const double* d_affine, float* d_features)
try {
    if (!topo) return fail(MKAMD_EINVAL, "topology is NULL");
    return voxelize_lattice_dev_impl(ctx, B, d_coords, d_atom_offsets, total_atoms, nullptr, topo->dev.sigmas_f64, topo->dev.C, d_origins, nvoxels,
                                     voxelsize, d_box, max_images, d_affine, d_features, topo);
} MK_API_CATCH

int mkamd_voxelize_lattice_topo_range_dev(mkamd_ctx* ctx, int32_t B, const float* d_coords, const int64_t* d_atom_offsets, int64_t total_atoms,
                                          const mkamd_topology* topo, int32_t first_item, const double* d_origins, const int32_t* nvoxels,
                                          double voxelsize, const float* d_box, int32_t max_images, const double* d_affine, float* d_features)
try {
    if (!topo) return fail(MKAMD_EINVAL, "topology is NULL");
    if (!topo->dev.batch) return fail(MKAMD_EINVAL, "a range of items is a call on a batch topology (mkamd_topology_create_batch_*)");
    return voxelize_lattice_dev_impl(ctx, B, d_coords, d_atom_offsets, total_atoms, nullptr, topo->dev.sigmas_f64, topo->dev.C, d_origins, nvoxels,
                                     voxelsize, d_box, max_images, d_affine, d_features, topo, first_item);
} MK_API_CATCH

int mkamd_topology_cover_mask(const mkamd_topology* topo, int32_t group, uint32_t* mask)
try {
    if (!topo || !mask) return fail(MKAMD_EINVAL, "topology / mask is NULL");
    if (group < 0 || group >= topo->dev.G) return fail(MKAMD_EINVAL, "not a channel group of the topology");
    *mask = topo->h_cover[(size_t)group];
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_topology_batch_info(const mkamd_topology* topo, int32_t* n_items, int64_t* longest_item)
try {
    if (!topo) return fail(MKAMD_EINVAL, "topology is NULL");
    if (n_items) *n_items = topo->dev.batch ? topo->dev.n_items : 0;
    if (longest_item) *longest_item = topo->dev.batch ? (int64_t)topo->dev.max_item : 0;
    return MKAMD_OK;
} MK_API_CATCH

// Would a call on items [first_item, + n_items) of a batch handle use it -- take the count / scan / fill chain in front of the tile
// kernels -- or be served as a plain call on the handle's sigma copy?  The path is chosen where every call's is (choose_lattice_path,
// settle_lattice_path), with the context's settings as they are now; `promised`: the call will come with mkamd_ctx_promise_inputs.
int mkamd_topology_batch_used(mkamd_ctx* ctx, const mkamd_topology* topo, int32_t first_item, int32_t n_items, const int32_t* nvoxels,
                              int32_t periodic, int32_t max_images, int32_t promised, int32_t* used)
try {
    if (!ctx || !topo || !nvoxels || !used) return fail(MKAMD_EINVAL, "ctx / topology / nvoxels / used is NULL");
    *used = 0;
    const TopologyDev& t = topo->dev;
    if (!t.batch) return fail(MKAMD_EINVAL, "not a batch topology");
    if (first_item < 0 || n_items < 0 || (long long)first_item + n_items > (long long)t.n_items) return fail(MKAMD_EINVAL, "not a range of the batch topology's items");
    LatticeProblem P;
    P.B = n_items; P.total_atoms = t.h_offsets[first_item + n_items] - t.h_offsets[first_item]; P.C = t.C; P.sigmas_f64 = t.sigmas_f64;
    P.nvox[0] = nvoxels[0]; P.nvox[1] = nvoxels[1]; P.nvox[2] = nvoxels[2];
    P.voxelsize = t.voxelsize; P.pbc = periodic ? 1 : 0; P.max_images = periodic ? max_images : 1;
    P.tile_k = ctx->tile_k; P.force_general = ctx->force_general; P.lds_tier = ctx->lds_tier; P.prepass_mode = ctx->prepass_mode; P.tile_team = ctx->tile_team; P.tile_items = ctx->tile_items; P.exact_redo_list = ctx->exact_redo; P.cover_fold = ctx->cover_fold; P.fine_cells = ctx->fine_cells; P.value_tol = ctx->value_tol; P.direct = ctx->direct;
    P.topo = &t; P.topo_first_item = first_item;
    GridDesc g;
    std::string err;
    int st = plan_lattice(P, g, err);
    if (st) return fail(st, err);
    if (P.B == 0 || g.V == 0 || P.total_atoms == 0 || g.force_general || g.reach_tau > 0.f) return MKAMD_OK;
    const bool may_pipeline = (ctx->pipelining || promised) && ctx->side_stream && !ctx->pipeline_broken;
    LatticePath L = choose_lattice_path(P, g, may_pipeline);
    settle_lattice_path(L, P, g, may_pipeline && L.pipelined_wanted);
    *used = L.topo() ? 1 : 0;
    return MKAMD_OK;
} MK_API_CATCH

// End of a small synchronous call (tens of microseconds of GPU work): poll the stream instead of blocking on it -- the
// blocking wait's wake-up costs more than the polls; a call that is still running after ~2 000 polls blocks after all.
// The runtime answers a stream query with a marker packet of its own when the stream's last command is a kernel -- and that
// packet then takes its ~5-10 us to retire while the caller polls.  A small host call therefore records an event right
// behind its last launch (it retires while the host is busy with the result) and asks the EVENT.
static hipError_t wait_for_small_call(hipStream_t s, hipEvent_t done = nullptr)
{
    for (int i = 0; i < 2000; ++i) {
        const hipError_t e = done ? hipEventQuery(done) : hipStreamQuery(s);
        if (e != hipErrorNotReady) {
            if (i != 0 && e == hipSuccess) (void)hipGetLastError();    // "not ready" is an answer, not an error to find later
            return e;
        }
    }
    (void)hipGetLastError();
    return done ? hipEventSynchronize(done) : hipStreamSynchronize(s);
}

// float32 -> float64 over the result of a call (the drop-in path returns the reference's float64 [V, C]): the baseline
// x86-64 build converts two values per instruction; where the host has AVX2 (checked at run time) eight
__attribute__((target("avx2"))) static void widen_avx2(const float* __restrict__ src, double* __restrict__ dst, size_t n)
{
    for (size_t i = 0; i < n; ++i) dst[i] = (double)src[i];
}
// AVX-512 hosts: 16 values per trip, the source (device-written pinned memory: it comes from DRAM) prefetched ahead
__attribute__((target("avx512f"))) static void widen_avx512(const float* __restrict__ src, double* __restrict__ dst, size_t n)
{
    size_t i = 0;
    for (; i + 16 <= n; i += 16) {
        __builtin_prefetch(src + i + 512, 0, 0);
        typedef float v16f __attribute__((vector_size(64), aligned(4)));
        typedef double v8d __attribute__((vector_size(64), aligned(8)));
        typedef float v8f __attribute__((vector_size(32)));
        const v16f v = *(const v16f*)(src + i);
        const v8f lo = __builtin_shufflevector(v, v, 0, 1, 2, 3, 4, 5, 6, 7), hi = __builtin_shufflevector(v, v, 8, 9, 10, 11, 12, 13, 14, 15);
        *(v8d*)(dst + i) = __builtin_convertvector(lo, v8d);
        *(v8d*)(dst + i + 8) = __builtin_convertvector(hi, v8d);
    }
    for (; i < n; ++i) dst[i] = (double)src[i];
}
static void widen(const float* __restrict__ src, double* __restrict__ dst, size_t n)
{
    static const bool avx512 = __builtin_cpu_supports("avx512f") && getenv("MKAMD_NO_AVX512") == nullptr;
    if (avx512) { widen_avx512(src, dst, n); return; }
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) { widen_avx2(src, dst, n); return; }
    for (size_t i = 0; i < n; ++i) dst[i] = (double)src[i];
}

// `features64` != NULL: the caller wants the reference's float64 [B,V,C] (voxeldescriptors.py:531); the widening is
// done here, in the pass that takes the results out of the pinned buffer anyway, instead of in a second pass in numpy

// A host call in two halves: `begin` checks, ships the inputs and enqueues the kernels; `end` waits and takes the result
// out.  The one-piece entry points run them back to back; the drop-in getVoxelDescriptors does its own host work (the copy
// of the cached voxel centres, 330 KB for a 24^3 grid) between the two, while the device computes.
static int voxelize_lattice_host_begin_impl(mkamd_ctx* ctx, int32_t B, const float* coords, const int64_t* atom_offsets,
                                            const void* sigmas, int sigmas_are_f64, int32_t C, const double* origins,
                                            const int32_t* nvoxels, double voxelsize, const float* box, int32_t max_images)
{
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (ctx->pending.active) {                                      // a begin without its end: that call is abandoned
        (void)hipStreamSynchronize(ctx->stream);
        ctx->pending.active = false;
    }
    if (B < 0 || C <= 0) return fail(MKAMD_EINVAL, "n_items must be >= 0 and n_channels > 0");
    if (!nvoxels) return fail(MKAMD_EINVAL, "nvoxels pointer is NULL");
    if (nvoxels[0] < 0 || nvoxels[1] < 0 || nvoxels[2] < 0) return fail(MKAMD_EINVAL, "nvoxels must be >= 0");
    const long long V = (long long)nvoxels[0] * nvoxels[1] * nvoxels[2];
    if (B == 0 || V == 0) { ctx->pending = mkamd_ctx::PendingHostCall{}; ctx->pending.active = true; return MKAMD_OK; }
    if (!atom_offsets || !origins) return fail(MKAMD_EINVAL, "atom_offsets/origins pointer is NULL");
    if (atom_offsets[0] != 0) return fail(MKAMD_EINVAL, "atom_offsets[0] must be 0");
    for (int b = 0; b < B; ++b)
        if (atom_offsets[b + 1] < atom_offsets[b]) return fail(MKAMD_EINVAL, "atom_offsets must be non-decreasing");
    const int64_t N = atom_offsets[B];
    if (N > 0 && (!coords || !sigmas)) return fail(MKAMD_EINVAL, "coords/sigmas pointer is NULL");
    if (box && max_images <= 0) {
        std::string err;
        const int nv[3] = {nvoxels[0], nvoxels[1], nvoxels[2]};
        max_images = max_images_from_boxes(box, B, nv, voxelsize, err);
        if (max_images < 0) return fail(MKAMD_EBOX, err);
    }
    const size_t sz = sigmas_are_f64 ? 8 : 4;
    const size_t out_bytes = (size_t)B * (size_t)V * (size_t)C * 4;
    void *dx = nullptr, *ds = nullptr, *doff = nullptr, *dorg = nullptr, *dbox = nullptr, *dout = nullptr;
    // small results (the drop-in path: one molecule per call): the kernels store straight into pinned host memory
    // mapped into the device's address space -- the stores cross PCIe while the kernel runs, and the copy engine's
    // start-up latency (~15 us before a ~13 us copy on the 3PTB grid) disappears
    constexpr size_t OUT_HOST_BYTES = (size_t)1 << 20;
    bool mapped_out = out_bytes <= OUT_HOST_BYTES;
    if (mapped_out && !ctx->out_host) {
        if (hipHostMalloc(&ctx->out_host, OUT_HOST_BYTES, hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer(&ctx->out_host_dev, ctx->out_host, 0) != hipSuccess) {
            if (ctx->out_host) (void)hipHostFree(ctx->out_host);
            ctx->out_host = nullptr;
            (void)hipGetLastError();
            mapped_out = false;
        }
    }
    if (mapped_out) dout = ctx->out_host_dev;
    else if ((st = ctx->ensure(WS_H_OUT, out_bytes, &dout))) return st;
    // small calls (the drop-in path: one molecule per call) are latency-bound: pack the inputs into one pinned
    // buffer and ship them with ONE asynchronous copy instead of five staged pageable ones
    const size_t a16 = 15;
    const size_t o_x = 0, o_s = (o_x + (size_t)N * 12 + a16) & ~a16, o_off = (o_s + (size_t)N * C * sz + a16) & ~a16,
                 o_org = (o_off + (size_t)(B + 1) * 8 + a16) & ~a16, o_box = (o_org + (size_t)B * 24 + a16) & ~a16,
                 packed_bytes = o_box + (box ? (size_t)B * 12 : 0);
    constexpr size_t STAGE_BYTES = (size_t)1 << 20;
    bool packed = packed_bytes <= STAGE_BYTES;
    if (packed && !ctx->stage_host) {
        if (hipHostMalloc(&ctx->stage_host, STAGE_BYTES, hipHostMallocMapped) == hipSuccess) {
            ctx->stage_cap = STAGE_BYTES;
            if (hipHostGetDevicePointer(&ctx->stage_host_dev, ctx->stage_host, 0) != hipSuccess) { ctx->stage_host_dev = nullptr; (void)hipGetLastError(); }
        } else { ctx->stage_host = nullptr; packed = false; }
    }
    if (packed) {
        void* dstage = nullptr;
        if ((st = ctx->ensure(WS_H_STAGE, packed_bytes, &dstage))) return st;
        char* h = (char*)ctx->stage_host;       // free again: every _host call ends with a stream synchronize
        if (N > 0) { memcpy(h + o_x, coords, (size_t)N * 12); memcpy(h + o_s, sigmas, (size_t)N * C * sz); }
        memcpy(h + o_off, atom_offsets, (size_t)(B + 1) * 8);
        memcpy(h + o_org, origins, (size_t)B * 24);
        if (box) memcpy(h + o_box, box, (size_t)B * 12);
        // up to 256 KiB the kernels read the packed inputs in place over PCIe (each byte is read once, by the binning):
        // cheaper than waking the copy engine (~8 us + ~8 us before the first kernel starts on the 3PTB call)
        if (ctx->stage_host_dev != nullptr && packed_bytes <= ((size_t)256 << 10)) dstage = ctx->stage_host_dev;
        else HIP_TRY(hipMemcpyAsync(dstage, h, packed_bytes, hipMemcpyHostToDevice, ctx->stream));
        dx = (char*)dstage + o_x; ds = (char*)dstage + o_s; doff = (char*)dstage + o_off; dorg = (char*)dstage + o_org;
        dbox = (char*)dstage + o_box;
    } else {
        if ((st = ctx->ensure(WS_H_COORDS, (size_t)N * 12, &dx))) return st;
        if ((st = ctx->ensure(WS_H_SIGMAS, (size_t)N * C * sz, &ds))) return st;
        if ((st = ctx->ensure(WS_H_OFFSETS, (size_t)(B + 1) * 8, &doff))) return st;
        if ((st = ctx->ensure(WS_H_ORIGINS, (size_t)B * 24, &dorg))) return st;
        if (box && (st = ctx->ensure(WS_H_BOX, (size_t)B * 12, &dbox))) return st;
        if (N > 0) {
            HIP_TRY(hipMemcpyAsync(dx, coords, (size_t)N * 12, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(ds, sigmas, (size_t)N * C * sz, hipMemcpyHostToDevice, ctx->stream));
        }
        HIP_TRY(hipMemcpyAsync(doff, atom_offsets, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dorg, origins, (size_t)B * 24, hipMemcpyHostToDevice, ctx->stream));
        if (box) HIP_TRY(hipMemcpyAsync(dbox, box, (size_t)B * 12, hipMemcpyHostToDevice, ctx->stream));
    }
    // the per-item pre-pass gives every item ONE workgroup: here the offsets are visible, so a ragged batch whose
    // average is small but which holds a huge item is kept on the kernel chain (automatic mode only)
    long long biggest = 0;
    for (int b = 0; b < B; ++b) biggest = std::max<long long>(biggest, atom_offsets[b + 1] - atom_offsets[b]);
    const int saved_mode = ctx->prepass_mode;
    if (saved_mode < 0 && biggest > 16384) ctx->prepass_mode = 0;
    // small results: the host pass over them (copy / float64 widening) starts when the TILE kernel is done (k_tail says so in
    // the host-visible feedback words as it starts), not when the stream is -- see FB_TILES_DONE
    unsigned seq = 0u;
    if (mapped_out && ctx->fb_host != nullptr) { if (++ctx->seq_counter == 0u) ctx->seq_counter = 1u; seq = ctx->seq_counter; }
    ctx->seq_next = seq;
    ctx->tail_reports = false;
    // an outstanding promise is about the next DEVICE call of whoever made it, not about this host call (whose inputs went up
    // on the main stream a moment ago: a pre-pass on the side stream would race the upload): set aside, handed back after
    const bool saved_promise = ctx->promise;
    const hipEvent_t saved_promise_event = ctx->promise_event;
    ctx->promise = false; ctx->promise_event = nullptr;
    st = mkamd_voxelize_lattice_dev(ctx, B, (const float*)dx, (const int64_t*)doff, N, ds, sigmas_are_f64, C,
                                    (const double*)dorg, nvoxels, voxelsize, box ? (const float*)dbox : nullptr,
                                    max_images, (float*)dout);
    ctx->promise = saved_promise; ctx->promise_event = saved_promise_event;
    ctx->prepass_mode = saved_mode;
    ctx->seq_next = 0u;
    if (st) return st;
    ctx->pending.active = true; ctx->pending.out_bytes = out_bytes; ctx->pending.mapped_out = mapped_out; ctx->pending.seq = seq;
    ctx->pending.dout = dout;
    ctx->pending.done = nullptr;
    if (mapped_out) {
        if (!ctx->ev_host_done && hipEventCreateWithFlags(&ctx->ev_host_done, hipEventDisableTiming) != hipSuccess) { ctx->ev_host_done = nullptr; (void)hipGetLastError(); }
        if (ctx->ev_host_done && hipEventRecord(ctx->ev_host_done, ctx->stream) == hipSuccess) ctx->pending.done = ctx->ev_host_done;
        else (void)hipGetLastError();
    }
    return MKAMD_OK;
}

static int voxelize_lattice_host_end_impl(mkamd_ctx* ctx, float* features, double* features64, double* max_into)
{
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (!ctx->pending.active) return fail(MKAMD_EINVAL, "no host call was begun on this context");
    const size_t out_bytes = ctx->pending.out_bytes;
    const bool mapped_out = ctx->pending.mapped_out;
    const unsigned seq = ctx->pending.seq;
    void* const dout = ctx->pending.dout;
    const hipEvent_t done = ctx->pending.done;
    ctx->pending.active = false;
    if (out_bytes == 0) return MKAMD_OK;                            // no items / no voxels
    if (!features && !features64 && !max_into) { (void)hipStreamSynchronize(ctx->stream); return fail(MKAMD_EINVAL, "features pointer is NULL"); }
    const size_t nvals = out_bytes / 4;
    if (max_into) {
        // calculate_occupancy's contract (occupancy_utils.pyx:61): results[i] = max(results[i], value) -- straight out of the
        // mapped result buffer, once the whole call is done (an early pass could not be repeated: a maximum does not undo)
        const float* src = (const float*)ctx->out_host;
        if (!mapped_out) {
            ctx->f32_stage.resize(nvals);
            HIP_TRY(hipMemcpyAsync(ctx->f32_stage.data(), dout, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
            src = ctx->f32_stage.data();
        }
        HIP_TRY(mapped_out ? wait_for_small_call(ctx->stream, done) : hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < nvals; ++i) {
            const double v = (double)src[i];
            if (v > max_into[i]) max_into[i] = v;
        }
        return collect_async_errors(ctx);
    }
    // wait for "tile kernel done" (a read of host memory per poll; gives up after ~1 ms: the stream wait below covers it)
    bool early = false;
    static const bool no_early = [] { const char* e = std::getenv("MKAMD_NO_EARLY_PASS"); return e && e[0] == '1'; }();   // debugging switch
    if (seq != 0u && ctx->tail_reports && !no_early) {
        const volatile unsigned* fb = ctx->fb_host;
        for (int i = 0; i < 400000 && !early; ++i) early = fb[FB_TILES_DONE] == seq;
        // the result buffer is coherent, uncached host memory the tile kernel wrote before k_tail (same stream) released its
        // system-scope fence and raised the word: nothing of the result may be read ahead of the poll
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!mapped_out) prefault_big_result(features64 ? (void*)features64 : (void*)features, features64 ? out_bytes * 2 : out_bytes);
    if (features64) {
        const float* src = (const float*)ctx->out_host;
        if (!mapped_out) {                                    // big result: through a host staging vector
            ctx->f32_stage.resize(nvals);
            HIP_TRY(hipMemcpyAsync(ctx->f32_stage.data(), dout, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
            src = ctx->f32_stage.data();
        }
        if (early) {
            widen(src, features64, nvals);                          // ... while k_tail runs and the stream signals its completion
            HIP_TRY(wait_for_small_call(ctx->stream, done));
            if (((const volatile unsigned*)ctx->fb_host)[FB_TAIL_WROTE] == seq) widen(src, features64, nvals);     // k_tail changed values (rare): once more
        } else {
            HIP_TRY(mapped_out ? wait_for_small_call(ctx->stream, done) : hipStreamSynchronize(ctx->stream));
            widen(src, features64, nvals);
        }
        st = collect_async_errors(ctx);
        return st;
    }
    if (!mapped_out) HIP_TRY(hipMemcpyAsync(features, dout, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (early) {
        memcpy(features, ctx->out_host, out_bytes);
        HIP_TRY(wait_for_small_call(ctx->stream, done));
        if (((const volatile unsigned*)ctx->fb_host)[FB_TAIL_WROTE] == seq) memcpy(features, ctx->out_host, out_bytes);
        return collect_async_errors(ctx);
    }
    HIP_TRY(mapped_out ? wait_for_small_call(ctx->stream, done) : hipStreamSynchronize(ctx->stream));
    if (mapped_out) memcpy(features, ctx->out_host, out_bytes);
    return collect_async_errors(ctx);
}

static int voxelize_lattice_host_impl(mkamd_ctx* ctx, int32_t B, const float* coords, const int64_t* atom_offsets,
                                      const void* sigmas, int sigmas_are_f64, int32_t C, const double* origins,
                                      const int32_t* nvoxels, double voxelsize, const float* box,
                                      int32_t max_images, float* features, double* features64)
{
    if (ctx && B > 0 && nvoxels && nvoxels[0] > 0 && nvoxels[1] > 0 && nvoxels[2] > 0 && !features && !features64)
        return fail(MKAMD_EINVAL, "atom_offsets/origins/features pointer is NULL");
    const int st = voxelize_lattice_host_begin_impl(ctx, B, coords, atom_offsets, sigmas, sigmas_are_f64, C, origins, nvoxels, voxelsize, box, max_images);
    if (st) return st;
    return voxelize_lattice_host_end_impl(ctx, features, features64, nullptr);
}

int mkamd_voxelize_lattice_host_begin(mkamd_ctx* ctx, int32_t B, const float* coords, const int64_t* atom_offsets,
                                      const void* sigmas, int sigmas_are_f64, int32_t C, const double* origins,
                                      const int32_t* nvoxels, double voxelsize, const float* box, int32_t max_images)
try {
    return voxelize_lattice_host_begin_impl(ctx, B, coords, atom_offsets, sigmas, sigmas_are_f64, C, origins, nvoxels, voxelsize, box, max_images);
} MK_API_CATCH

int mkamd_voxelize_lattice_host_end(mkamd_ctx* ctx, float* features, double* features_f64, uint64_t n_values)
try {
    if (features && features_f64) return fail(MKAMD_EINVAL, "pass ONE result array: float32 or float64");
    // the array the caller brings must hold exactly what the pending call produced: the library writes B*V*C values into it
    if (ctx && ctx->pending.active && ctx->pending.out_bytes / 4 != (size_t)n_values) {
        (void)hipStreamSynchronize(ctx->main_stream);
        ctx->pending.active = false;
        return fail(MKAMD_EINVAL, "the result array does not hold n_items * n_voxels * n_channels values (the pending call is abandoned)");
    }
    return voxelize_lattice_host_end_impl(ctx, features, features_f64, nullptr);
} MK_API_CATCH

int mkamd_voxelize_lattice_host(mkamd_ctx* ctx, int32_t B, const float* coords, const int64_t* atom_offsets,
                                const void* sigmas, int sigmas_are_f64, int32_t C, const double* origins,
                                const int32_t* nvoxels, double voxelsize, const float* box,
                                int32_t max_images, float* features)
try {
    return voxelize_lattice_host_impl(ctx, B, coords, atom_offsets, sigmas, sigmas_are_f64, C, origins, nvoxels, voxelsize, box,
                                      max_images, features, nullptr);
} MK_API_CATCH

int mkamd_voxelize_lattice_host_f64(mkamd_ctx* ctx, int32_t B, const float* coords, const int64_t* atom_offsets,
                                    const void* sigmas, int sigmas_are_f64, int32_t C, const double* origins,
                                    const int32_t* nvoxels, double voxelsize, const float* box,
                                    int32_t max_images, double* features)
try {
    return voxelize_lattice_host_impl(ctx, B, coords, atom_offsets, sigmas, sigmas_are_f64, C, origins, nvoxels, voxelsize, box,
                                      max_images, nullptr, features);
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// lattice centres
// ---------------------------------------------------------------------------------------------
int mkamd_grid_centers_dev(mkamd_ctx* ctx, const double* bb_min, const int32_t* nvoxels, double voxelsize,
                           double* d_centers)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (!bb_min || !nvoxels) return fail(MKAMD_EINVAL, "bb_min/nvoxels pointer is NULL");
    const int nv[3] = {nvoxels[0], nvoxels[1], nvoxels[2]};
    std::string err;
    st = run_grid_centers(*ctx, bb_min, nv, voxelsize, d_centers, err);
    return run_status(st, err);
} MK_API_CATCH

int mkamd_grid_centers_host(mkamd_ctx* ctx, const double* bb_min, const int32_t* nvoxels, double voxelsize,
                            double* centers)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (!bb_min || !nvoxels) return fail(MKAMD_EINVAL, "bb_min/nvoxels pointer is NULL");
    if (nvoxels[0] < 0 || nvoxels[1] < 0 || nvoxels[2] < 0) return fail(MKAMD_EINVAL, "nvoxels must be >= 0");
    const long long V = (long long)nvoxels[0] * nvoxels[1] * nvoxels[2];
    if (V == 0) return MKAMD_OK;
    if (!centers) return fail(MKAMD_EINVAL, "centers pointer is NULL");
    void* dc = nullptr;
    if ((st = ctx->ensure(WS_H_CENTERS, (size_t)V * 24, &dc))) return st;
    if ((st = mkamd_grid_centers_dev(ctx, bb_min, nvoxels, voxelsize, (double*)dc))) return st;
    HIP_TRY(hipMemcpyAsync(centers, dc, (size_t)V * 24, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_frames_to_items_dev(mkamd_ctx* ctx, void* hip_stream, const float* d_src, int64_t rows, int64_t src_pitch,
                                         int64_t n_frames, float scale, float* d_dst)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (rows < 0 || n_frames < 0 || src_pitch < n_frames) return fail(MKAMD_EINVAL, "rows / n_frames must be >= 0 and src_pitch >= n_frames");
    if (rows == 0 || n_frames == 0) return MKAMD_OK;
    if (!d_src || !d_dst) return fail(MKAMD_EINVAL, "NULL pointer");
    const long long tiles = ((n_frames + 63) / 64) * ((rows + 63) / 64);
    if (tiles > 0x7ffffff0LL) return fail(MKAMD_EINVAL, "too many tiles (rows x frames / 4096 >= 2^31)");
    hipLaunchKernelGGL(mkamd::k_frames_to_items, dim3((unsigned)(((tiles + 7) / 8) * 8)), dim3(256), 0, (hipStream_t)hip_stream,
                       d_src, (long long)rows, (long long)src_pitch, (long long)n_frames, scale, d_dst);
    HIP_TRY(hipGetLastError());
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_copy_to_host(mkamd_ctx* ctx, void* host_dst, const void* device_src, uint64_t bytes)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (bytes == 0) return MKAMD_OK;
    if (!host_dst || !device_src) return fail(MKAMD_EINVAL, "NULL pointer");
    HIP_TRY(hipMemcpyAsync(host_dst, device_src, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_copy_dev(mkamd_ctx* ctx, void* device_dst, const void* device_src, uint64_t bytes)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (bytes == 0) return MKAMD_OK;
    if (!device_dst || !device_src) return fail(MKAMD_EINVAL, "NULL pointer");
    HIP_TRY(hipMemcpyAsync(device_dst, device_src, (size_t)bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_prefault(void* buffer, uint64_t bytes)
try {
    if (!buffer) return MKAMD_OK;
    const int nt = (int)std::min<unsigned>(32u, std::max(1u, std::thread::hardware_concurrency()));
    mkamd::xtc::prefault_output(static_cast<float*>(buffer), (size_t)bytes / sizeof(float), nt);
    return MKAMD_OK;
} catch (...) { return MKAMD_OK; }

// The lattice test of moleculekit_amd/voxeldescriptors.py::_recognise_lattice_numpy in two passes over the array instead
// of a dozen numpy temporaries: axis lengths from the first place z (then y, at stride nz) stops increasing, one common
// positive step, then every centre against fl64(index * step) + centre 0 with the tolerance 1e-9 * max(1, max |c|).
extern "C" int mkamd_lattice_from_centers(const double* c, int64_t V, double* bb_min, int32_t* nvoxels, double* voxelsize)
try {
    return mkamd::lattice_from_centers(c, (long long)V, bb_min, nvoxels, voxelsize) ? 1 : 0;
} catch (...) { return 0; }

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// what the _host entry points of the trajectory metrics share: validate, stage (pack, upload), run, download
// ---------------------------------------------------------------------------------------------
static int upload(mkamd_ctx* ctx, int slot, const void* src, size_t bytes, void** dst)
try {
    int st = ctx->ensure(slot, bytes, dst, 0);
    if (st) return st;
    if (bytes) HIP_TRY(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
} MK_API_CATCH

// every index of a list below N, or "<what> index out of range"
template <class T>
static int check_indices(const T* idx, int64_t n, int64_t N, const char* what)
{
    for (int64_t i = 0; i < n; ++i)
        if ((uint64_t)(int64_t)idx[i] >= (uint64_t)N) {              // (a negative index of a signed list is out of range as well)
            char msg[96];
            snprintf(msg, sizeof msg, "%s index out of range", what);
            return fail(MKAMD_EINVAL, msg);
        }
    return 0;
}

// The coordinates ([N][3][F]) of a host call and what names their atoms, on the way up.  Only the rows of the atoms the call's index
// lists name go up (host_pack.h), with the lists and the per-atom arrays in the packed numbering, when those atoms are few and avoid
// bit 32 is clear -- or whatever their number (`always`: group moments); the caller's arrays as they are otherwise.
struct HostStage {
    using List = std::pair<const uint32_t*, int64_t>;                // atom indices and their number
    mkamd_ctx* ctx;
    const float* coords;
    int64_t N, F;
    mkamd::PackedAtoms pk;
    std::vector<std::shared_ptr<const void>> held;                   // the rewritten arrays, until sync()

    HostStage(mkamd_ctx* ctx_, const float* coords_, int64_t N_, int64_t F_, std::initializer_list<List> lists, bool always = false)
        : ctx(ctx_), coords(coords_), N(N_), F(F_)
    {
        for (const List& l : lists) if (l.first) pk.collect(l.first, l.second);
        if (always || !(ctx->dist_avoid & 32)) pk.finish(coords, N, F, ctx->packed_coords, always);
    }
    int64_t rows() const { return pk.on ? pk.size() : N; }           // atoms of the array that goes up
    const float* host_rows() const { return pk.on ? ctx->packed_coords.data() : coords; }
    int coords_to(int slot, void** d) { return upload(ctx, slot, host_rows(), (size_t)rows() * 3 * F * 4, d); }
    template <class T>
    const T* hold(std::vector<T> v)
    {
        auto p = std::make_shared<const std::vector<T>>(std::move(v));
        held.push_back(p);
        return p->data();
    }
    template <class T>                                               // an index list: in the numbering of the rows that went up
    int list_to(int slot, const T* idx, int64_t n, void** d) { return upload(ctx, slot, pk.on ? hold(pk.remap(idx, n)) : idx, (size_t)n * sizeof(T), d); }
    template <class T>                                               // one value per atom (chain ids, masses): those of the rows that went up
    int per_atom_to(int slot, const T* values, void** d) { return upload(ctx, slot, pk.on ? hold(pk.gather(values)) : values, (size_t)rows() * sizeof(T), d); }
    int sync()                                                       // the copies have read `held` and the packed rows (the caller's arrays need no wait)
    {
        if (pk.on) HIP_TRY(hipStreamSynchronize(ctx->stream));
        held.clear();
        return 0;
    }
    void unpack_in_place(std::vector<uint32_t>& atoms) const { if (pk.on) pk.unpack_in_place(atoms.data(), atoms.size()); }   // results that name atoms
};

// [rows][F] of the host -> frame-major [F][rows] on the device: up into `slab_slot`, transposed into `xyz_slot`
static int upload_frame_major(mkamd_ctx* ctx, int slab_slot, int xyz_slot, const float* src, int64_t rows, int64_t F, void** d_xyz)
{
    int st;
    void* dslab;
    if ((st = upload(ctx, slab_slot, src, (size_t)rows * F * 4, &dslab))) return st;
    if ((st = ctx->ensure(xyz_slot, (size_t)rows * F * 4, d_xyz))) return st;
    return mkamd_frames_to_items_dev(ctx, ctx->stream, (const float*)dslab, rows, F, F, 1.0f, (float*)*d_xyz);
}

// a result down to the caller's array; `prefault`: a big one's pages are touched first (prefault_big_result)
static int download(mkamd_ctx* ctx, void* dst, const void* d_src, size_t bytes, bool prefault)
{
    if (prefault) prefault_big_result(dst, bytes);
    return ctx->to_host(dst, d_src, bytes);
}

// ---------------------------------------------------------------------------------------------
// distance_utils row (include/mkamd_distance.h)
// ---------------------------------------------------------------------------------------------
extern "C" {

int64_t mkamd_dist_count_pairs(int64_t n1, int64_t n2, int selfdist) { return count_pairs(n1, n2, selfdist); }

int mkamd_dist_trajectory_dev(mkamd_ctx* ctx, const float* d_coords, int64_t F, const float* d_box,
                              const uint32_t* d_sel1, int64_t n1, const uint32_t* d_sel2, int64_t n2,
                              const uint32_t* d_chains, int selfdist, int pbc, int squared, float* d_results)
try {
    int st = dist_entry(ctx);
    if (st) return st;
    std::string err;
    st = run_dist_trajectory(*ctx, d_coords, F, d_box, d_sel1, n1, d_sel2, n2, d_chains, selfdist, pbc, squared, d_results, err, ctx->dist_avoid);
    return run_status(st, err);
} MK_API_CATCH

int mkamd_dist_trajectory_host(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const float* box,
                               const uint32_t* sel1, int64_t n1, const uint32_t* sel2, int64_t n2,
                               const uint32_t* chains, int selfdist, int pbc, int squared, float* results)
try {
    int st = dist_entry(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || n1 < 0 || n2 < 0) return fail(MKAMD_EINVAL, "negative size");
    const int64_t P = count_pairs(n1, n2, selfdist);
    if (F == 0 || P == 0) return MKAMD_OK;
    if (!coords || !box || !sel1 || !sel2 || !chains || !results) return fail(MKAMD_EINVAL, "NULL pointer");
    if ((st = check_indices(sel1, n1, N, "sel1")) || (st = check_indices(sel2, n2, N, "sel2"))) return st;
    void *dc, *db, *d1, *d2, *dch, *dout;
    HostStage up(ctx, coords, N, F, {{sel1, n1}, {sel2, n2}});
    if ((st = up.coords_to(WS_H_COORDS, &dc))) return st;
    if ((st = up.list_to(WS_D_SEL1, sel1, n1, &d1))) return st;
    if ((st = up.list_to(WS_D_SEL2, sel2, n2, &d2))) return st;
    if ((st = up.per_atom_to(WS_D_CHAINS, chains, &dch))) return st;
    if ((st = up.sync())) return st;
    if ((st = upload(ctx, WS_H_BOX, box, (size_t)3 * F * 4, &db))) return st;
    if ((st = ctx->ensure(WS_H_OUT, (size_t)F * P * 4, &dout, 0))) return st;
    st = mkamd_dist_trajectory_dev(ctx, (const float*)dc, F, (const float*)db, (const uint32_t*)d1, n1, (const uint32_t*)d2, n2,
                                   (const uint32_t*)dch, selfdist, pbc, squared, (float*)dout);
    if (st) return st;
    return download(ctx, results, dout, (size_t)F * P * 4, true);
} MK_API_CATCH

// contacts_trajectory / get_collisions on the device (dist_kernels.h: count -> scan -> fill per chunk of frames)
int mkamd_contacts_trajectory_host(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const float* box,
                                   const uint32_t* sel1, int64_t n1, const uint32_t* sel2, int64_t n2,
                                   const uint32_t* chains, int selfdist, int pbc, float dist_threshold,
                                   int64_t* frame_offsets, const uint32_t** pairs)
try {
    int st = dist_entry(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || n1 < 0 || n2 < 0) return fail(MKAMD_EINVAL, "negative size");
    if (!frame_offsets || !pairs) return fail(MKAMD_EINVAL, "frame_offsets/pairs pointer is NULL");
    ctx->contacts_host.clear();
    *pairs = nullptr;
    for (int64_t f = 0; f <= F; ++f) frame_offsets[f] = 0;
    const int64_t P = count_pairs(n1, n2, selfdist);
    if (F == 0 || P == 0) return MKAMD_OK;
    if (!coords || !box || !sel1 || !sel2 || !chains) return fail(MKAMD_EINVAL, "NULL pointer");
    if ((st = check_indices(sel1, n1, N, "sel1")) || (st = check_indices(sel2, n2, N, "sel2"))) return st;
    void *dc, *db, *d1, *d2, *dch;
    HostStage up(ctx, coords, N, F, {{sel1, n1}, {sel2, n2}});
    if ((st = up.coords_to(WS_H_COORDS, &dc))) return st;
    if ((st = up.list_to(WS_D_SEL1, sel1, n1, &d1))) return st;
    if ((st = up.list_to(WS_D_SEL2, sel2, n2, &d2))) return st;
    if ((st = up.per_atom_to(WS_D_CHAINS, chains, &dch))) return st;
    if ((st = up.sync())) return st;
    if ((st = upload(ctx, WS_H_BOX, box, (size_t)3 * F * 4, &db))) return st;
    std::string err;
    static_assert(sizeof(long long) == sizeof(int64_t), "frame offsets are int64");
    st = run_contacts(*ctx, (const float*)dc, (long long)F, (const float*)db, (const unsigned*)d1, (long long)n1, (const unsigned*)d2,
                      (long long)n2, (const unsigned*)dch, selfdist, pbc, dist_threshold, (size_t)256 << 20,
                      (long long*)frame_offsets, HostPairSink<mkamd_ctx>{*ctx, ctx->contacts_host}, err);
    if (st) return run_status(st, err);
    if (ctx->contacts_host.empty()) return MKAMD_OK;
    up.unpack_in_place(ctx->contacts_host);                          // the list names atoms of the caller's array
    *pairs = ctx->contacts_host.data();
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_dist_reduction_host(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const float* box,
                              const int32_t* g1_atoms, const int64_t* g1_off, int64_t ng1, const int32_t* g2_atoms,
                              const int64_t* g2_off, int64_t ng2, const uint32_t* chains1, const uint32_t* chains2,
                              int selfdist, int pairs, int pbc, const float* masses, int reduction1, int reduction2,
                              float* results)
try {
    int st = dist_entry(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || ng1 < 0 || ng2 < 0) return fail(MKAMD_EINVAL, "negative size");
    if (pairs && ng1 != ng2) return fail(MKAMD_EINVAL, "pairs mode needs the same number of groups on both sides");
    const int64_t P = pairs ? ng1 : count_pairs(ng1, ng2, selfdist);
    if (F == 0 || P == 0) return MKAMD_OK;
    if (!coords || !box || !g1_off || !g2_off || !chains1 || !chains2 || !results) return fail(MKAMD_EINVAL, "NULL pointer");
    if ((reduction1 == 1 || reduction2 == 1) && !masses) return fail(MKAMD_EINVAL, "masses are required for the com reduction");
    for (int64_t g = 0; g < ng1; ++g) if (g1_off[g + 1] <= g1_off[g]) return fail(MKAMD_EINVAL, "empty group in groups1");
    for (int64_t g = 0; g < ng2; ++g) if (g2_off[g + 1] <= g2_off[g]) return fail(MKAMD_EINVAL, "empty group in groups2");
    if ((st = check_indices(g1_atoms, g1_off[ng1], N, "groups1 atom")) || (st = check_indices(g2_atoms, g2_off[ng2], N, "groups2 atom"))) return st;
    void *dc, *db, *a1, *o1, *a2, *o2, *c1, *c2, *dm = nullptr, *dout;
    HostStage up(ctx, coords, N, F, {{reinterpret_cast<const uint32_t*>(g1_atoms), g1_off[ng1]}, {reinterpret_cast<const uint32_t*>(g2_atoms), g2_off[ng2]}});
    if ((st = up.coords_to(WS_H_COORDS, &dc))) return st;
    if ((st = up.list_to(WS_D_G1A, g1_atoms, g1_off[ng1], &a1))) return st;
    if ((st = up.list_to(WS_D_G2A, g2_atoms, g2_off[ng2], &a2))) return st;
    if (masses && (st = up.per_atom_to(WS_D_MASS, masses, &dm))) return st;
    if ((st = up.sync())) return st;
    if ((st = upload(ctx, WS_H_BOX, box, (size_t)3 * F * 4, &db))) return st;
    if ((st = upload(ctx, WS_D_G1O, g1_off, (size_t)(ng1 + 1) * 8, &o1))) return st;
    if ((st = upload(ctx, WS_D_G2O, g2_off, (size_t)(ng2 + 1) * 8, &o2))) return st;
    if ((st = upload(ctx, WS_D_CHAINS, chains1, (size_t)ng1 * 4, &c1))) return st;
    if ((st = upload(ctx, WS_D_CHAINS2, chains2, (size_t)ng2 * 4, &c2))) return st;
    if ((st = ctx->ensure(WS_H_OUT, (size_t)F * P * 4, &dout, 0))) return st;
    std::string err;
    st = run_dist_reduction(*ctx, (const float*)dc, up.rows(), F, (const float*)db, (const int*)a1, (const long long*)o1, ng1, g1_off[ng1], (const int*)a2,
                            (const long long*)o2, ng2, (const unsigned*)c1, (const unsigned*)c2, selfdist, pairs, pbc,
                            (const float*)dm, reduction1, reduction2, (float*)dout, err,
                            ctx->reduction_block ? ctx->reduction_block : reduction_block_for((const long long*)g1_off, ng1),
                            ctx->reduction_block == -2 ? 1 : ctx->reduction_block ? -1 : 0);
    if (st) return run_status(st, err);
    return download(ctx, results, dout, (size_t)F * P * 4, true);
} MK_API_CATCH

// ---- device-resident forms (round 6): coordinates, selections / groups and results stay on the GPU; asynchronous on the
// context's stream except for the contact list, whose size has to reach the host ----
int mkamd_contacts_trajectory_dev(mkamd_ctx* ctx, const float* d_coords, int64_t F, const float* d_box, const uint32_t* d_sel1,
                                  int64_t n1, const uint32_t* d_sel2, int64_t n2, const uint32_t* d_chains, int selfdist, int pbc,
                                  float dist_threshold, int64_t* frame_offsets, const uint32_t** d_pairs)
try {
    int st = dist_entry(ctx);
    if (st) return st;
    if (F < 0 || n1 < 0 || n2 < 0) return fail(MKAMD_EINVAL, "negative size");
    if (!frame_offsets || !d_pairs) return fail(MKAMD_EINVAL, "frame_offsets/d_pairs pointer is NULL");
    *d_pairs = nullptr;
    for (int64_t f = 0; f <= F; ++f) frame_offsets[f] = 0;
    if (F == 0 || count_pairs(n1, n2, selfdist) == 0) return MKAMD_OK;
    if (!d_coords || !d_box || !d_sel1 || !d_sel2 || !d_chains) return fail(MKAMD_EINVAL, "NULL pointer");
    std::string err;
    DevicePairSink<mkamd_ctx> sink{*ctx};
    st = run_contacts(*ctx, d_coords, (long long)F, d_box, d_sel1, (long long)n1, d_sel2, (long long)n2, d_chains, selfdist, pbc,
                      dist_threshold, (size_t)256 << 20, (long long*)frame_offsets, sink, err);
    if (st) return run_status(st, err);
    if (sink.size) *d_pairs = static_cast<const uint32_t*>(sink.base);
    return MKAMD_OK;
} MK_API_CATCH

int mkamd_dist_reduction_dev(mkamd_ctx* ctx, const float* d_coords, int64_t N, int64_t F, const float* d_box,
                             const int32_t* d_g1_atoms, const int64_t* d_g1_off, int64_t ng1, int64_t n_g1_atoms,
                             const int32_t* d_g2_atoms, const int64_t* d_g2_off, int64_t ng2, const uint32_t* d_chains1,
                             const uint32_t* d_chains2, int selfdist, int pairs, int pbc, const float* d_masses, int reduction1,
                             int reduction2, float* d_results)
try {
    int st = dist_entry(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || ng1 < 0 || ng2 < 0 || n_g1_atoms < 0) return fail(MKAMD_EINVAL, "negative size");
    if (pairs && ng1 != ng2) return fail(MKAMD_EINVAL, "pairs mode needs the same number of groups on both sides");
    const int64_t P = pairs ? ng1 : count_pairs(ng1, ng2, selfdist);
    if (F == 0 || P == 0) return MKAMD_OK;
    if (!d_coords || !d_box || !d_g1_atoms || !d_g1_off || !d_g2_atoms || !d_g2_off || !d_chains1 || !d_chains2 || !d_results)
        return fail(MKAMD_EINVAL, "NULL pointer");
    if ((reduction1 == 1 || reduction2 == 1) && !d_masses) return fail(MKAMD_EINVAL, "masses are required for the com reduction");
    std::string err;
    static_assert(sizeof(long long) == sizeof(int64_t), "group offsets are int64");
    st = run_dist_reduction(*ctx, d_coords, N, F, d_box, (const int*)d_g1_atoms, (const long long*)d_g1_off, ng1, n_g1_atoms,
                            (const int*)d_g2_atoms, (const long long*)d_g2_off, ng2, d_chains1, d_chains2, selfdist, pairs, pbc, d_masses,
                            reduction1, reduction2, d_results, err, ctx->reduction_block,
                            ctx->reduction_block == -2 ? 1 : ctx->reduction_block ? -1 : 0);
    return run_status(st, err);
} MK_API_CATCH

int mkamd_cdist_dev(mkamd_ctx* ctx, const float* d_c1, int64_t n1, const float* d_c2, int64_t n2, int32_t D, float* d_results)
try {
    int st = dist_entry(ctx);
    if (st) return st;
    if (n1 < 0 || n2 < 0 || D < 0) return fail(MKAMD_EINVAL, "negative size");
    if (n1 == 0 || n2 == 0) return MKAMD_OK;
    if (!d_c1 || !d_c2 || !d_results) return fail(MKAMD_EINVAL, "NULL pointer");
    std::string err;
    st = run_cdist(*ctx, d_c1, n1, d_c2, n2, D, d_results, err);
    return run_status(st, err);
} MK_API_CATCH

int mkamd_pdist_dev(mkamd_ctx* ctx, const float* d_c, int64_t n, int32_t D, float* d_results)
try {
    int st = dist_entry(ctx);
    if (st) return st;
    if (n < 0 || D < 0) return fail(MKAMD_EINVAL, "negative size");
    if (n < 2) return MKAMD_OK;
    if (!d_c || !d_results) return fail(MKAMD_EINVAL, "NULL pointer");
    std::string err;
    st = run_pdist(*ctx, d_c, n, D, d_results, err);
    return run_status(st, err);
} MK_API_CATCH

int mkamd_cdist_host(mkamd_ctx* ctx, const float* c1, int64_t n1, const float* c2, int64_t n2, int32_t D, float* results)
try {
    int st = dist_entry(ctx);
    if (st) return st;
    if (n1 < 0 || n2 < 0 || D < 0) return fail(MKAMD_EINVAL, "negative size");
    if (n1 == 0 || n2 == 0) return MKAMD_OK;
    if (!c1 || !c2 || !results) return fail(MKAMD_EINVAL, "NULL pointer");
    void *d1, *d2, *dout;
    if ((st = upload(ctx, WS_H_COORDS, c1, (size_t)n1 * D * 4, &d1))) return st;
    if ((st = upload(ctx, WS_H_SIGMAS, c2, (size_t)n2 * D * 4, &d2))) return st;
    if ((st = ctx->ensure(WS_H_OUT, (size_t)n1 * n2 * 4, &dout, 0))) return st;
    std::string err;
    st = run_cdist(*ctx, (const float*)d1, n1, (const float*)d2, n2, D, (float*)dout, err);
    if (st) return run_status(st, err);
    return download(ctx, results, dout, (size_t)n1 * n2 * 4, true);
} MK_API_CATCH

int mkamd_pdist_host(mkamd_ctx* ctx, const float* c, int64_t n, int32_t D, float* results)
try {
    int st = dist_entry(ctx);
    if (st) return st;
    if (n < 0 || D < 0) return fail(MKAMD_EINVAL, "negative size");
    if (n < 2) return MKAMD_OK;
    if (!c || !results) return fail(MKAMD_EINVAL, "NULL pointer");
    void *d1, *dout;
    if ((st = upload(ctx, WS_H_COORDS, c, (size_t)n * D * 4, &d1))) return st;
    if ((st = ctx->ensure(WS_H_OUT, (size_t)n * (n - 1) / 2 * 4, &dout, 0))) return st;
    std::string err;
    st = run_pdist(*ctx, (const float*)d1, n, D, (float*)dout, err);
    if (st) return run_status(st, err);
    return download(ctx, results, dout, (size_t)n * (n - 1) / 2 * 4, true);
} MK_API_CATCH

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// XTC decoding (host side, include/mkamd_xtc.h)
// ---------------------------------------------------------------------------------------------
extern "C" int mkamd_xtc_info(const char* path, int64_t* n_atoms, int64_t* n_frames)
try {
    if (!path || !n_atoms || !n_frames) return fail(MKAMD_EINVAL, "path/n_atoms/n_frames pointer is NULL");
    std::string err;
    int64_t na = 0, nf = 0;
    const int st = mkamd::xtc::info(path, na, nf, err);
    if (st) return fail(MKAMD_EINVAL, err);
    *n_atoms = na; *n_frames = nf;
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_xtc_read(const char* path, const int64_t* frames, int64_t n_sel, int64_t n_atoms, float* coords, float* box,
                              float* time, int32_t* step, int32_t n_threads)
try {
    if (!path) return fail(MKAMD_EINVAL, "path is NULL");
    if (n_sel < 0 || n_atoms < 0) return fail(MKAMD_EINVAL, "n_sel and n_atoms must be >= 0");
    if (n_sel == 0) return MKAMD_OK;
    if (!coords || !box || !time || !step) return fail(MKAMD_EINVAL, "coords/box/time/step pointer is NULL");
    std::string err;
    const int st = mkamd::xtc::read(path, frames, n_sel, n_atoms, coords, box, time, step, (int)n_threads, err);
    if (st) return fail(MKAMD_EINVAL, err);
    return MKAMD_OK;
} MK_API_CATCH

// ---- XTC decoding on the device (xtc_gpu.h): the host parses the record headers and copies the records' bytes; a lane walks a frame,
// a thread decodes a group ----
// (the record headers are parsed by xtc_parse_headers, csrc/xtc_headers.h: host code without HIP, so that the CPU tier runs it under
// sanitizers -- tests/emu/xtc_damage_main.cpp)
static int xtc_parse_headers(const uint8_t* base, size_t base_off, size_t limit, size_t file_size, const mkamd::xtc::FrameIndex& idx,
                             const int64_t* frames, int64_t n_sel, int64_t n_atoms, void* desc_out, int64_t* byte_lo, int64_t* byte_hi,
                             float* box, float* time, int32_t* step)
{
    return mkamd::xtc_parse_headers(base, base_off, limit, file_size, idx, frames, n_sel, n_atoms, desc_out, byte_lo, byte_hi, box, time, step,
                                    [](const char* msg) { return fail(MKAMD_EINVAL, msg); });
}

extern "C" int mkamd_xtc_chunk_desc(const char* path, const int64_t* frames, int64_t n_sel, int64_t n_atoms, void* desc_out,
                                    int64_t* byte_lo, int64_t* byte_hi, float* box, float* time, int32_t* step)
try {
    using namespace mkamd::xtc;
    if (!path) return fail(MKAMD_EINVAL, "path is NULL");
    if (n_sel <= 0 || n_atoms < 0) return fail(MKAMD_EINVAL, "n_sel must be > 0 and n_atoms >= 0");
    if (!desc_out || !byte_lo || !byte_hi || !box || !time || !step) return fail(MKAMD_EINVAL, "NULL pointer");
    Mapped m;
    if (!m.open_file(path)) return fail(MKAMD_EINVAL, std::string("cannot open ") + path);
    std::shared_ptr<const FrameIndex> idx;
    if (index_frames_cached(m, idx) != OK) return fail(MKAMD_EINVAL, "not an XTC file (bad magic number)");
    if (idx->natoms != n_atoms) return fail(MKAMD_EINVAL, "atom count of the file differs from the buffers'");
    return xtc_parse_headers(m.p, 0, m.n, m.n, *idx, frames, n_sel, n_atoms, desc_out, byte_lo, byte_hi, box, time, step);
} MK_API_CATCH

// The byte range [lo, hi) of the selected frames' records from the frame index alone (no record is touched): what a streaming reader
// copies FIRST (mkamd_xtc_copy_bytes) -- the headers are then parsed out of that copy (mkamd_xtc_chunk_desc_mem) instead of out of the
// file: a fresh mapping takes a page fault per header, 2 ms per 2 048 frames beside a 4-ms copy (round 6)
extern "C" int mkamd_xtc_byte_range(const char* path, const int64_t* frames, int64_t n_sel, int64_t n_atoms, int64_t* byte_lo, int64_t* byte_hi)
try {
    using namespace mkamd::xtc;
    if (!path || !byte_lo || !byte_hi) return fail(MKAMD_EINVAL, "NULL pointer");
    if (n_sel <= 0 || n_atoms < 0) return fail(MKAMD_EINVAL, "n_sel must be > 0 and n_atoms >= 0");
    Mapped m;
    if (!m.open_file(path)) return fail(MKAMD_EINVAL, std::string("cannot open ") + path);
    std::shared_ptr<const FrameIndex> idx;
    if (index_frames_cached(m, idx) != OK) return fail(MKAMD_EINVAL, "not an XTC file (bad magic number)");
    if (idx->natoms != n_atoms) return fail(MKAMD_EINVAL, "atom count of the file differs from the buffers'");
    size_t lo = (size_t)-1, hi = 0;
    for (int64_t j = 0; j < n_sel; ++j) {
        const int64_t f = frames ? frames[j] : j;
        if (f < 0 || f >= (int64_t)idx->offs.size()) return fail(MKAMD_EINVAL, "frame index out of range");
        const size_t r = idx->offs[(size_t)f], e = (size_t)f + 1 < idx->offs.size() ? idx->offs[(size_t)f + 1] : m.n;   // (records lie behind one another)
        lo = std::min(lo, r); hi = std::max(hi, e);
    }
    *byte_lo = (int64_t)lo; *byte_hi = (int64_t)hi;
    return MKAMD_OK;
} MK_API_CATCH

// mkamd_xtc_chunk_desc from a COPY of the file's bytes [bytes_lo, bytes_hi) (host memory, e.g. the pinned staging buffer the records were
// just copied into); same results, the same checks; byte_lo / byte_hi come out as mkamd_xtc_chunk_desc gives them (byte_lo >= bytes_lo)
extern "C" int mkamd_xtc_chunk_desc_mem(const char* path, const int64_t* frames, int64_t n_sel, int64_t n_atoms, const void* bytes, int64_t bytes_lo,
                                        int64_t bytes_hi, void* desc_out, int64_t* byte_lo, int64_t* byte_hi, float* box, float* time, int32_t* step)
try {
    using namespace mkamd::xtc;
    if (!path || !bytes) return fail(MKAMD_EINVAL, "NULL pointer");
    if (n_sel <= 0 || n_atoms < 0) return fail(MKAMD_EINVAL, "n_sel must be > 0 and n_atoms >= 0");
    if (!desc_out || !byte_lo || !byte_hi || !box || !time || !step) return fail(MKAMD_EINVAL, "NULL pointer");
    Mapped m;
    if (!m.open_file(path)) return fail(MKAMD_EINVAL, std::string("cannot open ") + path);
    std::shared_ptr<const FrameIndex> idx;
    if (index_frames_cached(m, idx) != OK) return fail(MKAMD_EINVAL, "not an XTC file (bad magic number)");
    if (idx->natoms != n_atoms) return fail(MKAMD_EINVAL, "atom count of the file differs from the buffers'");
    if (bytes_lo < 0 || bytes_hi < bytes_lo || (size_t)bytes_hi > m.n) return fail(MKAMD_EINVAL, "byte range outside the file");
    return xtc_parse_headers(static_cast<const uint8_t*>(bytes), (size_t)bytes_lo, (size_t)bytes_hi, m.n, *idx, frames, n_sel, n_atoms, desc_out, byte_lo, byte_hi,
                             box, time, step);
} MK_API_CATCH

// Bytes [lo, hi) of the file into dst (pinned staging memory), by threads that pread() their slices: the page cache is copied straight
// into the destination.  (Until round 6 the threads copied out of a fresh mapping: 73 000 page faults per 300 MB chunk and an munmap of
// every touched page afterwards.)
extern "C" int mkamd_xtc_copy_bytes(const char* path, int64_t lo, int64_t hi, void* dst, int32_t n_threads)
try {
    if (!path || !dst) return fail(MKAMD_EINVAL, "NULL pointer");
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return fail(MKAMD_EINVAL, std::string("cannot open ") + path);
    struct stat stt;
    if (fstat(fd, &stt) != 0) { ::close(fd); return fail(MKAMD_EINVAL, std::string("cannot stat ") + path); }
    if (lo < 0 || hi < lo || (size_t)hi > (size_t)stt.st_size) { ::close(fd); return fail(MKAMD_EINVAL, "byte range outside the file"); }
    const size_t n = (size_t)(hi - lo);
    int nt = n_threads > 0 ? n_threads : (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
    nt = (int)std::min<size_t>((size_t)nt, std::max<size_t>(n >> 22, 1));         // >= 4 MB per thread
    std::atomic<int> bad{0};
    auto part = [&](int t) {
        size_t a = n / (size_t)nt * (size_t)t;
        const size_t b = t == nt - 1 ? n : n / (size_t)nt * (size_t)(t + 1);
        while (a < b) {
            const ssize_t got = ::pread(fd, (char*)dst + a, std::min<size_t>(b - a, (size_t)8 << 20), (off_t)((size_t)lo + a));
            if (got <= 0) { if (got < 0 && errno == EINTR) continue; bad.store(1); return; }
            a += (size_t)got;
        }
    };
    if (nt == 1) part(0);
    else { std::vector<std::thread> pool; for (int t = 0; t < nt; ++t) pool.emplace_back(part, t); for (auto& th : pool) th.join(); }
    ::close(fd);
    if (bad.load()) return fail(MKAMD_EINVAL, std::string("short read from ") + path);
    return MKAMD_OK;
} MK_API_CATCH

static uint64_t xtc_work_groups_offset(int64_t n_frames) { return ((uint64_t)n_frames * 4u + 255u) & ~(uint64_t)255u; }

extern "C" uint64_t mkamd_xtc_decode_work_bytes(int64_t n_frames, int64_t n_atoms)
{
    if (n_frames <= 0 || n_atoms < 0) return 0;
    return xtc_work_groups_offset(n_frames) + (uint64_t)n_frames * (uint64_t)(n_atoms + mkamd::XS_SPEC) * sizeof(mkamd::XtcGroup);
}

extern "C" int mkamd_xtc_decode_dev(mkamd_ctx* ctx, void* hip_stream, const void* d_bytes, const void* d_desc, int64_t n_frames,
                                    int64_t n_atoms, float scale, float* d_xyz, int32_t* d_status, void* d_work, uint64_t work_bytes)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (n_frames < 0 || n_atoms < 0) return fail(MKAMD_EINVAL, "n_frames / n_atoms must be >= 0");
    if (n_frames == 0) return MKAMD_OK;
    if (!d_bytes || !d_desc || !d_xyz || !d_status || !d_work) return fail(MKAMD_EINVAL, "NULL pointer");
    if (work_bytes < mkamd_xtc_decode_work_bytes(n_frames, n_atoms))
        return fail(MKAMD_EINVAL, "work buffer smaller than mkamd_xtc_decode_work_bytes(n_frames, n_atoms)");
    if (((uintptr_t)d_work & 7u) || ((uintptr_t)d_bytes & 3u)) return fail(MKAMD_EINVAL, "d_work must be 8-byte, d_bytes 4-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    int* ngroups = static_cast<int*>(d_work);
    mkamd::XtcGroup* groups = reinterpret_cast<mkamd::XtcGroup*>(static_cast<unsigned char*>(d_work) + xtc_work_groups_offset(n_frames));
    const unsigned char* bytes = static_cast<const unsigned char*>(d_bytes);
    const mkamd::XtcFrameDesc* desc = static_cast<const mkamd::XtcFrameDesc*>(d_desc);
    hipLaunchKernelGGL(mkamd::k_xtc_scan, dim3((unsigned)((n_frames + 63) / 64)), dim3(64), 0, s, bytes, desc, (long long)n_frames,
                       (long long)n_atoms, scale, d_xyz, groups, ngroups, d_status);
    HIP_TRY(hipGetLastError());
    if (n_atoms >= (1ll << 21)) return MKAMD_OK;                     // (every frame got status 2; nothing to expand)
    const int64_t bpf = (n_atoms + 255) / 256;
    if (bpf == 0) return MKAMD_OK;
    const int64_t per_launch = std::max<int64_t>(1, (int64_t)0x7fffffff / bpf);
    for (int64_t f0 = 0; f0 < n_frames; f0 += per_launch) {
        const int64_t nf = std::min(per_launch, n_frames - f0);
        hipLaunchKernelGGL(mkamd::k_xtc_expand, dim3((unsigned)(nf * bpf)), dim3(256), 0, s, bytes, desc, (long long)f0, (long long)n_atoms,
                           scale, d_xyz, groups, ngroups, (int)bpf);
        HIP_TRY(hipGetLastError());
    }
    return MKAMD_OK;
} MK_API_CATCH

// ---- XTC compression on the device (xtc_encode.h): the reference writer's bytes; asynchronous on the caller's stream ----
namespace {
struct XtcEncodeStreamBackend {
    hipStream_t stream;
    int fill(void* p, int byte, size_t bytes)
    {
        HIP_TRY(hipMemsetAsync(p, byte, bytes, stream));
        return 0;
    }
    template <class... KA, class... A>
    int launch(void (*kernel)(KA...), dim3 grid, dim3 block, A... args)
    {
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
        HIP_TRY(hipGetLastError());
        return 0;
    }
};
}  // namespace

extern "C" uint64_t mkamd_xtc_encode_work_bytes(int64_t n_frames, int64_t n_atoms) { return mkamd::xtc_encode_layout(n_frames, n_atoms).total; }

extern "C" uint64_t mkamd_xtc_encode_bound(int64_t n_frames, int64_t n_atoms) { return mkamd::xtc_encode_bound(n_frames, n_atoms); }

extern "C" int mkamd_xtc_encode_dev(mkamd_ctx* ctx, void* hip_stream, const float* d_xyz, float in_scale, const float* d_precision,
                                    const float* d_box, const float* d_time, const int32_t* d_step, int64_t n_frames, int64_t n_atoms,
                                    void* d_image, uint64_t image_capacity, uint64_t* d_offsets, int32_t* d_status, void* d_work,
                                    uint64_t work_bytes)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (n_frames < 0 || n_atoms < 0) return fail(MKAMD_EINVAL, "n_frames / n_atoms must be >= 0");
    if (n_frames == 0) return MKAMD_OK;
    if (n_atoms > 0x7fffffffll) return fail(MKAMD_EINVAL, "an XTC record counts its atoms in an int");
    if (!d_xyz || !d_precision || !d_box || !d_time || !d_step || !d_image || !d_offsets || !d_status || !d_work) return fail(MKAMD_EINVAL, "NULL pointer");
    if (work_bytes < mkamd_xtc_encode_work_bytes(n_frames, n_atoms))
        return fail(MKAMD_EINVAL, "work buffer smaller than mkamd_xtc_encode_work_bytes(n_frames, n_atoms)");
    if (image_capacity < mkamd_xtc_encode_bound(n_frames, n_atoms))
        return fail(MKAMD_EINVAL, "image buffer smaller than mkamd_xtc_encode_bound(n_frames, n_atoms)");
    if (((uintptr_t)d_work & 7u) || ((uintptr_t)d_image & 3u) || ((uintptr_t)d_offsets & 7u))
        return fail(MKAMD_EINVAL, "d_work and d_offsets must be 8-byte, d_image 4-byte aligned");
    XtcEncodeStreamBackend be{(hipStream_t)hip_stream};
    mkamd::XtcEncodeArgs a;
    a.xyz = d_xyz; a.in_scale = in_scale; a.precision = d_precision; a.box = d_box; a.time = d_time; a.step = d_step;
    a.n_frames = n_frames; a.n_atoms = n_atoms;
    a.image = static_cast<unsigned char*>(d_image); a.offsets = reinterpret_cast<unsigned long long*>(d_offsets); a.status = d_status;
    a.work = static_cast<unsigned char*>(d_work);
    return mkamd::run_xtc_encode(be, a);
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// DCD (include/mkamd_xtc.h "DCD"; dcd_reader.h on the host, dcd_kernels.h on the device)
// ---------------------------------------------------------------------------------------------
extern "C" int mkamd_dcd_info(const char* path, int64_t* n_atoms, int64_t* n_frames, int32_t* istart, int32_t* nsavc, double* delta,
                              int32_t* n_fixed, int32_t* flags)
try {
    if (!path || !n_atoms || !n_frames) return fail(MKAMD_EINVAL, "path/n_atoms/n_frames pointer is NULL");
    mkamd::xtc::Mapped m;
    mkamd::dcd::Header h;
    std::string err;
    if (mkamd::dcd::open_header(path, m, h, err)) return fail(MKAMD_EINVAL, err);
    *n_atoms = h.n_atoms; *n_frames = h.n_frames;
    if (istart) *istart = h.istart;
    if (nsavc) *nsavc = h.nsavc;
    if (delta) *delta = h.delta;
    if (n_fixed) *n_fixed = h.nfixed;
    if (flags) *flags = h.flags;
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_dcd_chunk_desc(const char* path, const int64_t* frames, int64_t n_sel, void* desc_out, int64_t* byte_lo, int64_t* byte_hi,
                                    float* cell)
try {
    if (!path || !desc_out || !byte_lo || !byte_hi || !cell) return fail(MKAMD_EINVAL, "NULL pointer");
    if (n_sel <= 0) return fail(MKAMD_EINVAL, "n_sel must be > 0");
    mkamd::xtc::Mapped m;
    mkamd::dcd::Header h;
    std::string err;
    if (mkamd::dcd::open_header(path, m, h, err)) return fail(MKAMD_EINVAL, err);
    if (mkamd::dcd::chunk_desc(m.p, m.n, h, frames, n_sel, static_cast<mkamd::dcd::FrameDesc*>(desc_out), byte_lo, byte_hi, cell, err))
        return fail(MKAMD_EINVAL, err);
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_dcd_source_table(const char* path, const int32_t* atoms, int64_t n_sel, int32_t* sel, int32_t* src)
try {
    if (!path) return fail(MKAMD_EINVAL, "path is NULL");
    if (n_sel < 0) return fail(MKAMD_EINVAL, "n_sel must be >= 0");
    if (n_sel == 0) return MKAMD_OK;
    if (!sel || !src) return fail(MKAMD_EINVAL, "NULL pointer");
    mkamd::xtc::Mapped m;
    mkamd::dcd::Header h;
    std::string err;
    if (mkamd::dcd::open_header(path, m, h, err)) return fail(MKAMD_EINVAL, err);
    if (!atoms && n_sel != h.n_atoms) return fail(MKAMD_EINVAL, "without an atom list n_sel must be the file's atom count");
    if (mkamd::dcd::source_table(h, atoms, n_sel, sel, src, err)) return fail(MKAMD_EINVAL, err);
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_dcd_read(const char* path, const int64_t* frames, int64_t n_frames, const int32_t* atoms, int64_t n_sel, float* xyz,
                              float* cell)
try {
    if (!path) return fail(MKAMD_EINVAL, "path is NULL");
    if (n_frames < 0 || n_sel < 0) return fail(MKAMD_EINVAL, "n_frames and n_sel must be >= 0");
    if (n_frames == 0) return MKAMD_OK;
    if (!cell || (n_sel > 0 && !xyz)) return fail(MKAMD_EINVAL, "xyz/cell pointer is NULL");
    mkamd::xtc::Mapped m;
    mkamd::dcd::Header h;
    std::string err;
    if (mkamd::dcd::open_header(path, m, h, err)) return fail(MKAMD_EINVAL, err);
    if (!atoms && n_sel != h.n_atoms) return fail(MKAMD_EINVAL, "without an atom list n_sel must be the file's atom count");
    if (mkamd::dcd::read(m.p, m.n, h, frames, n_frames, atoms, n_sel, xyz, cell, err)) return fail(MKAMD_EINVAL, err);
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_dcd_decode_dev(mkamd_ctx* ctx, void* hip_stream, const void* d_bytes, uint64_t n_bytes, const void* d_desc, int64_t n_frames,
                                    const int32_t* d_sel, const int32_t* d_src, int64_t n_sel, const float* d_frame0, int64_t n_atoms,
                                    float scale, float* d_xyz, int32_t* d_status)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (n_frames < 0 || n_sel < 0 || n_atoms < 0) return fail(MKAMD_EINVAL, "n_frames / n_sel / n_atoms must be >= 0");
    if (n_frames == 0) return MKAMD_OK;
    if (n_atoms > 0x7fffffffll || n_sel > 0x7fffffffll) return fail(MKAMD_EINVAL, "a DCD file counts its atoms in an int");
    if (!d_bytes || !d_desc || !d_status || (n_sel > 0 && (!d_sel || !d_src || !d_xyz))) return fail(MKAMD_EINVAL, "NULL pointer");
    if ((uintptr_t)d_bytes & 3u) return fail(MKAMD_EINVAL, "d_bytes must be 4-byte aligned");
    XtcEncodeStreamBackend be{(hipStream_t)hip_stream};
    return mkamd::run_dcd_decode(be, static_cast<const unsigned char*>(d_bytes), (unsigned long long)n_bytes,
                                 static_cast<const mkamd::dcd::FrameDesc*>(d_desc), (long long)n_frames, d_sel, d_src, (long long)n_sel, d_frame0,
                                 (long long)n_atoms, scale, d_xyz, d_status);
} MK_API_CATCH

extern "C" uint64_t mkamd_dcd_encode_bound(int64_t n_frames, int64_t n_atoms, int32_t with_cell)
{
    if (n_frames <= 0 || n_atoms <= 0) return 0;
    return (uint64_t)n_frames * mkamd::dcd_frame_bytes(n_atoms, with_cell != 0);
}

extern "C" int mkamd_dcd_encode_dev(mkamd_ctx* ctx, void* hip_stream, const float* d_xyz, const double* d_cell, int64_t n_frames, int64_t n_atoms,
                                    void* d_image, uint64_t image_capacity)
try {
    int st = check_ctx(ctx, true);
    if (st) return st;
    if (n_frames < 0 || n_atoms <= 0) return fail(MKAMD_EINVAL, "n_frames must be >= 0 and n_atoms > 0");
    if (n_frames == 0) return MKAMD_OK;
    if (n_atoms >= (1ll << 29)) return fail(MKAMD_EINVAL, "a DCD record marker holds 4 * n_atoms in an int");
    if (!d_xyz || !d_image) return fail(MKAMD_EINVAL, "NULL pointer");
    if (image_capacity < mkamd_dcd_encode_bound(n_frames, n_atoms, d_cell != nullptr))
        return fail(MKAMD_EINVAL, "image buffer smaller than mkamd_dcd_encode_bound(n_frames, n_atoms, with_cell)");
    if (((uintptr_t)d_image & 3u) || ((uintptr_t)d_cell & 7u)) return fail(MKAMD_EINVAL, "d_image must be 4-byte, d_cell 8-byte aligned");
    XtcEncodeStreamBackend be{(hipStream_t)hip_stream};
    return mkamd::run_dcd_encode(be, d_xyz, d_cell, (long long)n_frames, (long long)n_atoms, static_cast<unsigned char*>(d_image));
} MK_API_CATCH

extern "C" int mkamd_dcd_cell_record(const float* lengths, const float* angles, int64_t n, double* out)
try {
    if (n < 0) return fail(MKAMD_EINVAL, "n must be >= 0");
    if (n > 0 && (!lengths || !angles || !out)) return fail(MKAMD_EINVAL, "NULL pointer");
    for (int64_t i = 0; i < n; ++i) mkamd::dcd::cell_record(lengths + 3 * i, angles + 3 * i, out + 6 * i);
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_dcd_header(int64_t n_atoms, int64_t n_frames, int32_t istart, int32_t nsavc, double delta, int32_t with_cell, void* out)
try {
    if (!out) return fail(MKAMD_EINVAL, "out is NULL");
    if (n_atoms <= 0 || n_atoms >= (1ll << 29)) return fail(MKAMD_EINVAL, "n_atoms must be in [1, 2^29)");
    if (n_frames < 0 || n_frames > 0x7fffffffll) return fail(MKAMD_EINVAL, "n_frames must fit an int");
    mkamd::dcd::write_header((int32_t)n_atoms, (int32_t)n_frames, istart, nsavc, delta, with_cell != 0, static_cast<uint8_t*>(out));
    return MKAMD_OK;
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// alignment (include/mkamd_distance.h "alignment"; align_pipeline.h)
// ---------------------------------------------------------------------------------------------
static mkamd::AlignArgs align_args(const float* d_xyz, int64_t N, int64_t F, const float* d_ref, int64_t Nr, int64_t Fr,
                                   const uint32_t* d_sel, const uint32_t* d_refsel, int64_t n, const int64_t* d_frames, int64_t K,
                                   int64_t refframe, int matching)
{
    mkamd::AlignArgs a;
    a.xyz = d_xyz; a.n_atoms = N; a.n_frames = F;
    a.ref = d_ref; a.n_ref_atoms = Nr; a.n_ref_frames = Fr;
    a.sel = d_sel; a.refsel = d_refsel; a.n = n;
    a.frames = reinterpret_cast<const long long*>(d_frames); a.n_list = K;
    a.refframe = refframe; a.matching = matching != 0;
    return a;
}

extern "C" int mkamd_align_transforms_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t N, int64_t F, const float* d_ref, int64_t Nr,
                                          int64_t Fr, const uint32_t* d_sel, const uint32_t* d_refsel, int64_t n, const int64_t* d_frames,
                                          int64_t K, int64_t refframe, int matching, double* d_affine, double* d_fit_rmsd)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (K > 0 && (!d_xyz || !d_ref || !d_affine || (n > 0 && (!d_sel || !d_refsel)))) return fail(MKAMD_EINVAL, "NULL pointer");
    std::string err;
    st = mkamd::run_align_transforms(*ctx, align_args(d_xyz, N, F, d_ref, Nr, Fr, d_sel, d_refsel, n, d_frames, K, refframe, matching),
                                     d_affine, d_fit_rmsd, err);
    return run_status(st, err);
} MK_API_CATCH

extern "C" int mkamd_align_apply_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t N, const int64_t* d_frames, int64_t K,
                                     const double* d_affine, float* d_out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (N > 0 && K > 0 && (!d_xyz || !d_affine || !d_out)) return fail(MKAMD_EINVAL, "NULL pointer");
    if ((((uintptr_t)d_xyz) | ((uintptr_t)d_out)) & 3) return fail(MKAMD_EINVAL, "coordinates must be 4-byte aligned");
    std::string err;
    st = mkamd::run_align_apply(*ctx, d_xyz, N, reinterpret_cast<const long long*>(d_frames), K, d_affine, d_out, err);
    return run_status(st, err);
} MK_API_CATCH

extern "C" int mkamd_align_rmsd_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t N, int64_t F, const float* d_ref, int64_t Nr, int64_t Fr,
                                    const uint32_t* d_sel, const uint32_t* d_refsel, int64_t n, const int64_t* d_frames, int64_t K,
                                    int64_t refframe, int matching, const double* d_affine, float* d_rmsd)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (K > 0 && (!d_xyz || !d_ref || !d_affine || !d_rmsd || (n > 0 && (!d_sel || !d_refsel)))) return fail(MKAMD_EINVAL, "NULL pointer");
    std::string err;
    st = mkamd::run_align_rmsd(*ctx, align_args(d_xyz, N, F, d_ref, Nr, Fr, d_sel, d_refsel, n, d_frames, K, refframe, matching),
                               d_affine, d_rmsd, err);
    return run_status(st, err);
} MK_API_CATCH

extern "C" int mkamd_align_host(mkamd_ctx* ctx, float* coords, int64_t N, int64_t F, const float* refcoords, int64_t Nr, int64_t Fr,
                                const uint32_t* sel, const uint32_t* refsel, int64_t n, const int64_t* frames, int64_t K, int64_t refframe,
                                int matching)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || Nr < 0 || Fr < 0 || n < 0 || K < 0) return fail(MKAMD_EINVAL, "negative size");
    if (K == 0 || N == 0) return MKAMD_OK;
    if (!coords || !refcoords || !frames || (n > 0 && (!sel || !refsel))) return fail(MKAMD_EINVAL, "NULL pointer");
    if (matching && Fr != F) return fail(MKAMD_EINVAL, "matchingframes needs a reference with as many frames as the trajectory");
    if (!matching && (refframe < 0 || refframe >= Fr)) return fail(MKAMD_EINVAL, "refframe out of range");
    if ((st = check_indices(sel, n, N, "selection")) || (st = check_indices(refsel, n, Nr, "selection"))) return st;
    int64_t fmin = F, fmax = -1;
    for (int64_t i = 0; i < K; ++i) {
        if (frames[i] < 0 || frames[i] >= F) return fail(MKAMD_EINVAL, "frame index out of range");
        fmin = std::min(fmin, frames[i]);
        fmax = std::max(fmax, frames[i]);
    }
    const int64_t span = fmax - fmin + 1, rows = 3 * N;
    // the listed frames' span of [3N][F] -> [3N][span] -> frame-major [span][N][3]; the reference likewise (matchingframes) or its
    // one frame gathered on the host
    void *dslab, *dxyz, *dref, *dsel, *drefsel, *dframes, *daff;
    if ((st = ctx->ensure(WS_A_SLAB, (size_t)rows * span * 4, &dslab))) return st;
    if ((st = ctx->ensure(WS_A_XYZ, (size_t)rows * span * 4, &dxyz))) return st;
    HIP_TRY(hipMemcpy2DAsync(dslab, (size_t)span * 4, coords + fmin, (size_t)F * 4, (size_t)span * 4, (size_t)rows, hipMemcpyHostToDevice,
                             ctx->stream));
    if ((st = mkamd_frames_to_items_dev(ctx, ctx->stream, (const float*)dslab, rows, span, span, 1.0f, (float*)dxyz))) return st;
    int64_t ref_frames = 1, rf = 0;
    if (matching) {
        if ((st = ctx->ensure(WS_A_REF, (size_t)3 * Nr * span * 4, &dref))) return st;
        HIP_TRY(hipMemcpy2DAsync(dslab, (size_t)span * 4, refcoords + fmin, (size_t)Fr * 4, (size_t)span * 4, (size_t)(3 * Nr),
                                 hipMemcpyHostToDevice, ctx->stream));     // (stream order: the transpose above has read the slab)
        if ((st = mkamd_frames_to_items_dev(ctx, ctx->stream, (const float*)dslab, 3 * Nr, span, span, 1.0f, (float*)dref))) return st;
        ref_frames = span;
    } else {
        std::vector<float> r((size_t)3 * Nr);
        for (int64_t k = 0; k < 3 * Nr; ++k) r[(size_t)k] = refcoords[k * Fr + refframe];
        if ((st = upload(ctx, WS_A_REF, r.data(), r.size() * 4, &dref))) return st;
        HIP_TRY(hipStreamSynchronize(ctx->stream));                      // (r is a local)
    }
    std::vector<int64_t> rel((size_t)K);
    for (int64_t i = 0; i < K; ++i) rel[(size_t)i] = frames[i] - fmin;
    if ((st = upload(ctx, WS_A_SEL, sel, (size_t)n * 4, &dsel))) return st;
    if ((st = upload(ctx, WS_A_REFSEL, refsel, (size_t)n * 4, &drefsel))) return st;
    if ((st = upload(ctx, WS_A_FRAMES, rel.data(), (size_t)K * 8, &dframes))) return st;
    if ((st = ctx->ensure(WS_A_AFFINE, (size_t)K * 12 * 8, &daff))) return st;
    std::string err;
    st = mkamd::run_align_transforms(*ctx, align_args((const float*)dxyz, N, span, (const float*)dref, Nr, ref_frames, (const uint32_t*)dsel,
                                                      (const uint32_t*)drefsel, n, (const int64_t*)dframes, K, rf, matching),
                                     (double*)daff, nullptr, err);
    if (!st) st = mkamd::run_align_apply(*ctx, (const float*)dxyz, N, (const long long*)dframes, K, (const double*)daff, (float*)dxyz, err);
    if (st) return run_status(st, err);
    // back to [3N][span], to the host, and only the listed frames into coords
    if ((st = mkamd_frames_to_items_dev(ctx, ctx->stream, (const float*)dxyz, span, rows, rows, 1.0f, (float*)dslab))) return st;
    std::vector<float> out((size_t)rows * span);
    HIP_TRY(hipMemcpyAsync(out.data(), dslab, out.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int64_t r = 0; r < rows; ++r) {
        float* dst = coords + r * F;
        const float* src = out.data() + (size_t)r * span - fmin;
        for (int64_t i = 0; i < K; ++i) dst[frames[i]] = src[frames[i]];
    }
    return MKAMD_OK;
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// surface area (include/mkamd_distance.h "surface area"; sasa_pipeline.h)
// ---------------------------------------------------------------------------------------------
static mkamd::SasaArgs sasa_args(const float* d_xyz, int64_t N, int64_t F, const float* d_radii, int32_t n_points, const int32_t* d_mapping,
                                 const int32_t* d_mask, float coord_div, float* d_out, int64_t n_out)
{
    mkamd::SasaArgs a;
    a.xyz = d_xyz; a.n_atoms = N; a.n_frames = F; a.radii = d_radii; a.n_points = n_points;
    a.mapping = reinterpret_cast<const int*>(d_mapping); a.mask = reinterpret_cast<const int*>(d_mask);
    a.n_out = n_out; a.coord_div = coord_div; a.out = d_out;
    return a;
}

extern "C" int mkamd_sasa_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t N, int64_t F, const float* d_radii, int32_t n_points,
                              const int32_t* d_mapping, const int32_t* d_mask, float coord_div, float* d_out, int64_t n_out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (N > 0 && F > 0 && (!d_xyz || !d_radii || !d_mapping || !d_mask || !d_out)) return fail(MKAMD_EINVAL, "NULL pointer");
    std::string err;
    st = mkamd::run_sasa(*ctx, sasa_args(d_xyz, N, F, d_radii, n_points, d_mapping, d_mask, coord_div, d_out, n_out), err);
    return run_status(st, err);
} MK_API_CATCH

extern "C" int mkamd_sasa_host(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const uint32_t* keep, int64_t n_keep,
                               const float* radii, int32_t n_points, const int32_t* mapping, const int32_t* mask, float coord_div,
                               float* out, int64_t n_out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || n_keep < 0 || n_out < 0) return fail(MKAMD_EINVAL, "negative size");
    const int64_t n = keep ? n_keep : N;
    if (n == 0 || F == 0) return MKAMD_OK;
    if (!coords || !radii || !mapping || !mask || !out) return fail(MKAMD_EINVAL, "NULL pointer");
    if (keep && (st = check_indices(keep, n, N, "kept atom"))) return st;
    if (n_out < 1) return fail(MKAMD_EINVAL, "n_out must be at least 1");
    // the kept atoms' rows of [N][3][F], in the caller's order (repeats included) -> [3 n][F] -> frame-major [F][n][3] on the device
    if (keep) mkamd::gather_rows(coords, F, keep, n, ctx->packed_coords);
    void *dxyz, *drad, *dmap, *dmask, *dout;
    if ((st = upload_frame_major(ctx, WS_S_SLAB, WS_S_XYZ, keep ? ctx->packed_coords.data() : coords, 3 * n, F, &dxyz))) return st;
    if ((st = upload(ctx, WS_S_RADII, radii, (size_t)n * 4, &drad))) return st;
    if ((st = upload(ctx, WS_S_MAP, mapping, (size_t)n * 4, &dmap))) return st;
    if ((st = upload(ctx, WS_S_MASK, mask, (size_t)n * 4, &dmask))) return st;
    if ((st = upload(ctx, WS_S_OUT, out, (size_t)F * n_out * 4, &dout))) return st;
    std::string err;
    st = mkamd::run_sasa(*ctx, sasa_args((const float*)dxyz, n, F, (const float*)drad, n_points, (const int32_t*)dmap, (const int32_t*)dmask,
                                         coord_div, (float*)dout, n_out), err);
    if (st) return run_status(st, err);
    return download(ctx, out, dout, (size_t)F * n_out * 4, false);
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// shell counts (include/mkamd_distance.h "shell counts"; shell_pipeline.h)
// ---------------------------------------------------------------------------------------------
extern "C" int mkamd_shell_counts_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_atoms, int64_t F, const float* d_box, const uint32_t* d_sel1,
                                      int64_t n1, const uint32_t* d_sel2, int64_t n2, const uint32_t* d_chains, int symmetric, int pbc,
                                      const float* d2_thresholds, int64_t n_edges, int32_t* d_counts)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (n_atoms < 0) return fail(MKAMD_EINVAL, "negative size");
    if (F > 0 && n1 > 0 && (!d_coords || !d_box || !d_sel1 || (n2 > 0 && !d_sel2) || !d_chains || !d_counts)) return fail(MKAMD_EINVAL, "NULL pointer");
    std::string err;
    st = mkamd::run_shell_counts(*ctx, d_coords, F, d_box, d_sel1, n1, d_sel2, n2, d_chains, symmetric, pbc, d2_thresholds, n_edges,
                                 reinterpret_cast<int*>(d_counts), err, (ctx->dist_avoid >> 8) & 3);
    return run_status(st, err);
} MK_API_CATCH

extern "C" int mkamd_shell_counts_host(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const float* box, const uint32_t* sel1, int64_t n1,
                                       const uint32_t* sel2, int64_t n2, const uint32_t* chains, int symmetric, int pbc,
                                       const float* d2_thresholds, int64_t n_edges, int32_t* counts)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || n1 < 0 || n2 < 0) return fail(MKAMD_EINVAL, "negative size");
    if (n_edges < 2 || n_edges > mkamd::SH_MAX_EDGES) return fail(MKAMD_EINVAL, "numshells must be between 1 and 32 (n_edges between 2 and 33)");
    if (F == 0 || n1 == 0) {
        if (!d2_thresholds) return fail(MKAMD_EINVAL, "NULL pointer");
        return MKAMD_OK;
    }
    if (!coords || !box || !sel1 || (n2 > 0 && !sel2) || !chains || !d2_thresholds || !counts) return fail(MKAMD_EINVAL, "NULL pointer");
    if ((st = check_indices(sel1, n1, N, "sel1")) || (st = check_indices(sel2, n2, N, "sel2"))) return st;
    void *dc, *db, *d1, *d2, *dch, *dout;
    HostStage up(ctx, coords, N, F, {{sel1, n1}, {sel2, n2}});
    if ((st = up.coords_to(WS_H_COORDS, &dc))) return st;
    if ((st = up.list_to(WS_D_SEL1, sel1, n1, &d1))) return st;
    if ((st = up.list_to(WS_D_SEL2, sel2, n2, &d2))) return st;
    if ((st = up.per_atom_to(WS_D_CHAINS, chains, &dch))) return st;
    if ((st = up.sync())) return st;
    if ((st = upload(ctx, WS_H_BOX, box, (size_t)3 * F * 4, &db))) return st;
    const size_t bytes = (size_t)F * (size_t)n1 * (size_t)(n_edges - 1) * 4;
    if ((st = ctx->ensure(WS_H_OUT, bytes, &dout, 0))) return st;
    st = mkamd_shell_counts_dev(ctx, (const float*)dc, up.rows(), F, (const float*)db, (const uint32_t*)d1, n1, (const uint32_t*)d2, n2,
                                (const uint32_t*)dch, symmetric, pbc, d2_thresholds, n_edges, (int32_t*)dout);
    if (st) return st;
    return download(ctx, counts, dout, bytes, false);
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// ring interactions (include/mkamd_distance.h "ring interactions"; ring_pipeline.h)
// ---------------------------------------------------------------------------------------------
extern "C" int mkamd_ctx_set_ring_plan(mkamd_ctx* ctx, int avoid_mask, int64_t chunk_frames)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (avoid_mask < 0 || avoid_mask > 2) return fail(MKAMD_EINVAL, "ring plan: avoid mask 0, 1 (not the frame-lane kernels) or 2 (not the pair-lane kernels)");
    if (chunk_frames < 0) return fail(MKAMD_EINVAL, "ring plan: chunk_frames must not be negative");
    ctx->ring_avoid = avoid_mask;
    ctx->ring_chunk = (long long)chunk_frames;
    return MKAMD_OK;
} MK_API_CATCH

static mkamd::RingArgs ring_args(int kind, const float* d_coords, int64_t F, const float* d_box, const uint32_t* d_ring_atoms, int64_t n_ring_atoms,
                                 const uint32_t* d_starts1, int64_t n1, const uint32_t* d_starts2, const uint32_t* d_partners, int64_t n2,
                                 const uint32_t* d_emit, const float* thresholds)
{
    mkamd::RingArgs a;
    a.kind = kind;
    a.coords = d_coords; a.F = F; a.box = d_box;
    a.ring_atoms = d_ring_atoms; a.n_ring_atoms = n_ring_atoms;
    a.starts1 = d_starts1; a.n1 = n1; a.starts2 = d_starts2; a.partners = d_partners; a.n2 = n2;
    a.emit = kind == mkamd::RING_PIPI ? nullptr : d_emit;
    a.estride = kind == mkamd::RING_SIGMAHOLE ? 2 : 1;
    for (int i = 0; i < 4; ++i) a.thr[i] = thresholds[i];
    return a;
}

extern "C" int mkamd_ring_interactions_dev(mkamd_ctx* ctx, int kind, const float* d_coords, int64_t n_atoms, int64_t F, const float* d_box,
                                           const uint32_t* d_ring_atoms, int64_t n_ring_atoms, const uint32_t* d_starts1, int64_t n1,
                                           const uint32_t* d_starts2, const uint32_t* d_partners, int64_t n2, const float* thresholds,
                                           int64_t* frame_offsets, const uint32_t** d_pairs, const float** d_distang)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (n_atoms < 0 || F < 0 || n1 < 0 || n2 < 0 || n_ring_atoms < 0) return fail(MKAMD_EINVAL, "negative size");
    if (!frame_offsets || !d_pairs || !d_distang || !thresholds) return fail(MKAMD_EINVAL, "frame_offsets / d_pairs / d_distang / thresholds pointer is NULL");
    *d_pairs = nullptr;
    *d_distang = nullptr;
    std::string err;
    mkamd::RingDeviceSink<mkamd_ctx> sink{*ctx};
    static_assert(sizeof(long long) == sizeof(int64_t), "frame offsets are int64");
    st = mkamd::run_ring_interactions(*ctx, ring_args(kind, d_coords, F, d_box, d_ring_atoms, n_ring_atoms, d_starts1, n1, d_starts2, d_partners, n2,
                                                      d_partners, thresholds),
                                      (size_t)256 << 20, ctx->ring_chunk, (long long*)frame_offsets, sink, err, ctx->ring_avoid);
    if (st) return run_status(st, err);
    if (sink.size) {
        *d_pairs = static_cast<const uint32_t*>(sink.pairs);
        *d_distang = static_cast<const float*>(sink.distang);
    }
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_ring_interactions_host(mkamd_ctx* ctx, int kind, const float* coords, int64_t N, int64_t F, const float* box,
                                            const uint32_t* ring_atoms, int64_t n_ring_atoms, const uint32_t* starts1, int64_t n1,
                                            const uint32_t* starts2, const uint32_t* partners, int64_t n2, const float* thresholds,
                                            int64_t* frame_offsets, const uint32_t** pairs, const float** distang)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || n1 < 0 || n2 < 0 || n_ring_atoms < 0) return fail(MKAMD_EINVAL, "negative size");
    if (!frame_offsets || !pairs || !distang || !thresholds) return fail(MKAMD_EINVAL, "frame_offsets / pairs / distang / thresholds pointer is NULL");
    if (kind != mkamd::RING_PIPI && kind != mkamd::RING_CATIONPI && kind != mkamd::RING_SIGMAHOLE)
        return fail(MKAMD_EINVAL, "kind must be 0 (pi-pi), 1 (cation-pi) or 2 (sigma-hole)");
    ctx->ring_pairs_host.clear();
    ctx->ring_distang_host.clear();
    *pairs = nullptr;
    *distang = nullptr;
    for (int64_t f = 0; f <= F; ++f) frame_offsets[f] = 0;
    if (F == 0 || n1 == 0 || n2 == 0) return MKAMD_OK;
    const bool pipi = kind == mkamd::RING_PIPI;
    if (!coords || !ring_atoms || !starts1 || (pipi ? !starts2 : !partners)) return fail(MKAMD_EINVAL, "NULL pointer");
    const int64_t n_part = pipi ? 0 : n2 * (kind == mkamd::RING_SIGMAHOLE ? 2 : 1);
    if ((st = check_indices(ring_atoms, n_ring_atoms, N, "ring atom")) || (st = check_indices(partners, n_part, N, "partner atom"))) return st;
    void *dc, *db = nullptr, *da, *d1, *d2 = nullptr, *dp = nullptr, *de = nullptr;
    HostStage up(ctx, coords, N, F, {{ring_atoms, n_ring_atoms}, {partners, n_part}});
    if ((st = up.coords_to(WS_H_COORDS, &dc))) return st;
    if ((st = up.list_to(WS_R_ATOMS, ring_atoms, n_ring_atoms, &da))) return st;
    if (!pipi && (st = up.list_to(WS_R_PARTNERS, partners, n_part, &dp))) return st;
    if ((st = up.sync())) return st;
    if (!pipi && (st = upload(ctx, WS_R_EMIT, partners, (size_t)n_part * 4, &de))) return st;     // the list names atoms of the caller's array
    if (box && (st = upload(ctx, WS_H_BOX, box, (size_t)3 * F * 4, &db))) return st;
    if ((st = upload(ctx, WS_R_STARTS1, starts1, (size_t)(n1 + 1) * 4, &d1))) return st;
    if (pipi && (st = upload(ctx, WS_R_STARTS2, starts2, (size_t)(n2 + 1) * 4, &d2))) return st;
    std::string err;
    st = mkamd::run_ring_interactions(*ctx, ring_args(kind, (const float*)dc, F, (const float*)db, (const uint32_t*)da, n_ring_atoms, (const uint32_t*)d1, n1,
                                                      (const uint32_t*)d2, (const uint32_t*)dp, n2, (const uint32_t*)de, thresholds),
                                      (size_t)256 << 20, ctx->ring_chunk, (long long*)frame_offsets,
                                      mkamd::RingHostSink<mkamd_ctx>{*ctx, ctx->ring_pairs_host, ctx->ring_distang_host}, err, ctx->ring_avoid);
    if (st) return run_status(st, err);
    if (ctx->ring_pairs_host.empty()) return MKAMD_OK;
    *pairs = ctx->ring_pairs_host.data();
    *distang = ctx->ring_distang_host.data();
    return MKAMD_OK;
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// hydrogen bonds (include/mkamd_distance.h "hydrogen bonds"; hbond_pipeline.h)
// ---------------------------------------------------------------------------------------------
extern "C" int mkamd_ctx_set_hbond_plan(mkamd_ctx* ctx, int avoid_mask, int64_t chunk_frames)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (avoid_mask < 0 || avoid_mask > 2) return fail(MKAMD_EINVAL, "hbond plan: avoid mask 0, 1 (not the frame-lane kernels) or 2 (not the pair-lane kernels)");
    if (chunk_frames < 0) return fail(MKAMD_EINVAL, "hbond plan: chunk_frames must not be negative");
    ctx->hbond_avoid = avoid_mask;
    ctx->hbond_chunk = (long long)chunk_frames;
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_hbonds_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_atoms, int64_t F, const float* d_box, const uint32_t* donors,
                                int64_t n_donors, const uint32_t* acceptors, int64_t n_acceptors, const uint32_t* sel1, const uint32_t* sel2,
                                float dist_threshold, float angle_threshold, int intra, int ignore_hs, int64_t* frame_offsets, const int32_t** d_triples)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (n_atoms < 0 || F < 0 || n_donors < 0 || n_acceptors < 0) return fail(MKAMD_EINVAL, "negative size");
    if (!frame_offsets || !d_triples) return fail(MKAMD_EINVAL, "frame_offsets / d_triples pointer is NULL");
    *d_triples = nullptr;
    mkamd::HbondArgs a;
    a.coords = d_coords; a.n_atoms = n_atoms; a.F = F; a.box = d_box;
    a.donors = donors; a.nd = n_donors; a.acceptors = acceptors; a.na = n_acceptors; a.sel1 = sel1; a.sel2 = sel2;
    a.dist_threshold = dist_threshold; a.angle_threshold = angle_threshold; a.intra = intra != 0; a.ignore_hs = ignore_hs != 0;
    std::string err;
    mkamd::HbondDeviceSink<mkamd_ctx> sink{*ctx};
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "frame offsets are int64, triples int32");
    st = mkamd::run_hbonds(*ctx, a, (size_t)256 << 20, ctx->hbond_chunk, (long long*)frame_offsets, sink, err, ctx->hbond_avoid);
    if (st) return run_status(st, err);
    if (sink.size) *d_triples = static_cast<const int32_t*>(sink.triples);
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_hbonds_host(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const float* box, const uint32_t* donors, int64_t n_donors,
                                 const uint32_t* acceptors, int64_t n_acceptors, const uint32_t* sel1, const uint32_t* sel2, float dist_threshold,
                                 float angle_threshold, int intra, int ignore_hs, int64_t* frame_offsets, const int32_t** triples)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || n_donors < 0 || n_acceptors < 0) return fail(MKAMD_EINVAL, "negative size");
    if (!frame_offsets || !triples) return fail(MKAMD_EINVAL, "frame_offsets / triples pointer is NULL");
    ctx->hbond_triples_host.clear();
    *triples = nullptr;
    for (int64_t f = 0; f <= F; ++f) frame_offsets[f] = 0;
    if (dist_threshold != dist_threshold || angle_threshold != angle_threshold) return fail(MKAMD_EINVAL, "a threshold is NaN");
    if (F > 0x3fffffffLL || n_donors > 0x3fffffffLL || n_acceptors > 0x3fffffffLL) return fail(MKAMD_EINVAL, "too many frames, donor rows or acceptors (> 2^30)");
    if (F == 0 || n_donors == 0 || n_acceptors == 0) return MKAMD_OK;
    if (!coords || !donors || !acceptors || !sel1 || (!intra && !sel2)) return fail(MKAMD_EINVAL, "NULL pointer");
    const int64_t n_don = n_donors * (ignore_hs ? 1 : 2);
    if ((st = check_indices(donors, n_don, N, "donor atom")) || (st = check_indices(acceptors, n_acceptors, N, "acceptor atom"))) return st;
    void *dc, *db = nullptr;
    HostStage up(ctx, coords, N, F, {{donors, n_don}, {acceptors, n_acceptors}});
    if ((st = up.coords_to(WS_H_COORDS, &dc))) return st;
    if ((st = up.sync())) return st;
    if (box && (st = upload(ctx, WS_H_BOX, box, (size_t)3 * F * 4, &db))) return st;
    // the lists in the numbering of the rows that went up; the list names the caller's atoms
    std::vector<uint32_t> pd, pa, p1, p2;
    mkamd::HbondArgs a;
    a.coords = (const float*)dc; a.n_atoms = up.rows(); a.F = F; a.box = (const float*)db;
    a.donors = donors; a.nd = n_donors; a.acceptors = acceptors; a.na = n_acceptors; a.sel1 = sel1; a.sel2 = sel2;
    if (up.pk.on) {
        pd = up.pk.remap(donors, n_don); pa = up.pk.remap(acceptors, n_acceptors); p1 = up.pk.gather(sel1);
        if (!intra) p2 = up.pk.gather(sel2);
        a.donors = pd.data(); a.acceptors = pa.data(); a.sel1 = p1.data(); a.sel2 = intra ? nullptr : p2.data();
        a.names = up.pk.uniq.data();
    }
    a.dist_threshold = dist_threshold; a.angle_threshold = angle_threshold; a.intra = intra != 0; a.ignore_hs = ignore_hs != 0;
    std::string err;
    st = mkamd::run_hbonds(*ctx, a, (size_t)256 << 20, ctx->hbond_chunk, (long long*)frame_offsets,
                           mkamd::HbondHostSink<mkamd_ctx>{*ctx, ctx->hbond_triples_host}, err, ctx->hbond_avoid);
    if (st) return run_status(st, err);
    if (!ctx->hbond_triples_host.empty()) *triples = ctx->hbond_triples_host.data();
    return MKAMD_OK;
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// bond guesser (include/mkamd_distance.h "bond guesser"; bond_pipeline.h)
// ---------------------------------------------------------------------------------------------
extern "C" int mkamd_ctx_set_bond_plan(mkamd_ctx* ctx, int avoid_mask)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (avoid_mask < 0 || avoid_mask > 2) return fail(MKAMD_EINVAL, "bond plan: avoid mask 0, 1 (not a thread per owner) or 2 (not a wave per owner)");
    ctx->bond_avoid = avoid_mask;
    return MKAMD_OK;
} MK_API_CATCH

static int guess_bonds_impl(mkamd_ctx* ctx, const float* d_coords, const float* d_radii, const uint32_t* d_is_h, int64_t n_atoms, double grid_cutoff,
                            double max_boxes, double cutoff_incr, mkamd::BondResult& R, double* grid)
{
    mkamd::BondArgs a;
    a.coords = d_coords; a.radii = d_radii; a.is_h = d_is_h; a.n = n_atoms;
    a.grid_cutoff = grid_cutoff; a.max_boxes = max_boxes; a.cutoff_incr = cutoff_incr;
    std::string err;
    const int st = mkamd::run_guess_bonds(*ctx, a, R, err, ctx->bond_avoid);
    if (grid) {
        for (int ax = 0; ax < 3; ++ax) grid[ax] = (double)R.boxes[ax];
        grid[3] = R.pairdist;
    }
    return run_status(st, err);
}

extern "C" int mkamd_guess_bonds_dev(mkamd_ctx* ctx, const float* d_coords, const float* d_radii, const uint32_t* d_is_hydrogen, int64_t n_atoms,
                                     double grid_cutoff, double max_boxes, double cutoff_incr, int64_t* n, const int32_t** d_pairs, double* grid)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (!n || !d_pairs) return fail(MKAMD_EINVAL, "n / d_pairs pointer is NULL");
    *n = 0;
    *d_pairs = nullptr;
    static_assert(sizeof(int) == sizeof(int32_t) && sizeof(unsigned) == sizeof(uint32_t), "the list is int32, the flags uint32");
    mkamd::BondResult R;
    if ((st = guess_bonds_impl(ctx, d_coords, d_radii, d_is_hydrogen, n_atoms, grid_cutoff, max_boxes, cutoff_incr, R, grid))) return st;
    *n = R.n_pairs;
    if (R.n_pairs) *d_pairs = R.pairs;
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_guess_bonds_host(mkamd_ctx* ctx, const float* coords, const float* radii, const uint32_t* is_hydrogen, int64_t n_atoms,
                                      double grid_cutoff, double max_boxes, double cutoff_incr, int64_t* n, const int32_t** pairs, double* grid)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (!n || !pairs) return fail(MKAMD_EINVAL, "n / pairs pointer is NULL");
    *n = 0;
    *pairs = nullptr;
    ctx->bond_pairs_host.clear();
    if (n_atoms < 0) return fail(MKAMD_EINVAL, "negative size");
    if (n_atoms >= 0x80000000LL) return fail(MKAMD_EINVAL, "too many atoms (>= 2^31)");
    if (n_atoms > 0 && (!coords || !radii || !is_hydrogen)) return fail(MKAMD_EINVAL, "NULL pointer");
    void *dc = nullptr, *dr = nullptr, *dh = nullptr;
    if (n_atoms > 0) {
        if ((st = upload(ctx, WS_H_COORDS, coords, (size_t)n_atoms * 12, &dc)) || (st = upload(ctx, WS_H_SIGMAS, radii, (size_t)n_atoms * 4, &dr)) ||
            (st = upload(ctx, WS_H_OFFSETS, is_hydrogen, (size_t)n_atoms * 4, &dh)))
            return st;
    }
    mkamd::BondResult R;
    if ((st = guess_bonds_impl(ctx, (const float*)dc, (const float*)dr, (const uint32_t*)dh, n_atoms, grid_cutoff, max_boxes, cutoff_incr, R, grid))) {
        (void)hipStreamSynchronize(ctx->stream);                      // (the uploads read the caller's arrays)
        return st;
    }
    if (R.n_pairs) {
        ctx->bond_pairs_host.resize((size_t)R.n_pairs * 2);
        if ((st = ctx->to_host(ctx->bond_pairs_host.data(), R.pairs, (size_t)R.n_pairs * 8))) return st;
        *pairs = ctx->bond_pairs_host.data();
    } else {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    *n = R.n_pairs;
    return MKAMD_OK;
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// steric clashes (include/mkamd_distance.h "steric clashes"; clash_pipeline.h)
// ---------------------------------------------------------------------------------------------
extern "C" int mkamd_ctx_set_clash_plan(mkamd_ctx* ctx, int avoid_mask)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (avoid_mask < 0 || avoid_mask > 2) return fail(MKAMD_EINVAL, "clash plan: avoid mask 0, 1 (not a thread per owner) or 2 (not a wave per owner)");
    ctx->clash_avoid = avoid_mask;
    return MKAMD_OK;
} MK_API_CATCH

static int find_clashes_impl(mkamd_ctx* ctx, const float* d_coords, const float* d_radii, const uint32_t* d_sel1, const uint32_t* d_sel2, int64_t n_atoms,
                             int self_mode, const uint32_t* d_ex_start, const uint32_t* d_ex_partner, double overlap, double cutoff, double max_boxes,
                             mkamd::ClashResult& R, double* info)
{
    mkamd::ClashArgs a;
    a.coords = d_coords; a.radii = d_radii; a.sel1 = d_sel1; a.sel2 = d_sel2; a.n = n_atoms; a.self_mode = self_mode ? 1 : 0;
    a.ex_start = d_ex_start; a.ex_partner = d_ex_partner;
    a.overlap = overlap; a.cutoff = cutoff; a.max_boxes = max_boxes;
    std::string err;
    const int st = mkamd::run_find_clashes(*ctx, a, R, err, ctx->clash_avoid);
    if (info) {
        for (int ax = 0; ax < 3; ++ax) info[ax] = (double)R.boxes[ax];
        info[3] = R.side;
        info[4] = (double)R.max_occ;
        info[5] = (double)R.n_owners;
    }
    return run_status(st, err);
}

extern "C" int mkamd_find_clashes_dev(mkamd_ctx* ctx, const float* d_coords, const float* d_radii, const uint32_t* d_sel1, const uint32_t* d_sel2,
                                      int64_t n_atoms, int self_mode, const uint32_t* d_ex_start, const uint32_t* d_ex_partner, double overlap,
                                      double cutoff, double max_boxes, int64_t* n, const int32_t** d_pairs, const float** d_dist,
                                      const float** d_overlap, double* info)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (!n || !d_pairs || !d_dist || !d_overlap) return fail(MKAMD_EINVAL, "n / d_pairs / d_dist / d_overlap pointer is NULL");
    *n = 0;
    *d_pairs = nullptr; *d_dist = nullptr; *d_overlap = nullptr;
    mkamd::ClashResult R;
    if ((st = find_clashes_impl(ctx, d_coords, d_radii, d_sel1, d_sel2, n_atoms, self_mode, d_ex_start, d_ex_partner, overlap, cutoff, max_boxes, R, info)))
        return st;
    *n = R.n_pairs;
    if (R.n_pairs) { *d_pairs = R.pairs; *d_dist = R.dists; *d_overlap = R.overs; }
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_find_clashes_host(mkamd_ctx* ctx, const float* coords, const float* radii, const uint32_t* sel1, const uint32_t* sel2, int64_t n_atoms,
                                       int self_mode, const uint32_t* ex_start, const uint32_t* ex_partner, double overlap, double cutoff,
                                       double max_boxes, int64_t* n, const int32_t** pairs, const float** dist, const float** overlap_out, double* info)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (!n || !pairs || !dist || !overlap_out) return fail(MKAMD_EINVAL, "n / pairs / dist / overlap pointer is NULL");
    *n = 0;
    *pairs = nullptr; *dist = nullptr; *overlap_out = nullptr;
    ctx->clash_pairs_host.clear(); ctx->clash_dist_host.clear(); ctx->clash_over_host.clear();
    if (n_atoms < 0) return fail(MKAMD_EINVAL, "negative size");
    if (n_atoms >= 0x80000000LL) return fail(MKAMD_EINVAL, "too many atoms (>= 2^31)");
    if (n_atoms > 0 && (!coords || !radii || !sel1 || (!self_mode && !sel2))) return fail(MKAMD_EINVAL, "NULL pointer");
    if ((ex_start == nullptr) != (ex_partner == nullptr)) return fail(MKAMD_EINVAL, "exclusions: both arrays or neither");
    size_t n_ex = 0;
    if (ex_start && n_atoms > 0) {                                    // a CSR of ascending rows over n_atoms atoms, partners below n_atoms
        if (ex_start[0] != 0) return fail(MKAMD_EINVAL, "exclusions: ex_start[0] must be 0");
        for (int64_t a = 0; a < n_atoms; ++a) {
            if (ex_start[a + 1] < ex_start[a]) return fail(MKAMD_EINVAL, "exclusions: ex_start must not decrease");
            for (uint32_t k = ex_start[a]; k < ex_start[a + 1]; ++k) {
                if (ex_partner[k] >= (uint64_t)n_atoms) return fail(MKAMD_EINVAL, "exclusions: partner index out of range");
                if (k > ex_start[a] && ex_partner[k] <= ex_partner[k - 1]) return fail(MKAMD_EINVAL, "exclusions: a row must ascend strictly");
            }
        }
        n_ex = ex_start[n_atoms];
    }
    void *dc = nullptr, *dr = nullptr, *d1 = nullptr, *d2 = nullptr, *des = nullptr, *dep = nullptr;
    if (n_atoms > 0) {
        if ((st = upload(ctx, WS_H_COORDS, coords, (size_t)n_atoms * 12, &dc)) || (st = upload(ctx, WS_H_SIGMAS, radii, (size_t)n_atoms * 4, &dr)) ||
            (st = upload(ctx, WS_H_OFFSETS, sel1, (size_t)n_atoms * 4, &d1)))
            return st;
        if (!self_mode && (st = upload(ctx, WS_H_ORIGINS, sel2, (size_t)n_atoms * 4, &d2))) return st;
        if (ex_start && ((st = upload(ctx, WS_H_BOX, ex_start, ((size_t)n_atoms + 1) * 4, &des)) || (st = upload(ctx, WS_H_CENTERS, ex_partner, n_ex * 4, &dep))))
            return st;
    }
    mkamd::ClashResult R;
    if ((st = find_clashes_impl(ctx, (const float*)dc, (const float*)dr, (const uint32_t*)d1, (const uint32_t*)d2, n_atoms, self_mode, (const uint32_t*)des,
                                (const uint32_t*)dep, overlap, cutoff, max_boxes, R, info))) {
        (void)hipStreamSynchronize(ctx->stream);                      // (the uploads read the caller's arrays)
        return st;
    }
    if (R.n_pairs) {
        const size_t k = (size_t)R.n_pairs;
        std::vector<int> p(2 * k);
        std::vector<float> d(k), o(k);
        if ((st = ctx->to_host(p.data(), R.pairs, k * 8)) || (st = ctx->to_host(d.data(), R.dists, k * 4)) || (st = ctx->to_host(o.data(), R.overs, k * 4)))
            return st;
        std::vector<size_t> order(k);
        for (size_t i = 0; i < k; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) {
            if (o[x] != o[y]) return o[x] > o[y];                     // the largest overlap first
            if (p[2 * x] != p[2 * y]) return p[2 * x] < p[2 * y];
            return p[2 * x + 1] < p[2 * y + 1];
        });
        ctx->clash_pairs_host.resize(2 * k); ctx->clash_dist_host.resize(k); ctx->clash_over_host.resize(k);
        for (size_t i = 0; i < k; ++i) {
            ctx->clash_pairs_host[2 * i] = p[2 * order[i]];
            ctx->clash_pairs_host[2 * i + 1] = p[2 * order[i] + 1];
            ctx->clash_dist_host[i] = d[order[i]];
            ctx->clash_over_host[i] = o[order[i]];
        }
        *pairs = ctx->clash_pairs_host.data(); *dist = ctx->clash_dist_host.data(); *overlap_out = ctx->clash_over_host.data();
    } else {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    *n = R.n_pairs;
    return MKAMD_OK;
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// proximity selections (include/mkamd_distance.h "proximity selections"; within_pipeline.h)
// ---------------------------------------------------------------------------------------------
extern "C" int mkamd_ctx_set_within_plan(mkamd_ctx* ctx, int avoid_mask)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (avoid_mask < 0 || avoid_mask > 2) return fail(MKAMD_EINVAL, "within plan: avoid mask 0, 1 (not the all-pairs kernel) or 2 (not the cell list)");
    ctx->within_avoid = avoid_mask;
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_within_distance_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_atoms, int64_t n_frames, const uint32_t* d_sel1, int64_t n1,
                                         const uint32_t* d_sel2, int64_t n2, float cutoff, const float* d_gate, uint8_t* d_out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    mkamd::WithinArgs a;
    a.coords = d_coords; a.n_atoms = n_atoms; a.n_frames = n_frames;
    a.sel1 = d_sel1; a.n1 = n1; a.sel2 = d_sel2; a.n2 = n2;
    a.cutoff = cutoff; a.gate = d_gate; a.out = d_out;
    mkamd::WithinResult R;
    std::string err;
    st = mkamd::run_within(*ctx, a, R, err, ctx->within_avoid);
    return run_status(st, err);
} MK_API_CATCH

extern "C" int mkamd_within_distance_host(mkamd_ctx* ctx, const float* coords, int64_t n_atoms, int64_t n_frames, const uint32_t* sel1, int64_t n1,
                                          const uint32_t* sel2, int64_t n2, float cutoff, const float* gate, uint8_t* out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    const int64_t N = n_atoms, F = n_frames;
    if (N < 0 || F < 0 || n1 < 0 || n2 < 0) return fail(MKAMD_EINVAL, "negative size");
    if (N >= 0x80000000LL) return fail(MKAMD_EINVAL, "too many atoms (>= 2^31)");
    ctx->note_dist_kernel("");
    if (F == 0 || n1 == 0) return MKAMD_OK;
    if (!out || !sel1 || (n2 > 0 && !sel2)) return fail(MKAMD_EINVAL, "NULL pointer");
    if (n2 == 0) { memset(out, 0, (size_t)F * (size_t)n1); return MKAMD_OK; }
    if (!coords) return fail(MKAMD_EINVAL, "NULL pointer");
    if ((st = check_indices(sel1, n1, N, "sel1")) || (st = check_indices(sel2, n2, N, "sel2"))) return st;
    void *dxyz, *d1, *d2, *dg = nullptr, *dout;
    HostStage up(ctx, coords, N, F, {{sel1, n1}, {sel2, n2}}, /*always=*/true);      // only the rows of sel1 and sel2 travel
    if ((st = upload_frame_major(ctx, WS_H_COORDS, WS_WI_XYZ, up.host_rows(), 3 * up.rows(), F, &dxyz))) return st;
    if ((st = up.list_to(WS_D_SEL1, sel1, n1, &d1))) return st;
    if ((st = up.list_to(WS_D_SEL2, sel2, n2, &d2))) return st;
    if ((st = up.sync())) return st;
    if (gate && (st = upload(ctx, WS_WI_GATE, gate, (size_t)F * 6 * 4, &dg))) return st;
    if ((st = ctx->ensure(WS_H_OUT, (size_t)F * (size_t)n1, &dout, 0))) return st;
    if ((st = mkamd_within_distance_dev(ctx, (const float*)dxyz, up.rows(), F, (const uint32_t*)d1, n1, (const uint32_t*)d2, n2, cutoff, (const float*)dg,
                                        (uint8_t*)dout))) {
        (void)hipStreamSynchronize(ctx->stream);                      // (the uploads read the caller's arrays)
        return st;
    }
    return download(ctx, out, dout, (size_t)F * (size_t)n1, false);
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// secondary structure (include/mkamd_distance.h "secondary structure"; dssp_pipeline.h)
// ---------------------------------------------------------------------------------------------
extern "C" int mkamd_ctx_set_dssp_plan(mkamd_ctx* ctx, int avoid_mask)
try {
    if (!ctx) return fail(MKAMD_EINVAL, "ctx is NULL");
    if (avoid_mask < 0 || avoid_mask > 7 || (avoid_mask & 3) == 3)
        return fail(MKAMD_EINVAL, "dssp plan: avoid mask 1 (not the frame-lane energy kernel) or 2 (not the acceptor-lane one), + 4 (chunks of 64 frames)");
    ctx->dssp_avoid = avoid_mask;
    return MKAMD_OK;
} MK_API_CATCH

extern "C" int mkamd_dssp_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_atoms, int64_t F, const uint32_t* d_ca, const uint32_t* d_nco,
                              const int32_t* d_proline, const int32_t* d_chain, int64_t R, int simplified, uint8_t* d_out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (n_atoms < 0 || F < 0 || R < 0) return fail(MKAMD_EINVAL, "negative size");
    std::string err;
    st = mkamd::run_dssp(*ctx, d_coords, F, d_ca, d_nco, d_proline, d_chain, R, simplified, d_out, err, ctx->dssp_avoid,
                         [](const mkamd::DsspWs&, long long, long long) { return 0; });
    return run_status(st, err);
} MK_API_CATCH

extern "C" int mkamd_dssp_host(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const uint32_t* ca, const uint32_t* nco,
                               const int32_t* proline, const int32_t* chain, int64_t R, int simplified, uint8_t* out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || R < 0) return fail(MKAMD_EINVAL, "negative size");
    if (F > 0x3fffffffLL) return fail(MKAMD_EINVAL, "too many frames (>= 2^30)");
    if (R > mkamd::DSSP_MAX_RESIDUES) return fail(MKAMD_EINVAL, "too many residues (> 2^18)");
    if (F == 0 || R == 0) return MKAMD_OK;
    if (!coords || !ca || !nco || !proline || !chain || !out) return fail(MKAMD_EINVAL, "NULL pointer");
    if ((st = check_indices(ca, R, N, "ca: atom")) || (st = check_indices(nco, 3 * R, N, "nco: atom"))) return st;
    void *dc, *dca, *dnco, *dpro, *dchain, *dout;
    HostStage up(ctx, coords, N, F, {{ca, R}, {nco, 3 * R}});          // only the backbone atoms' rows travel
    if ((st = up.coords_to(WS_H_COORDS, &dc))) return st;
    if ((st = up.list_to(WS_D_SEL1, ca, R, &dca))) return st;
    if ((st = up.list_to(WS_SS_NCO, nco, 3 * R, &dnco))) return st;
    if ((st = up.sync())) return st;
    if ((st = upload(ctx, WS_SS_PROLINE, proline, (size_t)R * 4, &dpro))) return st;
    if ((st = upload(ctx, WS_D_CHAINS, chain, (size_t)R * 4, &dchain))) return st;
    if ((st = ctx->ensure(WS_H_OUT, (size_t)F * (size_t)R, &dout, 0))) return st;
    st = mkamd_dssp_dev(ctx, (const float*)dc, up.rows(), F, (const uint32_t*)dca, (const uint32_t*)dnco, (const int32_t*)dpro,
                        (const int32_t*)dchain, R, simplified, (uint8_t*)dout);
    if (st) {
        (void)hipStreamSynchronize(ctx->stream);                      // (the uploads read the caller's arrays)
        return st;
    }
    return download(ctx, out, dout, (size_t)F * (size_t)R, false);
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// dihedral angles (include/mkamd_distance.h "dihedral angles"; dihedral_pipeline.h)
// ---------------------------------------------------------------------------------------------
extern "C" int mkamd_dihedrals_dev(mkamd_ctx* ctx, const float* d_coords, int64_t n_atoms, int64_t F, const float* d_box, int64_t n_box_frames,
                                   const uint32_t* d_quads, int64_t D, int mode, float* d_out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (n_atoms < 0 || F < 0 || D < 0) return fail(MKAMD_EINVAL, "negative size");
    if (d_box && n_box_frames != F) return fail(MKAMD_EINVAL, "box must be [3, n_frames]: n_box_frames differs from n_frames");
    if (F > 0 && D > 0 && (!d_coords || !d_quads || !d_out)) return fail(MKAMD_EINVAL, "NULL pointer");
    std::string err;
    st = mkamd::run_dihedrals(*ctx, d_coords, F, d_box, d_box != nullptr, d_quads, D, mode, d_out, err, (ctx->dist_avoid >> 10) & 3);
    return run_status(st, err);
} MK_API_CATCH

extern "C" int mkamd_dihedrals_host(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const float* box, int64_t n_box_frames,
                                    const uint32_t* quads, int64_t D, int mode, float* out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || D < 0) return fail(MKAMD_EINVAL, "negative size");
    if (mode < mkamd::DIH_TERMS || mode > mkamd::DIH_SINCOS) return fail(MKAMD_EINVAL, "mode must be 0 (terms), 1 (radians), 2 (degrees) or 3 (sincos)");
    if (box && n_box_frames != F) return fail(MKAMD_EINVAL, "box must be [3, n_frames]: n_box_frames differs from n_frames");
    if (F == 0 || D == 0) return MKAMD_OK;
    if (!coords || !quads || !out) return fail(MKAMD_EINVAL, "NULL pointer");
    if (F > 0x3fffffffLL || D > 0x3fffffffLL || (double)F * (double)D * (double)mkamd::dih_width(mode) >= 1.0e18) return fail(MKAMD_EINVAL, "result too large");
    if ((st = check_indices(quads, 4 * D, N, "quads: atom"))) return st;
    // the reference wraps only where the box is not all zeros (dihedral.py:dihedralAngle)
    bool wrap = false;
    if (box) for (int64_t i = 0; i < 3 * F && !wrap; ++i) wrap = !(box[i] == 0.0f);
    void *dc, *db = nullptr, *dq, *dout;
    HostStage up(ctx, coords, N, F, {{quads, 4 * D}});
    if ((st = up.coords_to(WS_H_COORDS, &dc))) return st;
    if ((st = up.list_to(WS_D_SEL1, quads, 4 * D, &dq))) return st;
    if ((st = up.sync())) return st;
    if (wrap && (st = upload(ctx, WS_H_BOX, box, (size_t)3 * F * 4, &db))) return st;
    const size_t bytes = (size_t)F * (size_t)D * (size_t)mkamd::dih_width(mode) * 4;
    if ((st = ctx->ensure(WS_H_OUT, bytes, &dout, 0))) return st;
    st = mkamd_dihedrals_dev(ctx, (const float*)dc, up.rows(), F, (const float*)db, F, (const uint32_t*)dq, D, mode, (float*)dout);
    if (st) return st;
    return download(ctx, out, dout, bytes, false);
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// group moments (include/mkamd_distance.h "group moments"; moments_pipeline.h)
// ---------------------------------------------------------------------------------------------
static mkamd::MomArgs mom_args(const float* d_xyz, int64_t N, int64_t F, const double* d_affine, const uint32_t* d_atoms, const uint32_t* d_offsets,
                               const float* d_weights, int64_t G, int64_t n_sel, int64_t max_group)
{
    mkamd::MomArgs a;
    a.xyz = d_xyz; a.n_atoms = N; a.n_frames = F; a.affine = d_affine;
    a.atoms = d_atoms; a.offsets = d_offsets; a.weights = d_weights;
    a.n_groups = G; a.n_sel = n_sel; a.max_group = max_group;
    return a;
}

extern "C" int mkamd_group_moments_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t N, int64_t F, const double* d_affine, const uint32_t* d_atoms,
                                       const uint32_t* d_offsets, const float* d_weights, int64_t G, int64_t n_sel, int64_t max_group, int mode,
                                       float* d_out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    std::string err;
    st = mkamd::run_group_moments(*ctx, mom_args(d_xyz, N, F, d_affine, d_atoms, d_offsets, d_weights, G, n_sel, max_group), mode, d_out, err,
                                  (ctx->dist_avoid >> 12) & 3);
    return run_status(st, err);
} MK_API_CATCH

extern "C" int mkamd_fluctuation_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t N, int64_t F, const double* d_affine, const uint32_t* d_atoms,
                                     int64_t n_sel, const uint32_t* d_offsets, int64_t G, int64_t max_group, const double* d_ref, double* d_out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    std::string err;
    st = mkamd::run_fluctuation(*ctx, mom_args(d_xyz, N, F, d_affine, d_atoms, d_offsets, nullptr, d_offsets ? G : 0, n_sel, d_offsets ? max_group : 1),
                                d_ref, d_out, err, (ctx->dist_avoid >> 12) & 3);
    return run_status(st, err);
} MK_API_CATCH

// What the two host forms share: the rows of the atoms that `atoms` and `alnsel` name, packed ([M, 3, F]), uploaded and transposed to
// frame-major [F, M, 3]; the lists in the packed numbering; each frame's transform onto alnref where an alignment is asked for.
struct MomHostInputs {
    void *dxyz = nullptr, *datoms = nullptr, *doffs = nullptr, *dw = nullptr, *daff = nullptr;
    int64_t rows = 0, max_group = 1;
};

static int mom_host_inputs(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const uint32_t* alnsel, const float* alnref, int64_t n_aln,
                           const uint32_t* atoms, int64_t n_sel, const uint32_t* offsets, int64_t G, const float* weights, MomHostInputs& in)
{
    int st;
    if (!coords || !atoms || (alnsel && !alnref)) return fail(MKAMD_EINVAL, "NULL pointer");
    if ((st = check_indices(atoms, n_sel, N, "atoms: atom")) || (alnsel && (st = check_indices(alnsel, n_aln, N, "alnsel: atom")))) return st;
    if (offsets) {
        if (offsets[0] != 0 || (int64_t)offsets[G] != n_sel) return fail(MKAMD_EINVAL, "offsets must start at 0 and end at the number of group atoms");
        for (int64_t g = 0; g < G; ++g) {
            if (offsets[g + 1] <= offsets[g]) return fail(MKAMD_EINVAL, "an empty group (or decreasing offsets)");
            in.max_group = std::max<int64_t>(in.max_group, (int64_t)offsets[g + 1] - (int64_t)offsets[g]);
        }
    }
    HostStage up(ctx, coords, N, F, {{atoms, n_sel}, {alnsel, n_aln}}, /*always=*/true);
    in.rows = up.rows();
    if ((st = upload_frame_major(ctx, WS_A_SLAB, WS_A_XYZ, up.host_rows(), 3 * in.rows, F, &in.dxyz))) return st;
    if ((st = up.list_to(WS_M_ATOMS, atoms, n_sel, &in.datoms))) return st;
    if (offsets && (st = upload(ctx, WS_M_OFFS, offsets, (size_t)(G + 1) * 4, &in.doffs))) return st;
    if (weights && (st = upload(ctx, WS_M_W, weights, (size_t)n_sel * 4, &in.dw))) return st;
    if (!alnsel) return up.sync();
    std::vector<uint32_t> rs((size_t)n_aln);
    for (int64_t k = 0; k < n_aln; ++k) rs[(size_t)k] = (uint32_t)k;
    void *dsel, *drefsel, *dref;
    if ((st = up.list_to(WS_A_SEL, alnsel, n_aln, &dsel))) return st;
    if ((st = upload(ctx, WS_A_REFSEL, rs.data(), (size_t)n_aln * 4, &drefsel))) return st;
    if ((st = upload(ctx, WS_A_REF, alnref, (size_t)n_aln * 12, &dref))) return st;
    if ((st = ctx->ensure(WS_A_AFFINE, (size_t)F * 12 * 8, &in.daff))) return st;
    if ((st = up.sync())) return st;                                 // (rs is read by then as well)
    return mkamd_align_transforms_dev(ctx, (const float*)in.dxyz, in.rows, F, (const float*)dref, n_aln, 1, (const uint32_t*)dsel,
                                      (const uint32_t*)drefsel, n_aln, nullptr, F, 0, 0, (double*)in.daff, nullptr);
}

extern "C" int mkamd_group_moments_host(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const uint32_t* alnsel, const float* alnref,
                                        int64_t n_aln, const uint32_t* atoms, const uint32_t* offsets, const float* weights, int64_t G, int mode,
                                        float* out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || G < 0 || n_aln < 0) return fail(MKAMD_EINVAL, "negative size");
    if (mode < mkamd::MOM_CENTER || mode > mkamd::MOM_SPHERICAL) return fail(MKAMD_EINVAL, "mode must be 0 (center), 1 (gyration) or 2 (spherical)");
    if (F > 0x3fffffffLL || G > 0x3fffffffLL) return fail(MKAMD_EINVAL, "too many frames or groups (>= 2^30)");
    if (F == 0 || G == 0) return MKAMD_OK;
    if (!offsets || !out) return fail(MKAMD_EINVAL, "NULL pointer");
    const int64_t n_sel = offsets[G];
    MomHostInputs in;
    if ((st = mom_host_inputs(ctx, coords, N, F, alnsel, alnref, n_aln, atoms, n_sel, offsets, G, weights, in))) return st;
    const size_t bytes = (size_t)F * (mode == mkamd::MOM_SPHERICAL ? 3 : mode == mkamd::MOM_GYRATION ? 4 * (size_t)G : 3 * (size_t)G) * 4;
    void* dout;
    if ((st = ctx->ensure(WS_H_OUT, bytes, &dout, 0))) return st;
    st = mkamd_group_moments_dev(ctx, (const float*)in.dxyz, in.rows, F, (const double*)in.daff, (const uint32_t*)in.datoms, (const uint32_t*)in.doffs,
                                 (const float*)in.dw, G, n_sel, in.max_group, mode, (float*)dout);
    if (st) return st;
    return download(ctx, out, dout, bytes, false);
} MK_API_CATCH

extern "C" int mkamd_fluctuation_host(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const uint32_t* alnsel, const float* alnref,
                                      int64_t n_aln, const uint32_t* atoms, int64_t n_sel, const uint32_t* offsets, int64_t G, const double* ref,
                                      double* out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || G < 0 || n_aln < 0 || n_sel < 0) return fail(MKAMD_EINVAL, "negative size");
    if (F > 0x3fffffffLL || G > 0x3fffffffLL || n_sel > 0x3fffffffLL) return fail(MKAMD_EINVAL, "too many frames, groups or atoms");
    if (F == 0 || n_sel == 0 || (offsets && G == 0)) return MKAMD_OK;
    if (!out) return fail(MKAMD_EINVAL, "NULL pointer");
    MomHostInputs in;
    if ((st = mom_host_inputs(ctx, coords, N, F, alnsel, alnref, n_aln, atoms, n_sel, offsets, G, nullptr, in))) return st;
    void *dref = nullptr, *dout;
    if (ref) {
        if ((st = upload(ctx, WS_M_REFIN, ref, (size_t)n_sel * 24, &dref))) return st;
    }
    const size_t bytes = (size_t)F * (size_t)(offsets ? G : n_sel) * 8;
    if ((st = ctx->ensure(WS_H_OUT, bytes, &dout, 0))) return st;
    st = mkamd_fluctuation_dev(ctx, (const float*)in.dxyz, in.rows, F, (const double*)in.daff, (const uint32_t*)in.datoms, n_sel,
                               (const uint32_t*)in.doffs, G, in.max_group, (const double*)dref, (double*)dout);
    if (st) return st;
    return download(ctx, out, dout, bytes, false);
} MK_API_CATCH

// ---------------------------------------------------------------------------------------------
// periodic wrap (include/mkamd_distance.h "periodic wrap"; wrap_pipeline.h)
// ---------------------------------------------------------------------------------------------
extern "C" int64_t mkamd_wrap_small_max(mkamd_ctx* ctx) { return (int64_t)mkamd::wrap_small_max(ctx ? (ctx->dist_avoid >> 14) & 3 : 0); }

extern "C" int mkamd_wrap_box_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t N, int64_t F, const float* d_box, const uint32_t* d_starts, int64_t G,
                                  const uint32_t* d_large, int64_t n_large, const uint32_t* d_centersel, int64_t n_c, const float* center,
                                  float* d_out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (n_c == 0 && !center && N > 0 && F > 0 && G > 0) return fail(MKAMD_EINVAL, "NULL pointer (neither a centre selection nor a centre)");
    mkamd::WrapArgs a;
    a.xyz = d_xyz; a.n_atoms = N; a.n_frames = F; a.box = d_box; a.starts = d_starts; a.n_groups = G; a.large = d_large; a.n_large = n_large;
    a.centersel = d_centersel; a.n_centersel = n_c; a.out = d_out;
    if (n_c == 0 && center) { a.center[0] = center[0]; a.center[1] = center[1]; a.center[2] = center[2]; }
    std::string err;
    st = mkamd::run_wrap_box(*ctx, a, err, (ctx->dist_avoid >> 14) & 3);
    return run_status(st, err);
} MK_API_CATCH

extern "C" int mkamd_wrap_box_host(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const float* box, const uint32_t* rows, int64_t n_rows,
                                   const uint32_t* starts, int64_t G, const uint32_t* centersel, int64_t n_c, const float* center, float* out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (N < 0 || F < 0 || G < 0 || n_c < 0 || n_rows < 0) return fail(MKAMD_EINVAL, "negative size");
    if (N > 0x3fffffffLL || F > 0x3fffffffLL) return fail(MKAMD_EINVAL, "too many atoms or frames (>= 2^30)");
    const int64_t M = rows ? n_rows : N;                             // atoms that travel
    if (F == 0 || M == 0) return MKAMD_OK;
    if (!coords || !box || !out || (n_c > 0 && !centersel) || (n_c == 0 && !center)) return fail(MKAMD_EINVAL, "NULL pointer");
    if (rows) {
        if ((st = check_indices(rows, n_rows, N, "rows: atom"))) return st;
        for (int64_t k = 1; k < n_rows; ++k)
            if (rows[k] <= rows[k - 1]) return fail(MKAMD_EINVAL, "rows must be strictly increasing atom indices");
    }
    if (const char* e = mkamd::wrap_check_starts(starts, G, M)) return fail(MKAMD_EINVAL, e);
    if ((st = check_indices(centersel, n_c, N, "centersel: atom"))) return st;
    if (rows)
        for (int64_t k = 0; k < n_c; ++k)
            if (!std::binary_search(rows, rows + n_rows, centersel[k])) return fail(MKAMD_EINVAL, "centersel names an atom that is not among the rows");
    HostStage up(ctx, coords, N, F, {{rows, n_rows}}, /*always=*/rows != nullptr);
    void *dxyz, *dslab, *dbox, *dstarts, *dlarge = nullptr, *dsel = nullptr;
    if ((st = upload_frame_major(ctx, WS_A_SLAB, WS_A_XYZ, up.host_rows(), 3 * M, F, &dxyz))) return st;
    const int64_t small_max = mkamd_wrap_small_max(ctx);
    std::vector<uint32_t> large;
    for (int64_t g = 0; g < G; ++g)
        if ((int64_t)starts[g + 1] - (int64_t)starts[g] > small_max) large.push_back((uint32_t)g);
    if ((st = upload(ctx, WS_W_STARTS, starts, (size_t)(G + 1) * 4, &dstarts))) return st;
    if (!large.empty() && (st = upload(ctx, WS_W_LARGE, large.data(), large.size() * 4, &dlarge))) return st;
    if (n_c > 0 && (st = up.list_to(WS_W_SEL, centersel, n_c, &dsel))) return st;
    if ((st = upload(ctx, WS_H_BOX, box, (size_t)3 * F * 4, &dbox))) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));                      // (`large`, the packed rows and the rewritten selection are read by then)
    up.held.clear();
    st = mkamd_wrap_box_dev(ctx, (const float*)dxyz, M, F, (const float*)dbox, (const uint32_t*)dstarts, G, (const uint32_t*)dlarge,
                            (int64_t)large.size(), (const uint32_t*)dsel, n_c, center, (float*)dxyz);
    if (st) return st;
    // back to the reference's [M][3][F]
    const size_t bytes = (size_t)3 * M * F * 4;
    if ((st = ctx->ensure(WS_A_SLAB, bytes, &dslab))) return st;
    if ((st = mkamd_frames_to_items_dev(ctx, ctx->stream, (const float*)dxyz, F, 3 * M, 3 * M, 1.0f, (float*)dslab))) return st;
    return download(ctx, out, dslab, bytes, true);
} MK_API_CATCH

// ... of triclinic boxes (wrap_cell_pipeline.h)
extern "C" int64_t mkamd_wrap_cell_max_steps(void) { return (int64_t)mkamd::WRAP_CELL_MAX_STEPS; }

extern "C" int mkamd_wrap_cell_dev(mkamd_ctx* ctx, const float* d_xyz, int64_t N, int64_t F, const double* d_boxvectors, const uint32_t* d_starts,
                                   int64_t G, const uint32_t* d_large, int64_t n_large, const uint32_t* d_centersel, int64_t n_c,
                                   const float* center, int mode, float* d_out, int* d_status)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (n_c == 0 && !center && N > 0 && F > 0 && G > 0) return fail(MKAMD_EINVAL, "NULL pointer (neither a centre selection nor a centre)");
    mkamd::WrapCellArgs c;
    mkamd::WrapArgs& a = c.w;
    a.xyz = d_xyz; a.n_atoms = N; a.n_frames = F; a.starts = d_starts; a.n_groups = G; a.large = d_large; a.n_large = n_large;
    a.centersel = d_centersel; a.n_centersel = n_c; a.out = d_out;
    if (n_c == 0 && center) { a.center[0] = center[0]; a.center[1] = center[1]; a.center[2] = center[2]; }
    c.boxvectors = d_boxvectors; c.mode = mode; c.status = d_status;
    if (d_status) HIP_TRY(hipMemsetAsync(d_status, 0, mkamd::WRAP_CELL_NSTATUS * sizeof(int), ctx->stream));
    std::string err;
    st = mkamd::run_wrap_cell(*ctx, c, err, (ctx->dist_avoid >> 14) & 3);
    return run_status(st, err);
} MK_API_CATCH

extern "C" int mkamd_wrap_cell_host(mkamd_ctx* ctx, const float* coords, int64_t N, int64_t F, const double* boxvectors, const uint32_t* rows,
                                    int64_t n_rows, const uint32_t* starts, int64_t G, const uint32_t* centersel, int64_t n_c,
                                    const float* center, int mode, float* out)
try {
    int st = check_ctx(ctx);
    if (st) return st;
    if (mode < 0 || mode > 2) return fail(MKAMD_EINVAL, "mode must be 0 (rectangular), 1 (compact) or 2 (triclinic)");
    if (N < 0 || F < 0 || G < 0 || n_c < 0 || n_rows < 0) return fail(MKAMD_EINVAL, "negative size");
    if (N > 0x3fffffffLL || F > 0x3fffffffLL) return fail(MKAMD_EINVAL, "too many atoms or frames (>= 2^30)");
    const int64_t M = rows ? n_rows : N;                             // atoms that travel
    if (F == 0 || M == 0) return MKAMD_OK;
    if (!coords || !boxvectors || !out || (n_c > 0 && !centersel) || (n_c == 0 && !center)) return fail(MKAMD_EINVAL, "NULL pointer");
    if (const char* e = mkamd::wrap_cell_check_boxvectors(boxvectors, F)) return fail(MKAMD_EINVAL, e);
    if (rows) {
        if ((st = check_indices(rows, n_rows, N, "rows: atom"))) return st;
        for (int64_t k = 1; k < n_rows; ++k)
            if (rows[k] <= rows[k - 1]) return fail(MKAMD_EINVAL, "rows must be strictly increasing atom indices");
    }
    if (const char* e = mkamd::wrap_check_starts(starts, G, M)) return fail(MKAMD_EINVAL, e);
    if ((st = check_indices(centersel, n_c, N, "centersel: atom"))) return st;
    if (rows)
        for (int64_t k = 0; k < n_c; ++k)
            if (!std::binary_search(rows, rows + n_rows, centersel[k])) return fail(MKAMD_EINVAL, "centersel names an atom that is not among the rows");
    HostStage up(ctx, coords, N, F, {{rows, n_rows}}, /*always=*/rows != nullptr);
    void *dxyz, *dslab, *dbox, *dstarts, *dstatus, *dlarge = nullptr, *dsel = nullptr;
    if ((st = upload_frame_major(ctx, WS_A_SLAB, WS_A_XYZ, up.host_rows(), 3 * M, F, &dxyz))) return st;
    const int64_t small_max = mkamd_wrap_small_max(ctx);
    std::vector<uint32_t> large;
    for (int64_t g = 0; g < G; ++g)
        if ((int64_t)starts[g + 1] - (int64_t)starts[g] > small_max) large.push_back((uint32_t)g);
    if ((st = upload(ctx, WS_W_STARTS, starts, (size_t)(G + 1) * 4, &dstarts))) return st;
    if (!large.empty() && (st = upload(ctx, WS_W_LARGE, large.data(), large.size() * 4, &dlarge))) return st;
    if (n_c > 0 && (st = up.list_to(WS_W_SEL, centersel, n_c, &dsel))) return st;
    if ((st = upload(ctx, WS_W_BOXV, boxvectors, (size_t)9 * F * 8, &dbox))) return st;
    if ((st = ctx->ensure(WS_W_STATUS, mkamd::WRAP_CELL_NSTATUS * sizeof(int), &dstatus))) return st;
    HIP_TRY(hipStreamSynchronize(ctx->stream));                      // (`large`, the packed rows and the rewritten selection are read by then)
    up.held.clear();
    st = mkamd_wrap_cell_dev(ctx, (const float*)dxyz, M, F, (const double*)dbox, (const uint32_t*)dstarts, G, (const uint32_t*)dlarge,
                             (int64_t)large.size(), (const uint32_t*)dsel, n_c, center, mode, (float*)dxyz, (int*)dstatus);
    if (st) return st;
    // back to the reference's [M][3][F]
    const size_t bytes = (size_t)3 * M * F * 4;
    if ((st = ctx->ensure(WS_A_SLAB, bytes, &dslab))) return st;
    if ((st = mkamd_frames_to_items_dev(ctx, ctx->stream, (const float*)dxyz, F, 3 * M, 3 * M, 1.0f, (float*)dslab))) return st;
    if ((st = download(ctx, out, dslab, bytes, true))) return st;
    int status[mkamd::WRAP_CELL_NSTATUS];
    if ((st = download(ctx, status, dstatus, sizeof status, false))) return st;
    if (const char* e = mkamd::wrap_cell_status_error(status)) return fail(MKAMD_EINVAL, e);
    return MKAMD_OK;
} MK_API_CATCH

#ifdef MK_PHASE_TIMERS
// diagnostics build only (mk_diagnostics.h; tools/phase_timers.py): read and clear the per-phase cycle sums of the tile kernel
extern "C" int mkamd_debug_phase_cycles(unsigned long long* out8)
{
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(mkamd::g_phase_cycles), 8 * sizeof(unsigned long long)) != hipSuccess) return 1;
    unsigned long long z[8] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(mkamd::g_phase_cycles), z, sizeof z) == hipSuccess ? 0 : 1;
}
#endif
