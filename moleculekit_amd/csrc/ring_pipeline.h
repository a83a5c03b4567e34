// ring_pipeline.h -- launch plan of the ring-interaction kernels (ring_kernels.h), written against the backend concept of pipeline.h so
// that the product (capi.hip) and the test emulator (tests/emu/emu_rings.cpp) run the same plan.
//
// Per chunk of frames: pre-pass (ring records, partner records) -> count (a 64-bit mask per tile of 64 pairs and frame) ->
// k_contacts_scan (per-frame prefixes over the tiles, the frames' totals) -> the totals reach the host, which sizes the lists ->
// fill.  What a chunk needs is proportional to its frames: (9 floats per ring + 3 or 6 per partner + 12 bytes per tile) per frame, so
// the frames per chunk follow from a byte budget and the workspace stays bounded whatever frames x pairs is.
#pragma once
#include "ring_kernels.h"
#include "pipeline.h"

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

namespace mkamd {

enum { RING_AVOID_FRAMES = 1, RING_AVOID_PAIRS = 2 };   // `avoid`: the tests walk both lane assignments over the same shapes

// Lanes along the pairs of a frame instead of the frames?  Only calls of fewer than 64 frames leave lanes of the frame kernels idle;
// they go to the pair kernels when those fill their lanes better (pose scoring: one frame, 150 x 3 rings).
inline bool ring_takes_pairs(long long F, long long P)
{
    if (F >= WAVE) return false;
    return (double)P / (double)((P + RING_TILE - 1) / RING_TILE * RING_TILE) > (double)F / (double)WAVE;
}

struct RingArgs {
    int kind = RING_PIPI;
    const float* coords = nullptr;         // device float32 [N][3][F]
    long long F = 0;
    const float* box = nullptr;            // device float32 [3][F]; null: every axis open
    const unsigned* ring_atoms = nullptr;  // device: the rings' atoms, concatenated (pi-pi: both lists)
    long long n_ring_atoms = 0;
    const unsigned* starts1 = nullptr;     // device [n1 + 1]: offsets of the first list's rings into ring_atoms
    long long n1 = 0;
    const unsigned* starts2 = nullptr;     // pi-pi, device [n2 + 1]: the second list's
    const unsigned* partners = nullptr;    // cation-pi: device [n2] atoms; sigma-hole: [n2][2] (halogen, bonded atom)
    long long n2 = 0;
    const unsigned* emit = nullptr;        // cation-pi / sigma-hole: what the list names the partner by (emit[r2 * estride])
    int estride = 1;
    float thr[4] = {0, 0, 0, 0};           // pi-pi: dist1, angle1 max, dist2, angle2 min; the others: dist, angle min
};

// where the chunks' lists go: reserve(n, &pairs, &distang) before the fill kernel, commit(pairs, distang, n) after it
template <class BE>
struct RingHostSink {
    BE& be;
    std::vector<unsigned>& pairs;
    std::vector<float>& distang;
    int reserve(size_t n, void** dp, void** dd)
    {
        const int st = be.ensure(WS_H_OUT, n * 8, dp, 0);
        return st ? st : be.ensure(WS_R_OUT2, n * 8, dd, 0);
    }
    int commit(void* dp, void* dd, size_t n)
    {
        const size_t old = pairs.size();
        pairs.resize(old + n * 2);
        distang.resize(old + n * 2);
        const int st = be.to_host(pairs.data() + old, dp, n * 8);
        return st ? st : be.to_host(distang.data() + old, dd, n * 8);
    }
};
template <class BE>
struct RingDeviceSink {
    BE& be;
    size_t size = 0;                       // pairs written so far
    void *pairs = nullptr, *distang = nullptr;
    int reserve(size_t n, void** dp, void** dd)
    {
        int st = be.grow_keep(WS_R_PAIRS, (size + n) * 8, size * 8, &pairs);
        if (!st) st = be.grow_keep(WS_R_DISTANG, (size + n) * 8, size * 8, &distang);
        *dp = static_cast<char*>(pairs) + size * 8;
        *dd = static_cast<char*>(distang) + size * 8;
        return st;
    }
    int commit(void*, void*, size_t n) { size += n; return 0; }
};

// frame_offsets int64 [F + 1] (host): the pairs of frame f are [frame_offsets[f], frame_offsets[f + 1]) of the lists, in the
// reference's order (r1 outer, r2 inner).  The atom indices (ring_atoms, partners) are NOT checked here: the host entry point does.
// `budget_bytes` bounds the chunk's workspace; `chunk_frames` > 0 forces the frames per chunk (the tests cross chunk boundaries at
// tiny sizes).
template <class BE, class Sink>
int run_ring_interactions(BE& be, const RingArgs& a, size_t budget_bytes, long long chunk_frames, long long* frame_offsets, Sink&& sink,
                          std::string& err, int avoid = 0)
{
    const long long F = a.F, n1 = a.n1, n2 = a.n2;
    if (F < 0 || n1 < 0 || n2 < 0 || a.n_ring_atoms < 0) { err = "negative size"; return ST_EINVAL; }
    for (long long f = 0; f <= F; ++f) frame_offsets[f] = 0;
    if (a.kind != RING_PIPI && a.kind != RING_CATIONPI && a.kind != RING_SIGMAHOLE) { err = "kind must be 0 (pi-pi), 1 (cation-pi) or 2 (sigma-hole)"; return ST_EINVAL; }
    if (F == 0 || n1 == 0 || n2 == 0) return ST_OK;
    const bool pipi = a.kind == RING_PIPI;
    if (!a.coords || !a.ring_atoms || !a.starts1 || (pipi ? !a.starts2 : !a.partners)) { err = "NULL pointer"; return ST_EINVAL; }
    if (F > 0x3fffffffLL) { err = "too many frames (>= 2^30)"; return ST_EINVAL; }
    if (n1 > 0x3fffffffLL || n2 > 0x3fffffffLL || n1 * n2 > 0x3fffffffLL) { err = "too many ring pairs (> 2^30); split the lists"; return ST_EINVAL; }
    if (a.n_ring_atoms > 0x7fffffffLL) { err = "too many ring atoms"; return ST_EINVAL; }
    for (int i = 0; i < 4; ++i) if (a.thr[i] != a.thr[i]) { err = "a threshold is NaN"; return ST_EINVAL; }
    int st;
    // the rings: offsets inside the atom list, at least three atoms each (the normal reads the first three)
    std::vector<unsigned> hs((size_t)(n1 + 1) + (pipi ? (size_t)(n2 + 1) : 0));
    if ((st = be.to_host(hs.data(), a.starts1, (size_t)(n1 + 1) * 4))) return st;
    if (pipi && (st = be.to_host(hs.data() + n1 + 1, a.starts2, (size_t)(n2 + 1) * 4))) return st;
    for (int list = 0; list < (pipi ? 2 : 1); ++list) {
        const unsigned* s = hs.data() + (list ? n1 + 1 : 0);
        const long long n = list ? n2 : n1;
        for (long long r = 0; r < n; ++r) {
            if (s[r + 1] < s[r] || (long long)s[r + 1] > a.n_ring_atoms) { err = "ring offsets must not decrease and must end inside ring_atoms"; return ST_EINVAL; }
            if (s[r + 1] - s[r] < 3) { err = "a ring has fewer than 3 atoms (the plane normal needs three)"; return ST_EINVAL; }
        }
    }
    const long long P = n1 * n2, tiles = (P + RING_TILE - 1) / RING_TILE, R = n1 + (pipi ? n2 : 0);
    const int PW = ring_part_width(a.kind);
    const bool by_pairs = (avoid & RING_AVOID_FRAMES) || (!(avoid & RING_AVOID_PAIRS) && ring_takes_pairs(F, P));
    // frames per chunk
    const size_t per_frame = ((size_t)R * RING_REC + (pipi ? 0 : (size_t)n2 * PW)) * 4 + (size_t)tiles * 12 + 16;
    if (per_frame * WAVE > ((size_t)1 << 32)) { err = "too many ring pairs for one call; split the lists"; return ST_EINVAL; }
    long long chunk = std::max<long long>(WAVE, (long long)(budget_bytes / per_frame) / WAVE * WAVE);
    if (chunk_frames > 0) chunk = chunk_frames;
    chunk = std::min(std::min(chunk, F), by_pairs ? 65535LL : 65535LL * WAVE);       // (the frames of a chunk are the grids' y)
    const long long pitch = (chunk + WAVE - 1) / WAVE * WAVE;
    void *rec = nullptr, *part = nullptr, *msk = nullptr, *cnt = nullptr, *tot = nullptr, *base = nullptr, *dp = nullptr, *dd = nullptr;
    if ((st = be.ensure(WS_R_REC, (size_t)R * RING_REC * (size_t)pitch * 4, &rec, 0))) return st;
    if (!pipi && (st = be.ensure(WS_R_PART, (size_t)n2 * PW * (size_t)pitch * 4, &part, 0))) return st;
    if ((st = be.ensure(WS_R_MASK, (size_t)tiles * (size_t)pitch * 8, &msk, 0))) return st;
    if ((st = be.ensure(WS_R_CNT, (size_t)tiles * (size_t)pitch * 4, &cnt, 0))) return st;
    if ((st = be.ensure(WS_R_TOT, (size_t)pitch * 8, &tot, 0))) return st;
    if ((st = be.ensure(WS_R_BASE, (size_t)pitch * 8, &base, 0))) return st;
    RingThr T;
    T.d1sq = a.thr[0] * a.thr[0];                                    // `float dist_threshold` squared in float
    T.a1 = a.thr[1];
    T.d2sq = pipi ? a.thr[2] * a.thr[2] : T.d1sq;
    T.a2 = pipi ? a.thr[3] : a.thr[1];
    be.note_dist_kernel(by_pairs ? "mkamd::k_ring_count_pairs" : "mkamd::k_ring_count_frames");
    const float* recf = (const float*)rec;
    const float* partf = (const float*)part;
    const unsigned* starts2 = pipi ? a.starts2 : a.starts1;          // (never read in the other kinds)
    const long long n2r = pipi ? n2 : 0;                             // rings of the second list
    std::vector<unsigned long long> totals((size_t)pitch), bases((size_t)pitch);
    auto by_kind = [&](auto&& go) { return a.kind == RING_PIPI ? go(std::integral_constant<int, RING_PIPI>{})
                                         : a.kind == RING_CATIONPI ? go(std::integral_constant<int, RING_CATIONPI>{})
                                                                   : go(std::integral_constant<int, RING_SIGMAHOLE>{}); };
    for (long long f0 = 0; f0 < F; f0 += chunk) {
        const long long fc = std::min(chunk, F - f0);
        // pre-pass
        {
            const dim3 grid = by_pairs ? dim3((unsigned)((R + RP_THREADS - 1) / RP_THREADS), (unsigned)fc) : dim3((unsigned)((R + 3) / 4), (unsigned)(pitch / WAVE));
            const dim3 block(RP_THREADS);
            st = by_pairs ? be.launch(k_ring_prepass<false>, grid, block, a.coords, F, f0, fc, pitch, a.ring_atoms, a.starts1, n1, starts2, n2r, (float*)rec)
                          : be.launch(k_ring_prepass<true>, grid, block, a.coords, F, f0, fc, pitch, a.ring_atoms, a.starts1, n1, starts2, n2r, (float*)rec);
            if (st) return st;
        }
        if (!pipi) {
            const dim3 grid = by_pairs ? dim3((unsigned)((n2 + RP_THREADS - 1) / RP_THREADS), (unsigned)fc) : dim3((unsigned)((n2 + 3) / 4), (unsigned)(pitch / WAVE));
            const dim3 block(RP_THREADS);
            auto go = [&](auto kern) { return be.launch(kern, grid, block, a.coords, F, f0, fc, pitch, a.partners, n2, (float*)part); };
            st = a.kind == RING_CATIONPI ? (by_pairs ? go(k_ring_partners<RING_CATIONPI, false>) : go(k_ring_partners<RING_CATIONPI, true>))
                                         : (by_pairs ? go(k_ring_partners<RING_SIGMAHOLE, false>) : go(k_ring_partners<RING_SIGMAHOLE, true>));
            if (st) return st;
        }
        // count
        {
            const dim3 grid((unsigned)((tiles + 3) / 4), (unsigned)(by_pairs ? fc : pitch / WAVE)), block(RC_THREADS);
            st = by_kind([&](auto kind_) {
                constexpr int K = decltype(kind_)::value;
                auto go = [&](auto kern) {
                    return be.launch(kern, grid, block, recf, partf, pitch, fc, a.box, F, f0, a.starts1, n1, starts2, n2, T, (unsigned long long*)msk, (unsigned*)cnt);
                };
                return by_pairs ? go(k_ring_count_pairs<K>) : go(k_ring_count_frames<K>);
            });
            if (st) return st;
        }
        if ((st = be.launch(k_contacts_scan, dim3((unsigned)(pitch / WAVE)), dim3(CS_WAVES * WAVE), (unsigned*)cnt, tiles, pitch, fc, (unsigned long long*)tot))) return st;
        if ((st = be.to_host(totals.data(), tot, (size_t)pitch * 8))) return st;
        unsigned long long run = 0;
        for (long long i = 0; i < pitch; ++i) { bases[(size_t)i] = run; run += i < fc ? totals[(size_t)i] : 0ull; }
        for (long long i = 0; i < fc; ++i) frame_offsets[f0 + i + 1] = frame_offsets[f0 + i] + (long long)totals[(size_t)i];
        if (run == 0) continue;
        if ((st = sink.reserve((size_t)run, &dp, &dd))) return st;
        if ((st = be.to_device(base, bases.data(), (size_t)pitch * 8))) return st;
        {
            const dim3 grid = by_pairs ? dim3((unsigned)((tiles + RF_THREADS - 1) / RF_THREADS), (unsigned)fc) : dim3((unsigned)((tiles + 3) / 4), (unsigned)(pitch / WAVE));
            const dim3 block(RF_THREADS);
            st = by_kind([&](auto kind_) {
                constexpr int K = decltype(kind_)::value;
                auto go = [&](auto kern) {
                    return be.launch(kern, grid, block, recf, partf, pitch, fc, a.box, F, f0, n1, n2, T, (const unsigned long long*)msk, (const unsigned*)cnt,
                                     (const unsigned long long*)base, a.emit, a.estride, (uint2*)dp, (float2*)dd);
                };
                return by_pairs ? go(k_ring_fill<K, false>) : go(k_ring_fill<K, true>);
            });
            if (st) return st;
        }
        if ((st = sink.commit(dp, dd, (size_t)run))) return st;
    }
    return ST_OK;
}

}  // namespace mkamd
