// hbond_pipeline.h -- launch plan of the hydrogen-bond kernels (hbond_kernels.h), written against the backend concept of pipeline.h so
// that the product (capi.hip) and the test emulator (tests/emu/emu_hbonds.cpp) run the same plan.
//
// Once per call, on the host: the donor rows whose heavy atom is in a selection, their class, the three acceptor sublists and the
// numbering of the tiles (hbond_kernels.h "THE PAIR SPACE") -- work proportional to donors + acceptors, which is why the index lists and
// the selection flags are HOST arrays in both entry points; what goes to the device is one table of 20 bytes per row, 4 per sublist
// entry and 4 per tile.  Per chunk of frames: count (a 64-bit mask per tile and frame, a counter per row and frame) -> k_contacts_scan
// (per-frame prefixes over the rows, the frames' totals) -> the totals reach the host, which sizes the list -> fill.
// A chunk needs 8 bytes per (tile, frame), 4 per (row, frame) and 16 per frame, so the frames per chunk follow from a byte budget and the
// workspace stays bounded whatever frames x pairs is.
#pragma once
#include "hbond_kernels.h"
#include "pipeline.h"

#include <algorithm>
#include <string>
#include <vector>

namespace mkamd {

enum { HB_AVOID_FRAMES = 1, HB_AVOID_PAIRS = 2 };       // `avoid`: the tests walk both lane assignments over the same shapes

struct HbondArgs {
    const float* coords = nullptr;         // device float32 [N][3][F]
    long long n_atoms = 0, F = 0;
    const float* box = nullptr;            // device float32 [3][F]; null: every axis open
    // the lists, HOST arrays in the numbering of `coords`' rows
    const unsigned* donors = nullptr;      // [nd][2] (heavy atom, hydrogen); [nd][1] with ignore_hs
    long long nd = 0;
    const unsigned* acceptors = nullptr;   // [na]
    long long na = 0;
    const unsigned* sel1 = nullptr;        // [n_atoms] flags
    const unsigned* sel2 = nullptr;        // [n_atoms] flags (not read where intra)
    const unsigned* names = nullptr;       // HOST [n_atoms] or null: what the result calls the atom of a row (the host entry's packed rows)
    float dist_threshold = 2.5f, angle_threshold = 120.0f;
    bool intra = false, ignore_hs = false;
};

// where the chunks' triples go: reserve(n, &dev) before the fill kernel, commit(dev, n) after it
template <class BE>
struct HbondHostSink {
    BE& be;
    std::vector<int>& triples;
    int reserve(size_t n, void** d) { return be.ensure(WS_H_OUT, n * 12, d, 0); }
    int commit(void* d, size_t n)
    {
        const size_t old = triples.size();
        triples.resize(old + n * 3);
        return be.to_host(triples.data() + old, d, n * 12);
    }
};
template <class BE>
struct HbondDeviceSink {
    BE& be;
    size_t size = 0;                       // triples written so far
    void* triples = nullptr;               // context-owned: grows by copying
    int reserve(size_t n, void** d)
    {
        const int st = be.grow_keep(WS_HB_TRIPLES, (size + n) * 12, size * 12, &triples);
        *d = static_cast<char*>(triples) + size * 12;
        return st;
    }
    int commit(void*, size_t n) { size += n; return 0; }
};

// Lanes along the acceptors of a frame instead of the frames?  Only calls of fewer than 64 frames leave lanes of the frame kernels idle;
// they go to the pair kernels when those fill their lanes better.
inline bool hbond_takes_pairs(long long F, long long entries, long long tiles)
{
    if (F >= WAVE) return false;
    return (double)entries / (double)(tiles * HB_TILE) > (double)F / (double)WAVE;
}

// frame_offsets int64 [F + 1] (host): the bonds of frame f are triples [frame_offsets[f], frame_offsets[f + 1]) of the list, in the
// reference's order (donors outer, acceptors inner).  Every index of the lists is checked against n_atoms here.  `budget_bytes` bounds the chunk's workspace; `chunk_frames` > 0 forces the frames per chunk (the tests cross chunk
// boundaries at tiny sizes).
template <class BE, class Sink>
int run_hbonds(BE& be, const HbondArgs& a, size_t budget_bytes, long long chunk_frames, long long* frame_offsets, Sink&& sink, std::string& err,
               int avoid = 0)
{
    const long long F = a.F, nd = a.nd, na = a.na, N = a.n_atoms;
    if (F < 0 || nd < 0 || na < 0 || N < 0) { err = "negative size"; return ST_EINVAL; }
    if (F > 0x3fffffffLL) { err = "too many frames (> 2^30)"; return ST_EINVAL; }
    for (long long f = 0; f <= F; ++f) frame_offsets[f] = 0;
    if (a.dist_threshold != a.dist_threshold || a.angle_threshold != a.angle_threshold) { err = "a threshold is NaN"; return ST_EINVAL; }
    if (nd > 0x3fffffffLL || na > 0x3fffffffLL) { err = "too many donor rows or acceptors (> 2^30)"; return ST_EINVAL; }
    if (F == 0 || nd == 0 || na == 0) return ST_OK;
    if (!a.coords || !a.donors || !a.acceptors || !a.sel1 || (!a.intra && !a.sel2)) { err = "NULL pointer"; return ST_EINVAL; }
    if (N > 0xffffffffLL) { err = "too many atoms"; return ST_EINVAL; }
    int st;
    const int ds = a.ignore_hs ? 1 : 2;                              // columns of a donor row
    const unsigned *donors = a.donors, *acceptors = a.acceptors, *sel1 = a.sel1, *sel2 = a.intra ? a.sel1 : a.sel2;
    for (long long i = 0; i < nd * ds; ++i) if (donors[i] >= (unsigned long long)N) { err = "donor atom index out of range"; return ST_EINVAL; }
    for (long long i = 0; i < na; ++i) if (acceptors[i] >= (unsigned long long)N) { err = "acceptor atom index out of range"; return ST_EINVAL; }

    // the sublists: the loop tests `== 0` for an intra call and `== 1` otherwise, so a flag of 2 is in an intra selection only
    auto in1 = [&](unsigned atom) { return a.intra ? sel1[atom] != 0u : sel1[atom] == 1u; };
    auto in2 = [&](unsigned atom) { return !a.intra && sel2[atom] == 1u; };
    HbPlan P{};
    std::vector<unsigned> acc;                                         // class 0: acceptors in sel1; 1: in sel2; 2: in either
    for (int c = 0; c < 3; ++c) {
        P.off[c] = (unsigned)acc.size();
        if (c && a.intra) continue;
        for (long long j = 0; j < na; ++j) {
            const bool i1 = in1(acceptors[j]), i2 = in2(acceptors[j]);
            if (c == 0 ? i1 : c == 1 ? i2 : (i1 || i2)) acc.push_back(acceptors[j]);
        }
        P.len[c] = (unsigned)acc.size() - P.off[c];
    }
    std::vector<HbRow> rows;                                           // the reference's order
    std::vector<unsigned> crow[3];
    unsigned long long tiles = 0;
    for (long long d = 0; d < nd; ++d) {
        const unsigned heavy = donors[d * ds], ref = donors[d * ds + ds - 1];
        const bool d1 = in1(heavy), d2 = in2(heavy);
        const int c = a.intra ? (d1 ? 0 : -1) : (d1 && d2) ? 2 : d2 ? 0 : d1 ? 1 : -1;      // heavy in sel2: against the acceptors of sel1
        if (c < 0 || P.len[c] == 0) continue;
        crow[c].push_back((unsigned)rows.size());
        rows.push_back(HbRow{heavy, ref, (unsigned)tiles, (unsigned)c});
        tiles += (P.len[c] + HB_TILE - 1) / HB_TILE;
        if (tiles > (1ull << 25)) { err = "too many allowed donor-acceptor pairs for one call (> 2^31); split the lists"; return ST_EINVAL; }
    }
    if (rows.empty()) return ST_OK;
    // one table goes up: the rows | the rows of each class | the sublists | the row of every tile | the names
    const size_t R = rows.size(), o_crow = R * 4, o_acc = o_crow + R, o_trow = o_acc + acc.size(), o_names = o_trow + (size_t)tiles;
    std::vector<unsigned> table(o_names + (a.names ? (size_t)N : 0));
    static_assert(sizeof(HbRow) == 16, "a row is four words of the table");
    std::copy((const unsigned*)rows.data(), (const unsigned*)rows.data() + R * 4, table.begin());
    std::copy(acc.begin(), acc.end(), table.begin() + (long long)o_acc);
    if (a.names) std::copy(a.names, a.names + N, table.begin() + (long long)o_names);
    unsigned long long work = 0, entries = 0;
    const size_t HB_G = (size_t)hbond_group(!a.ignore_hs);
    for (int c = 0, at = 0; c < 3; ++c) {
        P.coff[c] = (unsigned)at;
        P.cnum[c] = (unsigned)crow[c].size();
        std::copy(crow[c].begin(), crow[c].end(), table.begin() + (long long)o_crow + at);
        at += (int)crow[c].size();
        P.wstart[c] = (unsigned)work;
        work += (unsigned long long)((crow[c].size() + HB_G - 1) / HB_G) * ((P.len[c] + HB_TILE - 1) / HB_TILE);
        entries += (unsigned long long)crow[c].size() * P.len[c];
    }
    P.wstart[3] = (unsigned)work;
    for (size_t r = 0; r < R; ++r) {
        const unsigned end = r + 1 < R ? rows[r + 1].tile0 : (unsigned)tiles;
        for (unsigned t = rows[r].tile0; t < end; ++t) table[o_trow + t] = (unsigned)r;
    }
    const bool by_pairs = (avoid & HB_AVOID_FRAMES) || (!(avoid & HB_AVOID_PAIRS) && hbond_takes_pairs(F, (long long)entries, (long long)tiles));

    // frames per chunk
    const size_t per_frame = (size_t)tiles * 8 + R * 4 + 16;
    if (per_frame * WAVE > ((size_t)1 << 32)) { err = "too many allowed donor-acceptor pairs for one call; split the lists"; return ST_EINVAL; }
    long long chunk = std::max<long long>(WAVE, (long long)(budget_bytes / per_frame) / WAVE * WAVE);
    if (chunk_frames > 0) chunk = chunk_frames;
    chunk = std::min(std::min(chunk, F), by_pairs ? 65535LL : 65535LL * WAVE);       // (the frames of a chunk are the grids' y)
    const long long pitch = (chunk + WAVE - 1) / WAVE * WAVE;
    void *dtab = nullptr, *msk = nullptr, *cnt = nullptr, *tot = nullptr, *base = nullptr, *out = nullptr;
    if ((st = be.ensure(WS_HB_TABLE, table.size() * 4, &dtab, 0)) || (st = be.to_device(dtab, table.data(), table.size() * 4))) return st;
    if ((st = be.ensure(WS_HB_MASK, (size_t)tiles * (size_t)pitch * 8, &msk, 0))) return st;
    if ((st = be.ensure(WS_HB_CNT, R * (size_t)pitch * 4, &cnt, 0))) return st;
    if ((st = be.ensure(WS_HB_TOT, (size_t)pitch * 8, &tot, 0))) return st;
    if ((st = be.ensure(WS_HB_BASE, (size_t)pitch * 8, &base, 0))) return st;
    HbThr T;
    T.d2 = a.dist_threshold * a.dist_threshold;                      // `float dist_threshold` squared in float
    T.ang = (float)((double)a.angle_threshold / 57.29578);           // the float widened, divided, narrowed once
    be.note_dist_kernel(by_pairs ? "mkamd::k_hbond_count_pairs" : "mkamd::k_hbond_count_frames");
    const unsigned* tab = (const unsigned*)dtab;
    const HbRow* rws = (const HbRow*)tab;
    const unsigned *cr = tab + o_crow, *ac = tab + o_acc, *tr = tab + o_trow, *nm = a.names ? tab + o_names : nullptr;
    const long long nt = (long long)tiles, nr = (long long)R;
    std::vector<unsigned long long> totals((size_t)pitch), bases((size_t)pitch);
    for (long long f0 = 0; f0 < F; f0 += chunk) {
        const long long fc = std::min(chunk, F - f0);
        // count
        if ((st = be.fill(cnt, 0, R * (size_t)pitch * 4))) return st;
        if (by_pairs) {
            const dim3 grid((unsigned)((nt + 3) / 4), (unsigned)fc), block(HC_THREADS);
            auto go = [&](auto kern) { return be.launch(kern, grid, block, a.coords, F, f0, pitch, a.box, rws, tr, nt, ac, P, T, (unsigned long long*)msk, (unsigned*)cnt); };
            st = a.ignore_hs ? go(k_hbond_count_pairs<false>) : go(k_hbond_count_pairs<true>);
        } else {
            // (frames past the chunk store nothing: their masks are never read -- the fill stops at fc)
            const dim3 grid((unsigned)((work + 3) / 4), (unsigned)((fc + WAVE - 1) / WAVE)), block(HC_THREADS);
            auto go = [&](auto kern) { return be.launch(kern, grid, block, a.coords, F, f0, fc, pitch, a.box, rws, cr, ac, P, T, (unsigned long long*)msk, (unsigned*)cnt); };
            st = a.ignore_hs ? go(k_hbond_count_frames<false, hbond_group(false)>) : go(k_hbond_count_frames<true, hbond_group(true)>);
        }
        if (st) return st;
        if ((st = be.launch(k_contacts_scan, dim3((unsigned)(pitch / WAVE)), dim3(CS_WAVES * WAVE), (unsigned*)cnt, nr, pitch, fc, (unsigned long long*)tot))) return st;
        if ((st = be.to_host(totals.data(), tot, (size_t)pitch * 8))) return st;
        unsigned long long run = 0;
        for (long long i = 0; i < pitch; ++i) { bases[(size_t)i] = run; run += i < fc ? totals[(size_t)i] : 0ull; }
        for (long long i = 0; i < fc; ++i) frame_offsets[f0 + i + 1] = frame_offsets[f0 + i] + (long long)totals[(size_t)i];
        if (run == 0) continue;
        if ((st = sink.reserve((size_t)run, &out))) return st;
        if ((st = be.to_device(base, bases.data(), (size_t)pitch * 8))) return st;
        {
            const dim3 grid = by_pairs ? dim3((unsigned)((nr + HF_THREADS - 1) / HF_THREADS), (unsigned)fc) : dim3((unsigned)((nr + 3) / 4), (unsigned)((fc + WAVE - 1) / WAVE));
            const dim3 block(HF_THREADS);
            auto go = [&](auto kern) {
                return be.launch(kern, grid, block, pitch, fc, rws, nr, ac, P, (const unsigned long long*)msk, (const unsigned*)cnt,
                                 (const unsigned long long*)tot, (const unsigned long long*)base, nm, a.ignore_hs ? 0 : 1, (int*)out);
            };
            st = by_pairs ? go(k_hbond_fill<false>) : go(k_hbond_fill<true>);
        }
        if (st) return st;
        if ((st = sink.commit(out, (size_t)run))) return st;
    }
    return ST_OK;
}

}  // namespace mkamd
