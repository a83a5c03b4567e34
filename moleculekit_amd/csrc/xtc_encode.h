// xtc_encode.h -- XTC coordinate COMPRESSION on the device: the reference writer's bytes (DESIGN.md "device XTC writer").
//
// What the reference does per frame in xdrfile_compress_coord_float (xdrfile.cpp:985-1279), restated: quantise every coordinate,
// take the ranges and the smallest neighbour step, then walk the atoms -- a full-precision atom, the run of up to 8 "small" atoms
// that follows it (differences to the atom before, in `smallidx` bits), the swap of the first small atom with the full one, a flag
// where the run length or the small-number table changes -- and append bits to one stream.  Frames are independent records; inside
// a frame only that walk is serial (whether an atom starts a run, how long the run is and the +-1 step of `smallidx` depend on the
// group before).  So, as the decoder of xtc_gpu.h, the work is split -- count, scan, fill:
//
//   k_xtc_quantise  a thread per atom: the three integers with the reference's float32 operations (each rounded once, no fused
//                   multiply-add), the frame's min / max per axis and its smallest L1 neighbour step by integer atomics (the same
//                   bits every run), the refusal flag
//   k_xtc_plan      a lane per frame: the header values, then the walk over the integers through LDS windows the wave refills
//                   together; per GROUP one record {bit position, first atom, smallidx, run length, swap, flag value}; no payload bit
//   k_xtc_offsets   record sizes -> file offsets (one block)
//   k_xtc_clear     zeroes the image up to the last record's end
//   k_xtc_pack      a thread per group: the mixed-radix numbers (or three bit fields), flag bits and small triples, MSB-first into
//                   the image; interior words of a group's span by plain stores, its first and last word -- shared with the
//                   neighbours -- by a 32-bit atomic OR (OR commutes: the bytes do not depend on arrival order)
//   k_xtc_headers   a thread per frame: the record header, big-endian; frames of <= 9 atoms as plain floats
//
//   status  per frame: 0 ok; 2 outside what the device path takes, nothing of that frame is written: a full triple of more than 64
//           bits, a header smallidx + 8 > 64 (runs might be coded in more than 64 bits; the reference itself reads past its table
//           from 65 on), a smallest step beyond the table's last entry, a value that is not finite or whose quantum count leaves
//           the int range, a range of >= INT_MAX - 2, a frame of >= 2^21 atoms
#pragma once
#ifndef MK_DEVICE_API_PROVIDED
#include "mk_device.h"
#endif
#include "xtc_gpu.h"

#include <algorithm>

namespace mkamd {

// per frame, reduced by atomic MIN only (the buffer is filled with 0xff): values biased to unsigned order, the maxima inverted
struct XtcEncStats { unsigned w[8]; };   // lo[3], ~hi[3], smallest step, 0 = refused
struct XtcEncPlan {                      // 64 bytes
    int lo[3], hi[3];
    unsigned size[3];                    // hi - lo + 1
    int bitsize;                         // bits of a full triple's mixed-radix number; 0 = three bit fields (`fieldbits`)
    int fieldbits[3];
    int smallidx;                        // of the header
    int ngroups;
    unsigned nbits;                      // of the stream
};
static_assert(sizeof(XtcEncPlan) == 64 && sizeof(XtcEncStats) == 32, "layout shared with the host");
struct XtcEncGroup { unsigned pos, first, meta; };   // meta = smallidx | small atoms << 8 | swap << 12 | flag value (0xff = no flag) << 16

constexpr int XE_HEAD = 56, XE_HEAD2 = 36;           // bytes of a record's header; of a compressed record's second part
constexpr int XE_WIN_WORDS = 256;                    // words of a lane's window of its frame's integers
constexpr int XE_ATOMS = XE_WIN_WORDS / 3;           // whole atoms in it (85)
constexpr int XE_ROW = XE_WIN_WORDS + 1;             // its LDS row in words (odd: lanes at the same place of their rows hit 64 banks)
constexpr int XE_LW = XE_WIN_WORDS / WAVE;           // words of a row a lane loads in a refill
constexpr int XE_BATCH = 32 / XE_LW;                 // rows refilled per batch of loads in flight
constexpr int XE_REACH = 10;                         // atoms a group's step may read: the full one and up to 9 behind it
constexpr int XE_PAD = 4 * XE_WIN_WORDS;             // bytes behind the integers (a refill reads a whole window from the walk's atom)
static_assert(XE_WIN_WORDS % WAVE == 0 && XE_BATCH >= 1 && WAVE % XE_BATCH == 0 && XE_REACH < XE_ATOMS, "window: whole words per lane");

MK_DEV unsigned xe_bias(int v) { return (unsigned)v ^ 0x80000000u; }
MK_DEV int xe_unbias(unsigned u) { return (int)(u ^ 0x80000000u); }
MK_DEV unsigned xe_absdiff(int a, int b)             // |a - b| (the difference fits an int in every frame that is walked)
{
    const int t = (int)((unsigned)a - (unsigned)b);
    return t < 0 ? 0u - (unsigned)t : (unsigned)t;
}
MK_DEV int xe_bitlen(unsigned v) { int n = 0; while (v) { ++n; v >>= 1; } return n; }
MK_DEV int xe_bitlen64(unsigned long long v) { return (v >> 32) ? 32 + xe_bitlen((unsigned)(v >> 32)) : xe_bitlen((unsigned)v); }

// the reference's rounding (xdrfile.cpp:1053-1063), float32, each operation rounded once; `in_scale` is the host's nm conversion
MK_DEV int xtc_quantum(float x, float in_scale, float precision, bool& bad)
{
    const float v = mk_fmul_rn(x, in_scale);
    float lf = mk_fmul_rn(v, precision);
    lf = v >= 0.0f ? mk_fadd_rn(lf, 0.5f) : mk_fsub_rn(lf, 0.5f);
    const bool ok = mk_abs(lf) < 2147483648.0f;      // |lf| <= INT_MAX - 2 for a float; false for NaN
    bad = bad || !ok;
    return ok ? (int)lf : 0;
}

// ---- pass 1: the integers, their ranges, the smallest step ----
MK_KERNEL(256) void k_xtc_quantise(const float* __restrict__ xyz, float in_scale, const float* __restrict__ precision, long long frame0,
                                   long long natoms, int blocks_per_frame, int* __restrict__ ints, XtcEncStats* __restrict__ stats)
{
    __shared__ unsigned red[8];
    const long long f = frame0 + (long long)(blockIdx.x / (unsigned)blocks_per_frame);
    const long long a = (long long)(blockIdx.x % (unsigned)blocks_per_frame) * 256 + (long long)threadIdx.x;
    if (threadIdx.x < 8u) red[threadIdx.x] = 0xffffffffu;
    mk_block_sync();
    if (a < natoms) {
        float p = precision[f];
        if (p <= 0.0f) p = 1000.0f;
        const float* __restrict__ x = xyz + ((size_t)f * (size_t)natoms + (size_t)a) * 3;
        bool bad = false;
        int q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = xtc_quantum(x[k], in_scale, p, bad);
        int* __restrict__ o = ints + ((size_t)f * (size_t)natoms + (size_t)a) * 3;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) { mk_lds_min(&red[k], xe_bias(q[k])); mk_lds_min(&red[3 + k], ~xe_bias(q[k])); }
        if (a > 0) {                                 // (the first atom's step from the origin is left out: xdrfile.cpp:1099-1101)
            bool other = false;                      // (the atom before flags itself)
            unsigned d = 0u;
#pragma unroll
            for (int k = 0; k < 3; ++k) d += xe_absdiff(xtc_quantum(x[k - 3], in_scale, p, other), q[k]);
            mk_lds_min(&red[6], xe_bias((int)d));
        }
        if (bad) mk_lds_min(&red[7], 0u);
    }
    mk_block_sync();
    if (threadIdx.x < 8u && red[threadIdx.x] != 0xffffffffu) mk_atomic_min(&stats[f].w[threadIdx.x], red[threadIdx.x]);
}

// ---- pass 2: the header values and the walk ----
MK_KERNEL(64) void k_xtc_plan(const int* __restrict__ ints, const XtcEncStats* __restrict__ stats, long long nframes, long long natoms,
                              XtcEncPlan* __restrict__ plan, XtcEncGroup* __restrict__ groups, int* __restrict__ status)
{
    __shared__ unsigned win[WAVE * XE_ROW];
    const int lane = (int)(threadIdx.x & (WAVE - 1));
    const long long f = (long long)blockIdx.x * WAVE + lane;
    const bool mine = f < nframes;
    XtcEncPlan P = {};
    if (natoms <= 9) {                                               // plain floats: nothing to plan (the same for every lane)
        if (mine) { plan[f] = P; status[f] = 0; }
        return;
    }
    mk_setprio_high();
    int st = 0;
    int smallidx = XTC_FIRST;
    if (mine) {
        const XtcEncStats s = stats[f];
        bool refuse = s.w[7] == 0u;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            P.lo[k] = xe_unbias(s.w[k]);
            P.hi[k] = xe_unbias(~s.w[3 + k]);
            refuse = refuse || !(mk_fsub_rn((float)P.hi[k], (float)P.lo[k]) < 2147483648.0f);   // (float)max - (float)min >= INT_MAX - 2
            P.size[k] = (unsigned)P.hi[k] - (unsigned)P.lo[k] + 1u;
        }
        if (!refuse) {
            if ((P.size[0] | P.size[1] | P.size[2]) > 0xffffffu) {
                for (int k = 0; k < 3; ++k) P.fieldbits[k] = xe_bitlen(P.size[k]);
                P.bitsize = 0;
            } else {                                                 // bits of the product of three numbers below 2^24: up to 72
                const unsigned long long p01 = (unsigned long long)P.size[0] * P.size[1];
                const unsigned long long lo = (p01 & 0xffffffffull) * P.size[2], top = (p01 >> 32) * P.size[2] + (lo >> 32);
                P.bitsize = top ? 32 + xe_bitlen64(top) : xe_bitlen((unsigned)lo);
                refuse = P.bitsize > 64;
            }
            const int mindiff = xe_unbias(s.w[6]);
            while (smallidx < XTC_NMAGIC && XTC_MAGIC[smallidx] < mindiff) ++smallidx;
            P.smallidx = smallidx;
            refuse = refuse || smallidx + 8 > 64;                    // (and with it an index of 73, past the table)
        }
        if (refuse || natoms >= (1ll << 21)) st = 2;
    }
    bool live = mine && st == 0;
    if (!live) smallidx = XTC_FIRST;                                 // (a refused frame's index may lie past the table)
    const int N = (int)natoms;
    const int maxidx = smallidx + 8, minidx = smallidx;              // (smallidx + 8 <= 64 < the table's end)
    const int larger = XTC_MAGIC[maxidx] / 2;
    int smallnum = XTC_MAGIC[smallidx] / 2;
    int smaller = XTC_MAGIC[smallidx - 1 > XTC_FIRST ? smallidx - 1 : XTC_FIRST] / 2;
    const unsigned full_bits = P.bitsize ? (unsigned)P.bitsize : (unsigned)(P.fieldbits[0] + P.fieldbits[1] + P.fieldbits[2]);
    const int* __restrict__ base = ints + (live ? (size_t)f * (size_t)natoms * 3 : (size_t)0);
    XtcEncGroup* __restrict__ grp = groups + (size_t)(mine ? f : 0) * (size_t)natoms;
    int i = 0, g = 0, prevrun = -1;
    int prev[3] = {0, 0, 0};
    unsigned pos = 0u;
    while (mk_ballot(live) != 0ull) {
        // the wave refills every lane's window: row l <- XE_WIN_WORDS words of frame l's integers from the atom its walk is at
        const int wstart = i;
        const unsigned long long src = (unsigned long long)(uintptr_t)(base + 3 * (size_t)wstart);
        const unsigned src_lo = (unsigned)src, src_hi = (unsigned)(src >> 32);
        mk_block_sync();                                             // the rows are no longer being read
        for (int l0 = 0; l0 < WAVE; l0 += XE_BATCH) {
            unsigned v[XE_BATCH][XE_LW];
#pragma unroll
            for (int j = 0; j < XE_BATCH; ++j) {
                const unsigned long long a = (unsigned long long)mk_readlane(src_lo, l0 + j) | ((unsigned long long)mk_readlane(src_hi, l0 + j) << 32);
                const unsigned* __restrict__ p = reinterpret_cast<const unsigned*>((uintptr_t)a);
#pragma unroll
                for (int k = 0; k < XE_LW; ++k) v[j][k] = p[XE_LW * lane + k];
            }
#pragma unroll
            for (int j = 0; j < XE_BATCH; ++j)
#pragma unroll
                for (int k = 0; k < XE_LW; ++k) win[(l0 + j) * XE_ROW + XE_LW * lane + k] = v[j][k];
        }
        mk_block_sync();
        const unsigned* row = &win[lane * XE_ROW];
        auto at = [&](int a, int (&c)[3]) { const unsigned* p = row + 3 * (a - wstart); c[0] = (int)p[0]; c[1] = (int)p[1]; c[2] = (int)p[2]; };
        auto near = [&](const int (&a)[3], const int (&b)[3], int lim) {
            return xe_absdiff(a[0], b[0]) < (unsigned)lim && xe_absdiff(a[1], b[1]) < (unsigned)lim && xe_absdiff(a[2], b[2]) < (unsigned)lim;
        };
        // a group's step reads atoms i .. i + 9 (as far as the frame has them): taken while they are inside the window
        while (live && (i - wstart + XE_REACH <= XE_ATOMS || N - wstart <= XE_ATOMS)) {
            int cur[3];
            at(i, cur);
            int is_smaller = 0;
            if (smallidx < maxidx && i >= 1 && near(cur, prev, larger)) is_smaller = 1;
            else if (smallidx > minidx) is_smaller = -1;
            bool is_small = false;
            int first_small[3] = {0, 0, 0};
            if (i + 1 < N) {
                int nx[3];
                at(i + 1, nx);
                if (near(cur, nx, smallnum)) {                       // the swap: the second atom goes out in full, the first as a small one
                    first_small[0] = cur[0]; first_small[1] = cur[1]; first_small[2] = cur[2];
                    cur[0] = nx[0]; cur[1] = nx[1]; cur[2] = nx[2];
                    is_small = true;
                }
            }
            prev[0] = cur[0]; prev[1] = cur[1]; prev[2] = cur[2];
            const int first = i;
            const bool swap = is_small;
            ++i;
            if (!is_small && is_smaller == -1) is_smaller = 0;
            int nsmall = 0;
            while (is_small && nsmall < 8) {
                int t[3];
                if (nsmall == 0) { t[0] = first_small[0]; t[1] = first_small[1]; t[2] = first_small[2]; }
                else at(i, t);
                // (the reference's int arithmetic, which wraps at the table's upper end: squares of up to 2^21 quanta)
                unsigned sum = 0u;
#pragma unroll
                for (int k = 0; k < 3; ++k) { const unsigned d = (unsigned)t[k] - (unsigned)prev[k]; sum += d * d; }
                if (is_smaller == -1 && (int)sum >= (int)((unsigned)smaller * (unsigned)smaller)) is_smaller = 0;
                ++nsmall;
                prev[0] = t[0]; prev[1] = t[1]; prev[2] = t[2];
                ++i;
                is_small = false;
                if (i < N) {
                    int n2[3];
                    at(i, n2);
                    is_small = near(n2, prev, smallnum);
                }
            }
            const int run = 3 * nsmall;
            const bool flag = run != prevrun || is_smaller != 0;
            if (flag) prevrun = run;
            grp[g] = XtcEncGroup{pos, (unsigned)first,
                                 (unsigned)smallidx | ((unsigned)nsmall << 8) | ((swap ? 1u : 0u) << 12) | ((flag ? (unsigned)(run + is_smaller + 1) : 0xffu) << 16)};
            ++g;                                                     // (g <= first < natoms)
            pos += full_bits + (flag ? 6u : 1u) + (unsigned)(nsmall * smallidx);
            if (is_smaller != 0) {
                smallidx += is_smaller;
                if (is_smaller < 0) { smallnum = smaller; smaller = XTC_MAGIC[smallidx - 1] / 2; }
                else { smaller = smallnum; smallnum = XTC_MAGIC[smallidx] / 2; }
            }
            live = i < N;
        }
        // a lane that is done keeps taking part in the refills, from the start of the buffer (nothing is read beyond XE_PAD)
        if (!live) { i = 0; base = ints; }
    }
    if (mine) {
        P.ngroups = st ? 0 : g;
        P.nbits = st ? 0u : pos;
        plan[f] = P;
        status[f] = st;
    }
}

// bytes of frame f's record in the image (0: refused)
MK_DEV unsigned long long xtc_record_bytes(const XtcEncPlan& p, int st, long long natoms)
{
    if (st) return 0ull;
    if (natoms <= 9) return (unsigned long long)XE_HEAD + 12ull * (unsigned long long)natoms;
    const unsigned long long nbytes = ((unsigned long long)p.nbits + 7ull) >> 3;
    return (unsigned long long)(XE_HEAD + XE_HEAD2) + ((nbytes + 3ull) & ~3ull);
}

// ---- the scan: record sizes -> offsets [nframes + 1] (one block; refuse_all: frames of >= 2^21 atoms, nothing else ran) ----
MK_KERNEL(256) void k_xtc_offsets(const XtcEncPlan* __restrict__ plan, int* __restrict__ status, long long nframes, long long natoms, int refuse_all,
                                  unsigned long long* __restrict__ offsets)
{
    __shared__ unsigned long long part[256];
    const int t = (int)threadIdx.x;
    const long long per = (nframes + 255) / 256, lo = (long long)t * per, hi = lo + per < nframes ? lo + per : nframes;
    unsigned long long sum = 0ull;
    for (long long f = lo; f < hi; ++f) {
        if (refuse_all) status[f] = 2;
        else sum += xtc_record_bytes(plan[f], status[f], natoms);
    }
    part[t] = sum;
    mk_block_sync();
    if (t == 0) {
        unsigned long long run = 0ull;
        for (int k = 0; k < 256; ++k) { const unsigned long long s = part[k]; part[k] = run; run += s; }
        offsets[nframes] = run;
    }
    mk_block_sync();
    unsigned long long run = part[t];
    for (long long f = lo; f < hi; ++f) {
        offsets[f] = run;
        if (!refuse_all) run += xtc_record_bytes(plan[f], status[f], natoms);
    }
}

MK_KERNEL(256) void k_xtc_clear(unsigned* __restrict__ image, const unsigned long long* __restrict__ offsets, long long nframes)
{
    const unsigned long long words = offsets[nframes] >> 2, stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long w = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; w < words; w += stride) image[w] = 0u;
}

// ---- pass 3: the bits ----
struct XtcBitWriter {                    // MSB-first over 32-bit big-endian words of a zeroed image, from any bit position
    unsigned* wp;
    unsigned long long acc;              // the last `nacc` bits taken (right-aligned)
    int nacc;
    bool first;                          // no word has gone out yet: the next one is shared with the group before
    MK_DEVFN void start(unsigned char* base, unsigned bitpos)
    {
        wp = reinterpret_cast<unsigned*>(base) + (bitpos >> 5);
        acc = 0ull;
        nacc = (int)(bitpos & 31u);      // (zeros in the neighbour's bits: an OR leaves them alone)
        first = true;
    }
    MK_DEVFN void put(int n, unsigned v)  // 0 <= n <= 32, v < 2^n
    {
        acc = (acc << n) | (unsigned long long)v;
        nacc += n;
        if (nacc >= 32) {
            const unsigned w = __builtin_bswap32((unsigned)(acc >> (nacc - 32)));
            if (first) mk_atomic_or(reinterpret_cast<int*>(wp), (int)w);
            else *wp = w;
            first = false;
            ++wp;
            nacc -= 32;
        }
    }
    MK_DEVFN void finish()                // the last, partial word: shared with the group behind
    {
        if (nacc > 0) mk_atomic_or(reinterpret_cast<int*>(wp), (int)__builtin_bswap32((unsigned)(acc << (32 - nacc))));
    }
};

// a number of nbits (<= 64) bits: least-significant byte first, the top nbits - 8 * ((nbits - 1) / 8) bits last (encodeints)
MK_DEV void xtc_put_number(XtcBitWriter& b, int nbits, unsigned long long x)
{
    int nfull = (nbits - 1) >> 3;
    const int top = nbits - 8 * nfull;
    while (nfull >= 4) { b.put(32, __builtin_bswap32((unsigned)x)); x >>= 32; nfull -= 4; }
    if (nfull) { b.put(8 * nfull, __builtin_bswap32((unsigned)x) >> (32 - 8 * nfull)); x >>= 8 * nfull; }
    b.put(top, (unsigned)x);
}

MK_KERNEL(256) void k_xtc_pack(const int* __restrict__ ints, const XtcEncPlan* __restrict__ plan, const XtcEncGroup* __restrict__ groups,
                               const int* __restrict__ status, const unsigned long long* __restrict__ offsets, long long frame0, long long natoms,
                               int blocks_per_frame, unsigned char* __restrict__ image)
{
    const long long f = frame0 + (long long)(blockIdx.x / (unsigned)blocks_per_frame);
    const int g = (int)(blockIdx.x % (unsigned)blocks_per_frame) * 256 + (int)threadIdx.x;
    if (status[f] != 0 || g >= plan[f].ngroups) return;
    const XtcEncPlan& P = plan[f];
    const XtcEncGroup rec = groups[(size_t)f * (size_t)natoms + (size_t)g];
    const int sidx = (int)(rec.meta & 0xffu), nsmall = (int)((rec.meta >> 8) & 15u);
    const bool swap = ((rec.meta >> 12) & 1u) != 0u;
    const unsigned flagval = (rec.meta >> 16) & 0xffu;
    const int* __restrict__ c = ints + ((size_t)f * (size_t)natoms + (size_t)rec.first) * 3;
    XtcBitWriter b;
    b.start(image + offsets[f] + (XE_HEAD + XE_HEAD2), rec.pos);
    const int* full = swap ? c + 3 : c;
    const unsigned t0 = (unsigned)full[0] - (unsigned)P.lo[0], t1 = (unsigned)full[1] - (unsigned)P.lo[1], t2 = (unsigned)full[2] - (unsigned)P.lo[2];
    if (P.bitsize == 0) { b.put(P.fieldbits[0], t0); b.put(P.fieldbits[1], t1); b.put(P.fieldbits[2], t2); }
    else xtc_put_number(b, P.bitsize, ((unsigned long long)t0 * P.size[1] + t1) * P.size[2] + t2);
    if (flagval == 0xffu) b.put(1, 0u);
    else { b.put(1, 1u); b.put(5, flagval); }
    const unsigned radix = (unsigned)XTC_MAGIC[sidx], smallnum = radix / 2u;
    int prev[3] = {full[0], full[1], full[2]};
    for (int k = 0; k < nsmall; ++k) {
        const int* t = k == 0 ? c : c + 3 * (k + 1);                  // (the first small atom is the group's first atom: the swap)
        const unsigned d0 = (unsigned)t[0] - (unsigned)prev[0] + smallnum, d1 = (unsigned)t[1] - (unsigned)prev[1] + smallnum,
                       d2 = (unsigned)t[2] - (unsigned)prev[2] + smallnum;
        xtc_put_number(b, sidx, ((unsigned long long)d0 * radix + d1) * radix + d2);
        prev[0] = t[0]; prev[1] = t[1]; prev[2] = t[2];
    }
    b.finish();
}

MK_KERNEL(256) void k_xtc_headers(const float* __restrict__ xyz, float in_scale, const float* __restrict__ precision, const float* __restrict__ box,
                                  const float* __restrict__ time, const int* __restrict__ step, const XtcEncPlan* __restrict__ plan,
                                  const int* __restrict__ status, const unsigned long long* __restrict__ offsets, long long nframes, long long natoms,
                                  unsigned char* __restrict__ image)
{
    const long long f = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (f >= nframes || status[f] != 0) return;
    unsigned* __restrict__ w = reinterpret_cast<unsigned*>(image + offsets[f]);
    auto be = [](unsigned v) { return __builtin_bswap32(v); };
    w[0] = be(1995u); w[1] = be((unsigned)natoms); w[2] = be((unsigned)step[f]); w[3] = be(mk_float_bits(time[f]));
    for (int k = 0; k < 9; ++k) w[4 + k] = be(mk_float_bits(box[(size_t)f * 9 + k]));
    w[13] = be((unsigned)natoms);
    if (natoms <= 9) {
        const float* __restrict__ x = xyz + (size_t)f * (size_t)natoms * 3;
        for (int k = 0; k < (int)natoms * 3; ++k) w[14 + k] = be(mk_float_bits(mk_fmul_rn(x[k], in_scale)));
        return;
    }
    const XtcEncPlan& P = plan[f];
    float p = precision[f];
    if (p <= 0.0f) p = 1000.0f;
    w[14] = be(mk_float_bits(p));
    for (int k = 0; k < 3; ++k) { w[15 + k] = be((unsigned)P.lo[k]); w[18 + k] = be((unsigned)P.hi[k]); }
    w[21] = be((unsigned)P.smallidx);
    w[22] = be((P.nbits + 7u) >> 3);
}

// ---- the call: sizes, work-buffer layout, launches (a backend gives `launch` and `fill`: capi.hip's stream, or the host emulation) ----
inline unsigned long long xtc_encode_bound(long long n_frames, long long n_atoms)
{
    if (n_frames <= 0 || n_atoms < 0) return 0ull;
    // a full atom costs at most 3 x 31 field bits (or a 64-bit number) and 6 flag bits, a small one at most 64: 13 bytes an atom
    const unsigned long long per = n_atoms <= 9 ? (unsigned long long)XE_HEAD + 12ull * (unsigned long long)n_atoms
                                                : (((unsigned long long)(XE_HEAD + XE_HEAD2) + 13ull * (unsigned long long)n_atoms + 3ull) & ~3ull);
    return (unsigned long long)n_frames * per;
}

struct XtcEncodeLayout { unsigned long long ints, stats, plan, groups, total; };
inline XtcEncodeLayout xtc_encode_layout(long long n_frames, long long n_atoms)
{
    XtcEncodeLayout L = {};
    if (n_frames <= 0 || n_atoms < 0) return L;
    auto up = [](unsigned long long v) { return (v + 255ull) & ~255ull; };
    const bool walked = n_atoms > 9 && n_atoms < (1ll << 21);
    const unsigned long long F = (unsigned long long)n_frames, N = (unsigned long long)n_atoms;
    L.ints = 0ull;
    L.stats = walked ? up(F * N * 12ull + (unsigned long long)XE_PAD) : 0ull;
    L.plan = L.stats + (walked ? up(F * sizeof(XtcEncStats)) : 0ull);
    L.groups = L.plan + up(F * sizeof(XtcEncPlan));
    L.total = L.groups + (walked ? up(F * N * sizeof(XtcEncGroup)) : 0ull);
    return L;
}

struct XtcEncodeArgs {
    const float* xyz; float in_scale; const float* precision; const float* box; const float* time; const int* step;
    long long n_frames, n_atoms;
    unsigned char* image; unsigned long long* offsets; int* status; unsigned char* work;
};

template <class Backend>
int run_xtc_encode(Backend& be, const XtcEncodeArgs& a)
{
    const long long F = a.n_frames, N = a.n_atoms;
    const XtcEncodeLayout L = xtc_encode_layout(F, N);
    int* ints = reinterpret_cast<int*>(a.work + L.ints);
    XtcEncStats* stats = reinterpret_cast<XtcEncStats*>(a.work + L.stats);
    XtcEncPlan* plan = reinterpret_cast<XtcEncPlan*>(a.work + L.plan);
    XtcEncGroup* groups = reinterpret_cast<XtcEncGroup*>(a.work + L.groups);
    int st;
    if (N >= (1ll << 21)) return be.launch(k_xtc_offsets, dim3(1), dim3(256), (const XtcEncPlan*)plan, a.status, F, N, 1, a.offsets);
    const long long bpf = (N + 255) / 256;
    const long long per_launch = bpf ? std::max<long long>(1, 0x7fffffffll / bpf) : F;
    if (N > 9) {
        if ((st = be.fill(stats, 0xff, (size_t)F * sizeof(XtcEncStats)))) return st;
        for (long long f0 = 0; f0 < F; f0 += per_launch) {
            const long long nf = std::min(per_launch, F - f0);
            if ((st = be.launch(k_xtc_quantise, dim3((unsigned)(nf * bpf)), dim3(256), a.xyz, a.in_scale, a.precision, f0, N, (int)bpf, ints, stats))) return st;
        }
    }
    if ((st = be.launch(k_xtc_plan, dim3((unsigned)((F + 63) / 64)), dim3(64), (const int*)ints, (const XtcEncStats*)stats, F, N, plan, groups, a.status))) return st;
    if ((st = be.launch(k_xtc_offsets, dim3(1), dim3(256), (const XtcEncPlan*)plan, a.status, F, N, 0, a.offsets))) return st;
    const unsigned long long bound_words = xtc_encode_bound(F, N) / 4ull;
    const unsigned clear_blocks = (unsigned)std::min<unsigned long long>(1024ull, (bound_words + 255ull) / 256ull);
    if ((st = be.launch(k_xtc_clear, dim3(clear_blocks), dim3(256), reinterpret_cast<unsigned*>(a.image), (const unsigned long long*)a.offsets, F))) return st;
    if (N > 9)
        for (long long f0 = 0; f0 < F; f0 += per_launch) {
            const long long nf = std::min(per_launch, F - f0);
            if ((st = be.launch(k_xtc_pack, dim3((unsigned)(nf * bpf)), dim3(256), (const int*)ints, (const XtcEncPlan*)plan, (const XtcEncGroup*)groups,
                                (const int*)a.status, (const unsigned long long*)a.offsets, f0, N, (int)bpf, a.image))) return st;
        }
    return be.launch(k_xtc_headers, dim3((unsigned)((F + 255) / 256)), dim3(256), a.xyz, a.in_scale, a.precision, a.box, a.time, a.step,
                     (const XtcEncPlan*)plan, (const int*)a.status, (const unsigned long long*)a.offsets, F, N, a.image);
}

}  // namespace mkamd
