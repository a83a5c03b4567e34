// xtc_headers.h -- host half of the device XTC decoder: the record headers of a selection of frames -> XtcFrameDesc (xtc_gpu.h).
// No HIP in here (capi.hip's mkamd_xtc_chunk_desc / mkamd_xtc_chunk_desc_mem call it; so does the sanitized CPU-tier driver
// tests/emu/xtc_damage_main.cpp, on damaged files).
#pragma once
#include "xtc_gpu.h"
#include "xtc_reader.h"

namespace mkamd {

// The record headers of the selected frames, read from `base` (= the file's bytes from offset base_off up to limit): descriptors for the
// device decoder (data offsets relative to the lowest selected record), boxes, times, steps, the byte range [lo, hi) of the selection.
// `fail(message)` records the message and returns the caller's error status (capi.hip: its last-error text and MKAMD_EINVAL); 0 = ok.
// The device's byte buffer is [lo, hi) + XTC_PAD bytes: `hi` rounds the last stream up to a whole word but never passes the file's end
// (a stream may end the file unpadded), and every stream lies inside the file -- nbytes is checked against its size --, so the walk's
// total_bits (nbytes * 8) ends inside [lo, hi) and only its windows' read-ahead reaches into the pad.
template <class Fail>
inline int xtc_parse_headers(const uint8_t* base, size_t base_off, size_t limit, size_t file_size, const mkamd::xtc::FrameIndex& idx,
                             const int64_t* frames, int64_t n_sel, int64_t n_atoms, void* desc_out, int64_t* byte_lo, int64_t* byte_hi,
                             float* box, float* time, int32_t* step, Fail&& fail)
{
    using namespace mkamd::xtc;
    mkamd::XtcFrameDesc* D = (mkamd::XtcFrameDesc*)desc_out;
    size_t lo = (size_t)-1, hi = 0;
    std::vector<size_t> rec((size_t)n_sel), end((size_t)n_sel);
    for (int64_t j = 0; j < n_sel; ++j) {
        const int64_t f = frames ? frames[j] : j;
        if (f < 0 || f >= (int64_t)idx.offs.size()) return fail("frame index out of range");
        const size_t r = idx.offs[(size_t)f];
        // the record's fixed header is 56 bytes; a compressed one (> 9 atoms) has 36 more before its stream, a raw one (1-9 atoms:
        // 56 + 12 n bytes in all) may end before byte 92
        if (r < base_off || r + 56 > limit || (n_atoms > 9 && r + 92 > limit)) return fail("frame outside the bytes handed over");
        const uint8_t* q = base + (r - base_off);
        if (be_i32(q) != FRAME_MAGIC || (int64_t)be_i32(q + 4) != n_atoms || (int64_t)be_i32(q + 52) != n_atoms) return fail("corrupt XTC frame");
        step[j] = be_i32(q + 8);
        time[j] = be_f32(q + 12);
        for (int i = 0; i < 9; ++i) box[(size_t)i * (size_t)n_sel + (size_t)j] = be_f32(q + 16 + 4 * i);
        mkamd::XtcFrameDesc d{};
        size_t data = r + 56, e;
        if (n_atoms <= 9) {
            d.raw = 1; d.nbytes = (unsigned)(12 * n_atoms);
            e = data + (size_t)12 * (size_t)n_atoms;
        } else {
            const uint8_t* h = base + (data - base_off);
            const float precision = be_f32(h);
            int32_t hi3[3];
            for (int k = 0; k < 3; ++k) { d.lo[k] = be_i32(h + 4 + 4 * k); hi3[k] = be_i32(h + 16 + 4 * k); }
            d.smallidx = be_i32(h + 28);
            const int32_t nbytes = be_i32(h + 32);
            data += 36;
            if (nbytes < 0 || data + (size_t)nbytes > file_size) return fail("corrupt XTC frame");
            d.nbytes = (unsigned)nbytes;
            for (int k = 0; k < 3; ++k) d.range[k] = (uint32_t)hi3[k] - (uint32_t)d.lo[k] + 1u;
            if (!d.range[0] || !d.range[1] || !d.range[2]) return fail("corrupt XTC frame");
            if ((d.range[0] | d.range[1] | d.range[2]) > 0xffffffu) { d.triple_bits = 0; for (int k = 0; k < 3; ++k) d.field_bits[k] = bits_for(d.range[k]); }
            else d.triple_bits = bits_for_product(d.range);
            d.inv_precision = (float)(1.0 / (double)precision);            // as decode_frame
            e = data + (((size_t)nbytes + 3) / 4) * 4;
        }
        rec[(size_t)j] = data; end[(size_t)j] = e;
        lo = std::min(lo, r); hi = std::max(hi, e);
        D[j] = d;
    }
    if (hi > file_size) hi = file_size;
    for (int64_t j = 0; j < n_sel; ++j) D[j].data_off = (unsigned long long)(rec[(size_t)j] - lo);
    *byte_lo = (int64_t)lo; *byte_hi = (int64_t)hi;
    return 0;
}

}  // namespace mkamd
