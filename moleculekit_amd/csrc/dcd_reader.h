// dcd_reader.h -- host side of the DCD trajectory path (CHARMM / NAMD / X-PLOR / OpenMM files): header parser, frame count, frame
// descriptors for the device decoder (csrc/dcd_kernels.h), a plain host read loop, and the writer's 276-byte file header.
//
// Restates, for reading, what moleculekit/fileformats/dcd does (src/dcdplugin.c: read_dcdheader, read_dcdstep, skip_dcdstep,
// open_dcd_read, read_next_timestep; dcd.pyx: DCDTrajectoryFile.read): the same float32 bits out.  The format, in Fortran records
// (a marker word before and after each record, 4 or 8 bytes, the byte count of the record):
//
//   file   := [84: "CORD" NSET ISTART NSAVC 5x0 NAMNF DELTA(f32; X-PLOR: f64) extra? four? ... version] [title: NTITLE 80*NTITLE]
//             [4: N] [4*(N-NAMNF): free atoms, 1-based]?   frame*
//   frame  := [48: six doubles A cosAB B cosAC cosBC C]?  [x plane] [y plane] [z plane] [4th plane]?
//   a plane holds N floats in the first frame and N - NAMNF (the free atoms) in every later one.
//
// So a frame lies at an offset the header fixes, and reading it is a byte swap, a gather and a 12-byte store per atom.  Own structure:
// the file is mapped (or a caller's buffer viewed), every read goes through a bounds-checked cursor, and everything a descriptor
// points to is checked against the file's size before it is handed out.  No HIP in here.
//
// Departures from the reference, all of them refusals with a message:
//   * an opposite-endian file with the 4th-dimension flag: the reference tests the flag before swapping it, takes the file for 3-D and
//     returns a wrong frame count with garbage frames or a format error behind the first frame;
//   * X-PLOR headers with 8-byte markers (the reference reads their frames with 4-byte markers);
//   * N <= 0, NAMNF outside [0, N), free indices outside 1..N or not strictly ascending, an extra block that is not 48 bytes, a plane
//     marker that disagrees with N -- where the reference reads or writes outside its buffers or returns an error code per frame.
// The frame count uses the frames' true sizes; the reference's recount assumes 4-byte markers also in files with 8-byte ones.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "xtc_reader.h"   // mkamd::xtc::Mapped: the mapped file / a view of caller memory

namespace mkamd {
namespace dcd {

enum Flags : int32_t { F_SWAP = 1, F_REC64 = 2, F_CHARMM = 4, F_EXTRA = 8, F_4DIMS = 16 };

// one selected frame for the device decoder: byte offsets of its planes inside the uploaded range, floats per plane, flags
struct FrameDesc {
    uint64_t x_off, y_off, z_off;
    uint32_t count;
    uint32_t flags;
};
static_assert(sizeof(FrameDesc) == 32, "the Python side sizes its buffers by this");
constexpr uint32_t D_SWAP = 1u, D_FREE_ONLY = 2u;

struct Header {
    int64_t n_atoms = 0, n_frames = 0;
    int32_t nset = 0, istart = 0, nsavc = 0, nfixed = 0, flags = 0;
    double delta = 0.0;
    size_t first_off = 0, first_size = 0, frame_size = 0, marker = 4, extra_size = 0;
    std::vector<int32_t> free_idx;                 // 1-based indices of the free atoms (NAMNF > 0 only)
    bool swap() const { return flags & F_SWAP; }
    int64_t n_free() const { return n_atoms - nfixed; }
    size_t frame_off(int64_t f) const { return f == 0 ? first_off : first_off + first_size + (size_t)(f - 1) * frame_size; }
    size_t frame_end(int64_t f) const { return frame_off(f) + (f == 0 ? first_size : frame_size); }
    int64_t plane_count(int64_t f) const { return f == 0 ? n_atoms : n_free(); }
};

inline uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// bounds-checked reads out of the file's bytes
struct Cursor {
    const uint8_t* p;
    size_t n, pos = 0;
    bool swap = false, rec64 = false;
    bool has(size_t bytes) const { return pos <= n && bytes <= n - pos; }
    bool raw32(uint32_t& v)
    {
        if (!has(4)) return false;
        std::memcpy(&v, p + pos, 4);
        pos += 4;
        return true;
    }
    bool u32(uint32_t& v)
    {
        if (!raw32(v)) return false;
        if (swap) v = bswap32(v);
        return true;
    }
    // a record marker: one word, or two whose sum is the value (the upper word of a 64-bit marker is zero in either byte order)
    bool marker(uint32_t& v)
    {
        uint32_t a = 0, b = 0;
        if (!u32(a)) return false;
        if (rec64 && !u32(b)) return false;
        v = a + b;
        return true;
    }
    bool skip(size_t bytes)
    {
        if (!has(bytes)) return false;
        pos += bytes;
        return true;
    }
};

inline uint32_t word_at(const uint8_t* q, bool swap)
{
    uint32_t v;
    std::memcpy(&v, q, 4);
    return swap ? bswap32(v) : v;
}

inline int fail(std::string& err, const char* msg)
{
    err = msg;
    return 1;
}

// The header of the file whose bytes are p[0, n): 0, or 1 with a message.
inline int parse_header(const uint8_t* p, size_t n, Header& h, std::string& err)
{
    constexpr uint32_t CORD = 0x44524f43u;         // "CORD" read as a little-endian word
    Cursor c{p, n};
    uint32_t w0 = 0, w1 = 0;
    if (!c.raw32(w0) || !c.raw32(w1)) return fail(err, "not a DCD file: shorter than its first record marker");
    if (w0 + w1 == 84u) c.rec64 = true;
    else if (w0 == 84u && w1 == CORD) {}
    else if (bswap32(w0) + bswap32(w1) == 84u) { c.swap = true; c.rec64 = true; }
    else if (bswap32(w0) == 84u && w1 == CORD) c.swap = true;
    else return fail(err, "not a DCD file: the first record is not 84 bytes of CORD in either byte order");
    if (c.rec64) {
        uint32_t magic = 0;
        if (!c.raw32(magic) || magic != CORD) return fail(err, "not a DCD file: no CORD behind a 64-bit record marker");
    }
    if (!c.has(80)) return fail(err, "DCD header is cut off inside its first record");
    const uint8_t* hdr = p + c.pos;
    c.pos += 80;
    h.flags = (c.swap ? F_SWAP : 0) | (c.rec64 ? F_REC64 : 0);
    if (word_at(hdr + 76, false) != 0) {           // the CHARMM version: nonzero in either byte order
        h.flags |= F_CHARMM;
        if (word_at(hdr + 40, false) != 0) h.flags |= F_EXTRA;
        if (word_at(hdr + 44, c.swap) == 1u) h.flags |= F_4DIMS;
    }
    if ((h.flags & F_4DIMS) && c.swap)
        return fail(err, "opposite-endian DCD file with a 4th dimension: refused (the reference reader tests the 4th-dimension flag before "
                         "swapping it and misreads such a file as 3-D)");
    if (!(h.flags & F_CHARMM) && c.rec64) return fail(err, "X-PLOR DCD header with 64-bit record markers: refused");
    h.nset = (int32_t)word_at(hdr, c.swap);
    h.istart = (int32_t)word_at(hdr + 4, c.swap);
    h.nsavc = (int32_t)word_at(hdr + 8, c.swap);
    h.nfixed = (int32_t)word_at(hdr + 32, c.swap);
    if (h.flags & F_CHARMM) {
        const uint32_t u = word_at(hdr + 36, c.swap);
        float f;
        std::memcpy(&f, &u, 4);
        h.delta = (double)f;
    } else {
        uint64_t u;
        std::memcpy(&u, hdr + 36, 8);
        if (c.swap) u = __builtin_bswap64(u);
        std::memcpy(&h.delta, &u, 8);
    }
    uint32_t m = 0;
    if (!c.marker(m)) return fail(err, "DCD header is cut off behind its first record");
    if (m != 84u) return fail(err, "DCD header: the first record does not close with 84");
    if (!c.marker(m)) return fail(err, "DCD header is cut off before the title block");
    if ((m - 4u) % 80u != 0u) return fail(err, "DCD header: the title block is not 4 + 80 * NTITLE bytes");
    uint32_t nt = 0;
    if (!c.u32(nt)) return fail(err, "DCD header is cut off inside the title block");
    int32_t ntitle = (int32_t)nt;
    if (ntitle < 0) return fail(err, "DCD header: negative NTITLE");
    if (ntitle > 1000) ntitle = ntitle == 1095062083 ? 2 : 0;     // (a known broken writer put "CORD"-like text there: two lines)
    if (!c.skip((size_t)80 * (size_t)ntitle)) return fail(err, "DCD header is cut off inside the titles");
    if (!c.marker(m)) return fail(err, "DCD header is cut off behind the titles");
    if (!c.marker(m)) return fail(err, "DCD header is cut off before the atom count");
    if (m != 4u) return fail(err, "DCD header: the atom-count record is not 4 bytes");
    uint32_t na = 0;
    if (!c.u32(na)) return fail(err, "DCD header is cut off inside the atom count");
    if (!c.marker(m)) return fail(err, "DCD header is cut off behind the atom count");
    if (m != 4u) return fail(err, "DCD header: the atom-count record does not close with 4");
    h.n_atoms = (int32_t)na;
    if (h.n_atoms <= 0) return fail(err, "DCD header: atom count N <= 0");
    if (h.nfixed < 0 || h.nfixed >= h.n_atoms) return fail(err, "DCD header: number of fixed atoms outside [0, N)");
    h.free_idx.clear();
    if (h.nfixed != 0) {
        const uint32_t nfree = (uint32_t)(h.n_atoms - h.nfixed);
        if (!c.marker(m)) return fail(err, "DCD header is cut off before the free-atom indices");
        if (m != nfree * 4u) return fail(err, "DCD header: the free-atom record's marker disagrees with N - NAMNF");
        if (!c.has((size_t)nfree * 4)) return fail(err, "DCD header is cut off inside the free-atom indices");
        h.free_idx.resize(nfree);
        int64_t prev = 0;
        for (uint32_t i = 0; i < nfree; ++i) {
            uint32_t v = 0;
            c.u32(v);
            const int32_t idx = (int32_t)v;
            if (idx < 1 || idx > h.n_atoms) return fail(err, "DCD header: a free-atom index lies outside 1..N");
            if (idx <= prev) return fail(err, "DCD header: the free-atom indices are not strictly ascending");
            prev = idx;
            h.free_idx[i] = idx;
        }
        if (!c.marker(m)) return fail(err, "DCD header is cut off behind the free-atom indices");
        if (m != nfree * 4u) return fail(err, "DCD header: the free-atom record does not close with its size");
    }
    // the frame count from the file's size
    h.first_off = c.pos;
    h.marker = c.rec64 ? 8 : 4;
    h.extra_size = (h.flags & F_EXTRA) ? 48 + 2 * h.marker : 0;
    const size_t ndims = (h.flags & F_4DIMS) ? 4 : 3;
    h.first_size = ((size_t)h.n_atoms * 4 + 2 * h.marker) * ndims + h.extra_size;
    h.frame_size = ((size_t)h.n_free() * 4 + 2 * h.marker) * ndims + h.extra_size;
    if (n - h.first_off < h.first_size) return fail(err, "DCD file holds no complete frame");
    h.n_frames = (int64_t)((n - h.first_off - h.first_size) / h.frame_size) + 1;
    return 0;
}

inline int open_header(const char* path, xtc::Mapped& m, Header& h, std::string& err)
{
    if (!m.open_file(path) || (m.n && !m.p)) {
        err = std::string("cannot open ") + path;
        return 1;
    }
    return parse_header(m.p, m.n, h, err);
}

// Frame f of the file p[0, n): its markers checked, its plane offsets (absolute) and its unit cell as the reference hands it on:
// cell[0..2] = A, B, C; cell[3..5] = alpha, beta, gamma in degrees, from cosines when all three stored values lie in [-1, 1].
inline int locate_frame(const uint8_t* p, size_t n, const Header& h, int64_t f, size_t off[3], float cell[6], std::string& err)
{
    if (f < 0 || f >= h.n_frames) return fail(err, "frame index out of range");
    size_t pos = h.frame_off(f);
    if (h.frame_end(f) > n || h.frame_end(f) < pos) return fail(err, "DCD frame lies outside the file");
    const bool sw = h.swap();
    auto marker = [&](size_t at) { return word_at(p + at, sw) + (h.marker == 8 ? word_at(p + at + 4, sw) : 0u); };
    float uc[6] = {0.f, 90.f, 0.f, 90.f, 90.f, 0.f};
    if (h.flags & F_EXTRA) {
        if (marker(pos) != 48u) return fail(err, "DCD frame: the unit-cell record is not 48 bytes");
        for (int i = 0; i < 6; ++i) {
            uint64_t u;
            std::memcpy(&u, p + pos + h.marker + 8 * (size_t)i, 8);
            if (sw) u = __builtin_bswap64(u);
            double d;
            std::memcpy(&d, &u, 8);
            uc[i] = (float)d;
        }
        pos += h.extra_size;
    }
    const size_t plane = (size_t)h.plane_count(f) * 4;
    for (int k = 0; k < 3; ++k) {
        if (marker(pos) != (uint32_t)plane || marker(pos + h.marker + plane) != (uint32_t)plane)
            return fail(err, "DCD frame: a coordinate record's marker disagrees with the atom count");
        off[k] = pos + h.marker;
        pos += plane + 2 * h.marker;
    }
    cell[0] = uc[0]; cell[1] = uc[2]; cell[2] = uc[5];
    if (uc[1] >= -1.0 && uc[1] <= 1.0 && uc[3] >= -1.0 && uc[3] <= 1.0 && uc[4] >= -1.0 && uc[4] <= 1.0) {
        cell[3] = (float)(90.0 - std::asin((double)uc[4]) * 90.0 / M_PI_2);
        cell[4] = (float)(90.0 - std::asin((double)uc[3]) * 90.0 / M_PI_2);
        cell[5] = (float)(90.0 - std::asin((double)uc[1]) * 90.0 / M_PI_2);
    } else {
        cell[3] = uc[4]; cell[4] = uc[3]; cell[5] = uc[1];
    }
    return 0;
}

// Descriptors of the selected frames (any order, repeats allowed; NULL = 0 .. n_sel-1), the byte range [lo, hi) that holds them
// (offsets in the descriptors count from lo) and their unit cells [n_sel, 6].
inline int chunk_desc(const uint8_t* p, size_t n, const Header& h, const int64_t* frames, int64_t n_sel, FrameDesc* desc, int64_t* byte_lo,
                      int64_t* byte_hi, float* cell, std::string& err)
{
    size_t lo = (size_t)-1, hi = 0;
    for (int64_t j = 0; j < n_sel; ++j) {
        const int64_t f = frames ? frames[j] : j;
        if (f < 0 || f >= h.n_frames) return fail(err, "frame index out of range");
        lo = std::min(lo, h.frame_off(f));
        hi = std::max(hi, h.frame_end(f));
    }
    if (hi > n) return fail(err, "DCD frame lies outside the file");
    for (int64_t j = 0; j < n_sel; ++j) {
        const int64_t f = frames ? frames[j] : j;
        size_t off[3];
        if (locate_frame(p, n, h, f, off, cell + 6 * j, err)) return 1;
        const size_t plane = (size_t)h.plane_count(f) * 4;
        for (int k = 0; k < 3; ++k)
            if (off[k] < lo || off[k] + plane > hi) return fail(err, "DCD frame descriptor lies outside the byte range");
        desc[j].x_off = off[0] - lo; desc[j].y_off = off[1] - lo; desc[j].z_off = off[2] - lo;
        desc[j].count = (uint32_t)h.plane_count(f);
        desc[j].flags = (h.swap() ? D_SWAP : 0u) | ((f != 0 && h.nfixed != 0) ? D_FREE_ONLY : 0u);
    }
    *byte_lo = (int64_t)lo;
    *byte_hi = (int64_t)hi;
    return 0;
}

// The selection (atoms, NULL = all) composed with the fixed-atom map, for the frames that hold free atoms only: src[i] >= 0 is an
// index into such a frame's planes, src[i] < 0 means atom -1 - src[i] of frame 0.  `sel` gets the checked atom indices themselves
// (the index into a full frame's planes).
inline int source_table(const Header& h, const int32_t* atoms, int64_t n_sel, int32_t* sel, int32_t* src, std::string& err)
{
    std::vector<int32_t> where;
    if (h.nfixed != 0) {
        where.assign((size_t)h.n_atoms, -1);
        for (size_t i = 0; i < h.free_idx.size(); ++i) where[(size_t)h.free_idx[i] - 1] = (int32_t)i;
    }
    for (int64_t i = 0; i < n_sel; ++i) {
        const int64_t a = atoms ? atoms[i] : i;
        if (a < 0 || a >= h.n_atoms) return fail(err, "atom index out of range");
        sel[i] = (int32_t)a;
        src[i] = h.nfixed == 0 ? (int32_t)a : (where[(size_t)a] >= 0 ? where[(size_t)a] : -1 - (int32_t)a);
    }
    return 0;
}

inline float plane_value(const uint8_t* plane, int64_t i, bool swap)
{
    const uint32_t u = word_at(plane + 4 * (size_t)i, swap);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// The host read path: selected frames and atoms into xyz [n_sel_frames, n_sel_atoms, 3], cells into cell [n_sel_frames, 6].
inline int read(const uint8_t* p, size_t n, const Header& h, const int64_t* frames, int64_t n_frames, const int32_t* atoms, int64_t n_sel,
                float* xyz, float* cell, std::string& err)
{
    std::vector<int32_t> sel((size_t)n_sel), src((size_t)n_sel);
    if (source_table(h, atoms, n_sel, sel.data(), src.data(), err)) return 1;
    size_t off0[3] = {0, 0, 0};
    float cell0[6];
    if (h.nfixed != 0 && locate_frame(p, n, h, 0, off0, cell0, err)) return 1;      // the fixed atoms live in frame 0
    const bool sw = h.swap();
    for (int64_t j = 0; j < n_frames; ++j) {
        const int64_t f = frames ? frames[j] : j;
        size_t off[3];
        if (locate_frame(p, n, h, f, off, cell + 6 * j, err)) return 1;
        const bool free_only = f != 0 && h.nfixed != 0;
        float* out = xyz + (size_t)j * (size_t)n_sel * 3;
        for (int64_t i = 0; i < n_sel; ++i) {
            const int32_t s = free_only ? src[(size_t)i] : sel[(size_t)i];
            for (int k = 0; k < 3; ++k) out[3 * i + k] = s >= 0 ? plane_value(p + off[k], s, sw) : plane_value(p + off0[k], -1 - s, sw);
        }
    }
    return 0;
}

// The file header the reference's writer produces for N atoms (276 bytes, CHARMM flavour, version 24, two title lines), with what it
// patches in after every frame already in place: NSET = n_frames at byte 8 and ISTART + n_frames * NSAVC at byte 20.  The second title
// line is the creation time, zero-padded.
constexpr size_t WRITE_HEADER_BYTES = 276;
inline void write_header(int32_t n_atoms, int32_t n_frames, int32_t istart, int32_t nsavc, double delta, bool with_cell, uint8_t* out)
{
    std::memset(out, 0, WRITE_HEADER_BYTES);
    auto put = [&](size_t at, int32_t v) { std::memcpy(out + at, &v, 4); };
    put(0, 84);
    std::memcpy(out + 4, "CORD", 4);
    put(8, n_frames);
    put(12, istart);
    put(16, nsavc);
    put(20, (int32_t)((uint32_t)istart + (uint32_t)n_frames * (uint32_t)nsavc));
    const float fdelta = (float)delta;
    std::memcpy(out + 44, &fdelta, 4);
    put(48, with_cell ? 1 : 0);
    put(84, 24);
    put(88, 84);
    put(92, 164);
    put(96, 2);
    std::strncpy((char*)out + 100, "Created by DCD plugin", 79);
    char stamp[80] = {0};
    const time_t now = time(nullptr);
    struct tm tmv;
    char when[32] = {0};
    if (localtime_r(&now, &tmv) && asctime_r(&tmv, when)) std::snprintf(stamp, sizeof stamp, "REMARKS Created %s", when);
    std::memcpy(out + 180, stamp, 80);
    put(260, 164);
    put(264, 4);
    put(268, n_atoms);
    put(272, 4);
}

// the six doubles of a frame's unit-cell record from lengths and angles (degrees), as the reference's writer forms them
inline void cell_record(const float lengths[3], const float angles[3], double out[6])
{
    out[0] = lengths[0];
    out[2] = lengths[1];
    out[5] = lengths[2];
    out[1] = std::sin((M_PI_2 / 90.0) * (90.0 - angles[2]));
    out[3] = std::sin((M_PI_2 / 90.0) * (90.0 - angles[1]));
    out[4] = std::sin((M_PI_2 / 90.0) * (90.0 - angles[0]));
}

}  // namespace dcd
}  // namespace mkamd
