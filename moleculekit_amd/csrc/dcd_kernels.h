// dcd_kernels.h -- DCD frames decoded and encoded on the device (include/mkamd_xtc.h "DCD"; host side: csrc/dcd_reader.h).
//
// A DCD frame is three planes of floats (x, y, z) between 4- or 8-byte record markers, at offsets the file's header fixes; the
// voxelizer and every metric here want frame-major items [frame, atom, 3].  Both kernels are that transpose and nothing else: the
// values travel as 32-bit patterns (byte-swapped per dword for an opposite-endian file) and are only touched as floats when a
// scale other than 1 is asked for, so NaN payloads and -0 arrive with the bits the reference reader returns.
//
//   k_dcd_decode   a block per (frame, tile of DCD_TILE selected atoms).  A thread gathers its atom's x, y, z through the source
//                  table -- one indirection: an index into the frame's planes, or, for a fixed atom of a file that stores free atoms
//                  only, -1 - atom into the resident copy of frame 0 -- and parks them in LDS; after the barrier the block writes the
//                  tile's 3 * DCD_TILE dwords one after the other.  Planes start 4 bytes behind a marker, and a frame's items at
//                  12 * n_sel * frame bytes: neither side is 16-byte aligned in general, so both sides move dwords -- consecutive
//                  lanes, consecutive dwords, whole 256-byte runs per wave instruction on the plane loads (identity selection) and on
//                  every store.
//                  A descriptor that reaches outside the n_bytes the kernel is given, or is not 4-byte aligned, sets the frame's
//                  status to 1 and stores nothing for that frame; so does (for its own item only) a table entry outside its plane.
//   k_dcd_encode   the reverse: a block reads a tile's 3 * DCD_TILE dwords of one frame in order into LDS and writes x, y and z runs
//                  into the three planes of the reference writer's frame image; the tile-0 block also writes the frame's markers and,
//                  when the file has unit cells, the 48-byte cell record from a host-computed [F, 6] array of doubles.  Every byte of
//                  the image is written exactly once, by plain vector stores; no atomics.
#pragma once
#ifndef MK_DEVICE_API_PROVIDED
#include "mk_device.h"
#endif
#include "dcd_reader.h"

namespace mkamd {

constexpr int DCD_TILE = 256;                       // atoms of a tile = threads of a block

MK_DEV unsigned dcd_word(const unsigned char* bytes, unsigned long long off, unsigned idx, bool swap)
{
    const unsigned v = reinterpret_cast<const unsigned*>(bytes + off)[idx];
    return swap ? __builtin_bswap32(v) : v;
}

MK_DEV unsigned dcd_scaled(unsigned bits, float scale)
{
    return scale != 1.0f ? mk_float_bits(mk_fmul_rn(mk_uint_as_float(bits), scale)) : bits;
}

// bytes: the uploaded byte range (4-byte aligned), n_bytes of it readable.  sel / src: int32 [n_sel], the index of each selected atom
// in a full frame's planes / in a free-atoms-only frame's planes (or -1 - atom: take it from frame0, f32 [n_atoms, 3], unscaled).
// status must be zeroed before the launch.  Grid: tiles * nframes blocks from frame `frame0_idx` on.
MK_KERNEL(256) void k_dcd_decode(const unsigned char* __restrict__ bytes, unsigned long long n_bytes, const dcd::FrameDesc* __restrict__ desc,
                                 long long first, const int* __restrict__ sel, const int* __restrict__ src, long long n_sel,
                                 const float* __restrict__ frame0, long long n_atoms, float scale, float* __restrict__ xyz,
                                 int* __restrict__ status, int tiles)
{
    __shared__ unsigned s[3 * DCD_TILE];
    const long long f = first + (long long)(blockIdx.x / (unsigned)tiles);
    const long long a0 = (long long)(blockIdx.x % (unsigned)tiles) * DCD_TILE;
    const int t = (int)threadIdx.x;
    const dcd::FrameDesc d = desc[f];
    const unsigned long long plane = 4ull * d.count;
    const bool free_only = (d.flags & dcd::D_FREE_ONLY) != 0, swap = (d.flags & dcd::D_SWAP) != 0;
    bool ok = plane <= n_bytes && d.x_off <= n_bytes - plane && d.y_off <= n_bytes - plane && d.z_off <= n_bytes - plane &&
              ((d.x_off | d.y_off | d.z_off) & 3ull) == 0;
    if (free_only && d.count < (unsigned long long)n_atoms && frame0 == nullptr) ok = false;
    if (!ok) {                                                   // (uniform over the block: nobody reaches the barrier)
        if (t == 0) status[f] = 1;
        return;
    }
    const long long a = a0 + t;
    bool good = true;
    unsigned vx = 0, vy = 0, vz = 0;
    if (a < n_sel) {
        const int i = free_only ? src[a] : sel[a];
        if (i >= 0) {
            good = (unsigned)i < d.count;
            if (good) {
                vx = dcd_word(bytes, d.x_off, (unsigned)i, swap);
                vy = dcd_word(bytes, d.y_off, (unsigned)i, swap);
                vz = dcd_word(bytes, d.z_off, (unsigned)i, swap);
            }
        } else {
            const long long fa = -1ll - (long long)i;
            good = free_only && frame0 != nullptr && fa < n_atoms;
            if (good) {
                vx = mk_float_bits(frame0[3 * fa]);
                vy = mk_float_bits(frame0[3 * fa + 1]);
                vz = mk_float_bits(frame0[3 * fa + 2]);
            }
        }
        if (!good) status[f] = 1;
    }
    s[3 * t] = dcd_scaled(vx, scale);
    s[3 * t + 1] = dcd_scaled(vy, scale);
    s[3 * t + 2] = dcd_scaled(vz, scale);
    // which items of the tile are stored: all of the selection's that were found in range (an item is 3 dwords: dword w belongs to item w / 3)
    __shared__ unsigned char keep[DCD_TILE];
    keep[t] = (a < n_sel && good) ? 1 : 0;
    mk_block_sync();
    unsigned* out = reinterpret_cast<unsigned*>(xyz) + ((size_t)f * (size_t)n_sel + (size_t)a0) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int w = k * DCD_TILE + t;
        if (keep[w / 3]) out[w] = s[w];
    }
}

// xyz f32 [F, N, 3]; cell f64 [F, 6] (the record's six doubles) or NULL for a file without unit cells; image: F frames of
// dcd_frame_bytes(N, cell) bytes, 4-byte aligned.  Grid: tiles * nframes blocks from frame `first` on.
inline unsigned long long dcd_frame_bytes(long long n_atoms, bool with_cell) { return (with_cell ? 56ull : 0ull) + 3ull * (4ull * (unsigned long long)n_atoms + 8ull); }

MK_KERNEL(256) void k_dcd_encode(const float* __restrict__ xyz, const double* __restrict__ cell, long long first, long long n_atoms,
                                 unsigned char* __restrict__ image, int tiles)
{
    __shared__ unsigned s[3 * DCD_TILE];
    const long long f = first + (long long)(blockIdx.x / (unsigned)tiles);
    const unsigned tile = blockIdx.x % (unsigned)tiles;
    const long long a0 = (long long)tile * DCD_TILE;
    const int t = (int)threadIdx.x;
    const long long left = n_atoms - a0;                          // atoms of this tile: min(left, DCD_TILE)
    const unsigned* in = reinterpret_cast<const unsigned*>(xyz) + ((size_t)f * (size_t)n_atoms + (size_t)a0) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int w = k * DCD_TILE + t;
        if ((long long)w < 3 * left) s[w] = in[w];
    }
    mk_block_sync();
    const unsigned cell_words = cell ? 14u : 0u;
    const size_t plane_words = (size_t)n_atoms + 2;              // marker, N floats, marker
    unsigned* img = reinterpret_cast<unsigned*>(image) + (size_t)f * ((size_t)cell_words + 3 * plane_words);
    if (tile == 0) {                                              // the frame's markers and its cell record
        const unsigned m = (unsigned)(4ull * (unsigned long long)n_atoms);
        if (t < 6) img[cell_words + (size_t)(t >> 1) * plane_words + ((t & 1) ? plane_words - 1 : 0)] = m;
        if (cell) {
            if (t == 6) img[0] = 48u;
            if (t == 7) img[13] = 48u;
            if (t >= 8 && t < 20) img[1 + (t - 8)] = reinterpret_cast<const unsigned*>(cell + 6 * f)[t - 8];
        }
    }
    if ((long long)t < left) {
        unsigned* p = img + cell_words + 1 + (size_t)a0 + t;
        p[0] = s[3 * t];
        p[plane_words] = s[3 * t + 1];
        p[2 * plane_words] = s[3 * t + 2];
    }
}

// ---- launch plans (the C ABI and the CPU tier's emulation drive the same ones) ----
template <class Backend>
int run_dcd_decode(Backend& be, const unsigned char* bytes, unsigned long long n_bytes, const dcd::FrameDesc* desc, long long n_frames,
                   const int* sel, const int* src, long long n_sel, const float* frame0, long long n_atoms, float scale, float* xyz, int* status)
{
    if (int st = be.fill(status, 0, (size_t)n_frames * sizeof(int))) return st;
    const long long tiles = (n_sel + DCD_TILE - 1) / DCD_TILE;
    if (tiles == 0) return 0;
    const long long per_launch = std::max<long long>(1, 0x7fffffffll / tiles);
    for (long long f0 = 0; f0 < n_frames; f0 += per_launch) {
        const long long nf = std::min(per_launch, n_frames - f0);
        if (int st = be.launch(k_dcd_decode, dim3((unsigned)(nf * tiles)), dim3(DCD_TILE), bytes, n_bytes, desc, f0, sel, src, n_sel, frame0, n_atoms,
                               scale, xyz, status, (int)tiles))
            return st;
    }
    return 0;
}

template <class Backend>
int run_dcd_encode(Backend& be, const float* xyz, const double* cell, long long n_frames, long long n_atoms, unsigned char* image)
{
    const long long tiles = (n_atoms + DCD_TILE - 1) / DCD_TILE;
    const long long per_launch = std::max<long long>(1, 0x7fffffffll / tiles);
    for (long long f0 = 0; f0 < n_frames; f0 += per_launch) {
        const long long nf = std::min(per_launch, n_frames - f0);
        if (int st = be.launch(k_dcd_encode, dim3((unsigned)(nf * tiles)), dim3(DCD_TILE), xyz, cell, f0, n_atoms, image, (int)tiles)) return st;
    }
    return 0;
}

}  // namespace mkamd
