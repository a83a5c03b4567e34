/* mkamd_xtc.h -- C ABI of the XTC trajectory decoder in libmkamd.so ("trajectory feeding").
 *
 * Host-side, no GPU involved: what the reference does in moleculekit/fileformats/xtc (xtc.pyx: read_xtc :34-53,
 * read_xtc_frames :57-81, get_xtc_natoms / get_xtc_nframes; src/xdrfile.cpp: xdrfile_decompress_coord_float :749-983;
 * src/xtc_src.cpp: xtc_read_new :195-262, xtc_read_frame :471-624).  Same float32 bits out.  Frames are decoded in
 * parallel on host threads (they are independent records); the reference decodes them one by one.
 *
 * Status: 0 = ok; non-zero = error, message via mkamd_last_error() (mkamd_voxel.h).
 */
#ifndef MKAMD_XTC_H
#define MKAMD_XTC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Atom count and number of (complete) frames of an XTC file  -- get_xtc_natoms / get_xtc_nframes (xtc.pyx:14-31). */
int mkamd_xtc_info(const char* path, int64_t* n_atoms, int64_t* n_frames);

/* Decode frames into caller-owned arrays with the reference's layouts (frame index fastest):
 *   coords f32 [n_atoms, 3, n_sel] in nm, box f32 [3, 3, n_sel] (box vectors, nm), time f32 [n_sel] (ps), step i32 [n_sel].
 * frames: n_sel frame indices (any order, repeats allowed), or NULL for frames 0 .. n_sel-1
 * (read_xtc = NULL with n_sel = n_frames; read_xtc_frames = an index list).  n_atoms must match the file.
 * n_threads: host threads to decode with, 0 = automatic (up to 32). */
int mkamd_xtc_read(const char* path, const int64_t* frames, int64_t n_sel, int64_t n_atoms, float* coords, float* box,
                   float* time, int32_t* step, int32_t n_threads);

/* Decoding ON THE DEVICE (round 4; csrc/xtc_gpu.h).  Frames are independent records; inside a frame only the WALK of the bit
 * stream is serial (where an atom's bits start depends on the flag / run length after every full-precision atom before it:
 * xdrfile.cpp:749-983).  So a GPU lane walks a frame and records where each group -- a full atom and the run of small atoms
 * after it -- starts, then a thread per group decodes the numbers; the host only parses the record headers and copies the
 * records' bytes.
 *   mkamd_xtc_chunk_desc   headers of the selected frames -> one 64-byte descriptor per frame (desc_out: n_sel x 64 bytes, the
 *                          layout of mkamd::XtcFrameDesc in csrc/xtc_gpu.h; data offsets relative to *byte_lo), the byte range
 *                          [*byte_lo, *byte_hi) of the file that holds their records, and what the host path returns besides the
 *                          coordinates: box vectors f32 [3,3,n_sel] (nm), time f32 [n_sel] (ps), step i32 [n_sel]
 *   mkamd_xtc_copy_bytes   that byte range into caller memory (pinned staging), by a few host threads (pread)
 *   mkamd_xtc_byte_range   (round 6) the byte range of the selection from the frame index alone -- a streaming reader copies the
 *                          bytes FIRST and then parses the headers out of its copy:
 *   mkamd_xtc_chunk_desc_mem   mkamd_xtc_chunk_desc from a host copy of the file's bytes [bytes_lo, bytes_hi) (the same results and
 *                          checks; a header read through a fresh mapping of the file costs a page fault: 2 ms per 2 048 frames)
 *   mkamd_xtc_decode_work_bytes   size of the device work buffer a decode of n_frames x n_atoms needs (8 bytes per atom: the
 *                          group records)
 *   mkamd_xtc_decode_dev   (needs mkamd_voxel.h's context) d_bytes / d_desc = device copies of the two, d_bytes
 *                          MKAMD_XTC_PAD bytes LONGER than the range (the kernels read ahead of what they use) and 4-byte
 *                          aligned: coordinates float32 [n_frames, n_atoms, 3] -- frame-major, the voxelizer's packed items --
 *                          times `scale` (10 = nm -> Angstrom), with the float32 operations of the host path ((float)int *
 *                          (1 / precision), then * scale: the same bits); d_status[f] = 0 ok, 1 corrupt stream, 2 outside what
 *                          the device path takes (a mixed-radix number of more than 64 bits, a frame of >= 2^21 atoms or
 *                          >= 512 MB: take the host decoder for such a file; that frame's coordinates are not written).
 *                          d_work: 8-byte aligned, only used during the call's kernels.  Asynchronous on `hip_stream`. */
#define MKAMD_XTC_PAD 1024
int mkamd_xtc_chunk_desc(const char* path, const int64_t* frames, int64_t n_sel, int64_t n_atoms, void* desc_out,
                         int64_t* byte_lo, int64_t* byte_hi, float* box, float* time, int32_t* step);
int mkamd_xtc_copy_bytes(const char* path, int64_t byte_lo, int64_t byte_hi, void* dst, int32_t n_threads);
int mkamd_xtc_byte_range(const char* path, const int64_t* frames, int64_t n_sel, int64_t n_atoms, int64_t* byte_lo, int64_t* byte_hi);
int mkamd_xtc_chunk_desc_mem(const char* path, const int64_t* frames, int64_t n_sel, int64_t n_atoms, const void* bytes, int64_t bytes_lo,
                             int64_t bytes_hi, void* desc_out, int64_t* byte_lo, int64_t* byte_hi, float* box, float* time, int32_t* step);
uint64_t mkamd_xtc_decode_work_bytes(int64_t n_frames, int64_t n_atoms);
struct mkamd_ctx;
int mkamd_xtc_decode_dev(struct mkamd_ctx* ctx, void* hip_stream, const void* d_bytes, const void* d_desc, int64_t n_frames,
                         int64_t n_atoms, float scale, float* d_xyz, int32_t* d_status, void* d_work, uint64_t work_bytes);

/* Compression ON THE DEVICE (csrc/xtc_encode.h): the file image of frames that are resident on the GPU, byte for byte what the
 * reference's writer makes of them (xtc_src.cpp: xtc_write :410-469; xdrfile.cpp: xdrfile_compress_coord_float :985-1279 -- runs of
 * small atoms, the water swap, the adaptive small-number index).  A thread per atom quantises, a lane per frame walks the integers
 * and records where every group starts, a thread per group packs its bits.
 *   mkamd_xtc_encode_work_bytes   size of the device work buffer an encode of n_frames x n_atoms needs (~24 bytes per atom)
 *   mkamd_xtc_encode_bound        upper bound of the image in bytes (13 bytes per atom and 92 per frame, rounded up to words)
 *   mkamd_xtc_encode_dev          d_xyz f32 [n_frames, n_atoms, 3] (frame-major), times `in_scale` (1 = nm input, the float32 0.1 =
 *                          Angstrom) with one float32 rounding, as the host path of the reference does before it writes;
 *                          d_precision f32 [n_frames] (<= 0 is written as 1000), d_box f32 [n_frames, 3, 3] (box vectors, nm),
 *                          d_time f32 [n_frames] (ps), d_step i32 [n_frames].  Out: d_image (4-byte aligned, image_capacity >=
 *                          mkamd_xtc_encode_bound bytes; the records one after the other, only bytes below d_offsets[n_frames] are
 *                          written), d_offsets u64 [n_frames + 1] (a refused frame takes no bytes), d_status i32 [n_frames]: 0 ok,
 *                          2 outside what the device path takes and nothing of that frame written -- a coordinate that is not
 *                          finite or leaves the int range at this precision, a range of >= INT_MAX - 2 quanta, a full triple of more
 *                          than 64 bits, a header small-number index + 8 > 64 (the rule of the device decoder; the reference reads
 *                          past its own table there), >= 2^21 atoms.  d_work: 8-byte aligned, only used during the call's
 *                          kernels.  Both sizes are checked before any launch.  Asynchronous on `hip_stream`. */
uint64_t mkamd_xtc_encode_work_bytes(int64_t n_frames, int64_t n_atoms);
uint64_t mkamd_xtc_encode_bound(int64_t n_frames, int64_t n_atoms);
int mkamd_xtc_encode_dev(struct mkamd_ctx* ctx, void* hip_stream, const float* d_xyz, float in_scale, const float* d_precision,
                         const float* d_box, const float* d_time, const int32_t* d_step, int64_t n_frames, int64_t n_atoms, void* d_image,
                         uint64_t image_capacity, uint64_t* d_offsets, int32_t* d_status, void* d_work, uint64_t work_bytes);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * DCD (CHARMM / NAMD / X-PLOR / OpenMM trajectories; csrc/dcd_reader.h, csrc/dcd_kernels.h).  What the reference does in
 * moleculekit/fileformats/dcd (src/dcdplugin.c, dcd.pyx): coordinates are float32 bit patterns carried unchanged, Angstrom.
 * A frame is three planes of floats at offsets the header fixes; the host parses the header and checks every selected frame's
 * markers, the device gathers, byte-swaps and transposes.
 *   mkamd_dcd_info          atom count, frame count (from the file's size: a frame cut off at the end is not counted), ISTART, NSAVC,
 *                           DELTA, the number of fixed atoms and flags (1 opposite endian, 2 64-bit record markers, 4 CHARMM, 8 unit
 *                           cells, 16 a 4th dimension).  Refused with a message: opposite endian with a 4th dimension (the reference
 *                           misreads it), N <= 0, fixed atoms outside [0, N), free indices outside 1..N or not strictly ascending.
 *   mkamd_dcd_chunk_desc    the selected frames (any order, repeats allowed; NULL = 0 .. n_sel-1) -> one 32-byte descriptor each
 *                           (mkamd::dcd::FrameDesc: byte offsets of the x, y, z planes counted from *byte_lo, floats per plane, flags:
 *                           1 swap, 2 free atoms only), the byte range [*byte_lo, *byte_hi) that holds them (a multiple of 4, copy it
 *                           with mkamd_xtc_copy_bytes) and the unit cells f32 [n_sel, 6]: A, B, C, alpha, beta, gamma (degrees; from
 *                           the stored cosines when all three lie in [-1, 1]; 0 0 0 90 90 90 in a file without cells).  Every marker
 *                           of a selected frame is checked against N, every descriptor against the file's size.
 *   mkamd_dcd_source_table  the atom selection (NULL = all n_sel = N atoms) composed with the fixed-atom map: sel i32 [n_sel] the checked
 *                           indices (into a full frame's planes), src i32 [n_sel] for a frame of free atoms only: >= 0 an index into its
 *                           planes, < 0 atom -1 - src of frame 0
 *   mkamd_dcd_read          the host path: selected frames and atoms into xyz f32 [n_frames, n_sel, 3], cells f32 [n_frames, 6]
 *   mkamd_dcd_decode_dev    (needs mkamd_voxel.h's context) d_bytes = device copy of the byte range (4-byte aligned, n_bytes long),
 *                           d_desc / d_sel / d_src device copies of the above, d_frame0 f32 [n_atoms, 3] = frame 0 decoded with the
 *                           identity selection and scale 1 (NULL for a file without fixed atoms) -> d_xyz f32 [n_frames, n_sel, 3]
 *                           times `scale` (multiplied only when != 1), d_status i32 [n_frames]: 0 ok, 1 a descriptor that reaches
 *                           outside n_bytes or is misaligned (nothing of that frame is stored) or a table entry outside its plane (that
 *                           item is not stored).  Asynchronous on `hip_stream`.
 *   mkamd_dcd_encode_bound  bytes of the image of n_frames frames: (with_cell ? 56 : 0) + 3 * (4 * n_atoms + 8) each
 *   mkamd_dcd_encode_dev    d_xyz f32 [n_frames, n_atoms, 3] -> the reference writer's frame images one after the other in d_image
 *                           (4-byte aligned); d_cell f64 [n_frames, 6] = the six doubles of each frame's cell record (mkamd_dcd_cell_record),
 *                           or NULL for a file without unit cells.  Every byte is written exactly once.  Asynchronous on `hip_stream`.
 *   mkamd_dcd_cell_record   lengths / angles f32 [n, 3] (degrees) -> the cell records f64 [n, 6]: A, cos(gamma), B, cos(beta), cos(alpha), C
 *                           with the cosines as sin(pi/2 / 90 * (90 - angle)), like the reference's writer
 *   mkamd_dcd_header        the 276-byte file header of that writer with NSET = n_frames (byte 8) and ISTART + n_frames * NSAVC (byte 20)
 *                           in place; bytes [180, 260) are "REMARKS Created <asctime>", zero-padded. */
#define MKAMD_DCD_DESC_BYTES 32
#define MKAMD_DCD_HEADER_BYTES 276
int mkamd_dcd_info(const char* path, int64_t* n_atoms, int64_t* n_frames, int32_t* istart, int32_t* nsavc, double* delta, int32_t* n_fixed,
                   int32_t* flags);
int mkamd_dcd_chunk_desc(const char* path, const int64_t* frames, int64_t n_sel, void* desc_out, int64_t* byte_lo, int64_t* byte_hi,
                         float* cell);
int mkamd_dcd_source_table(const char* path, const int32_t* atoms, int64_t n_sel, int32_t* sel, int32_t* src);
int mkamd_dcd_read(const char* path, const int64_t* frames, int64_t n_frames, const int32_t* atoms, int64_t n_sel, float* xyz, float* cell);
int mkamd_dcd_decode_dev(struct mkamd_ctx* ctx, void* hip_stream, const void* d_bytes, uint64_t n_bytes, const void* d_desc, int64_t n_frames,
                         const int32_t* d_sel, const int32_t* d_src, int64_t n_sel, const float* d_frame0, int64_t n_atoms, float scale,
                         float* d_xyz, int32_t* d_status);
uint64_t mkamd_dcd_encode_bound(int64_t n_frames, int64_t n_atoms, int32_t with_cell);
int mkamd_dcd_encode_dev(struct mkamd_ctx* ctx, void* hip_stream, const float* d_xyz, const double* d_cell, int64_t n_frames, int64_t n_atoms,
                         void* d_image, uint64_t image_capacity);
int mkamd_dcd_cell_record(const float* lengths, const float* angles, int64_t n, double* out);
int mkamd_dcd_header(int64_t n_atoms, int64_t n_frames, int32_t istart, int32_t nsavc, double delta, int32_t with_cell, void* out);

#ifdef __cplusplus
}
#endif
#endif
