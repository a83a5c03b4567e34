// dssp_pipeline.h -- launch plan of the secondary-structure kernels (dssp_kernels.h), written against the backend concept of
// pipeline.h so that the product (capi.hip) and the test emulator (tests/emu/emu_dssp.cpp) run the same plan.
#pragma once
#include "dssp_kernels.h"
#include "pipeline.h"

#include <string>

namespace mkamd {

enum { DSSP_AVOID_FRAMES = 1, DSSP_AVOID_ATOMS = 2, DSSP_SMALL_CHUNKS = 4 };    // `avoid`: the tests walk both energy plans, and chunks of 64 frames

constexpr long long DSSP_MAX_RESIDUES = 1LL << 18;
constexpr size_t DSSP_WORKSPACE_BYTES = (size_t)128 << 20;          // what a chunk of frames may take of the context's workspace
constexpr size_t DSSP_BYTES_PER_RESIDUE_FRAME = 15 * 4 + 3 * 2 * 4 + 4 + SS_BRIDGES * 4 + 8 * 5 * 4;       // see the carving below

// Lanes along the acceptors instead of the frames?  The frame kernel runs ceil(F / 64) * R waves of R steps each, the acceptor kernel
// F * R waves of R / 64 steps: the same work, and the many short waves win while the few long ones cannot fill the chip.  Measured
// on the MI355X (tools/bench_dssp.py): the plans cross at 150 frames of 223 residues and at 35 frames of 1 000 -- F * R = 33 000 and
// 35 000 -- so the switch is the product.
constexpr long long DSSP_ATOMS_BELOW = 32768;
inline bool dssp_takes_atoms(long long F, long long R) { return F * R < DSSP_ATOMS_BELOW; }

inline long long dssp_chunk_frames(long long F, long long R, int avoid)
{
    long long fc = (long long)(DSSP_WORKSPACE_BYTES / (DSSP_BYTES_PER_RESIDUE_FRAME * (size_t)R));
    if (avoid & DSSP_SMALL_CHUNKS) fc = WAVE;
    if (fc >= WAVE) fc -= fc % WAVE;                                 // whole waves of frames
    if (fc < 1) fc = 1;
    return fc < F ? fc : F;
}

// out uint8 [F, R]: the reference's integer codes (full: H 3 B 4 E 5 G 6 I 7 T 8 S 9 ' ' 10; simplified: helix 2, strand 1, coil 0);
// coords [N, 3, F]; ca uint32 [R], nco uint32 [R, 3] (every index < N: the caller's check), proline, chain int32 [R] -- all the
// device's.  after_chunk(ws, first frame, frames): what the emulator reads the slots through; the product passes nothing.
template <class BE, class AfterChunk>
int run_dssp(BE& be, const float* coords, long long F, const unsigned* ca, const unsigned* nco, const int* proline, const int* chain, long long R,
             int simplified, unsigned char* out, std::string& err, int avoid, AfterChunk&& after_chunk)
{
    if (F < 0 || R < 0) { err = "negative size"; return ST_EINVAL; }
    if (F > 0x3fffffffLL) { err = "too many frames (>= 2^30)"; return ST_EINVAL; }
    if (R > DSSP_MAX_RESIDUES) { err = "too many residues (> 2^18)"; return ST_EINVAL; }
    if (F == 0 || R == 0) return ST_OK;
    if (!coords || !ca || !nco || !proline || !chain || !out) { err = "NULL pointer"; return ST_EINVAL; }
    const bool atoms = (avoid & DSSP_AVOID_FRAMES) || (!(avoid & DSSP_AVOID_ATOMS) && dssp_takes_atoms(F, R));
    be.note_dist_kernel(atoms ? "mkamd::k_dssp_energy_atoms" : "mkamd::k_dssp_energy_frames");
    const long long Fc = dssp_chunk_frames(F, R, avoid);
    int st;
    int* run_start = nullptr;
    if ((st = ensure_as(be, WS_SS_SEG, (size_t)R * sizeof(int), run_start, 0))) return st;
    // the chunk's arrays, carved out of one buffer: the 4-byte ones first (each R * Fc words long), then the bytes
    const size_t cell = (size_t)R * (size_t)Fc;
    char* base = nullptr;
    if ((st = ensure_as(be, WS_SS_WORK, cell * DSSP_BYTES_PER_RESIDUE_FRAME, base, 0))) return st;
    DsspWs w{};
    w.R = R; w.Fc = Fc; w.L = 8 * R; w.run_start = run_start;
    size_t words = 0;
    auto take = [&](size_t n) { char* p = base + words * 4; words += n * cell; return p; };
    w.bb = (float*)take(15);
    w.slot_a = (int*)take(2); w.slot_e = (float*)take(2); w.hba = (int*)take(2);
    w.br = (unsigned*)take(SS_BRIDGES);
    w.lad = (int*)take(8 * 5);
    w.flags = (unsigned char*)(base + words * 4);
    w.nbr = w.flags + cell;
    w.label = w.nbr + cell;                                          // two planes
    if ((st = be.launch(k_dssp_segments, dim3(1), dim3(WAVE), chain, R, run_start))) return st;
    for (long long f0 = 0; f0 < F; f0 += Fc) {
        DsspWs c = w;
        const long long fc = F - f0 < Fc ? F - f0 : Fc;              // (the last chunk: the same buffers at a smaller frame pitch)
        c.Fc = fc;
        const long long n = R * fc;
        const dim3 per_cell((unsigned)((n + SSL_THREADS - 1) / SSL_THREADS)), blk(SSL_THREADS);
        if ((st = be.launch(k_dssp_backbone, per_cell, dim3(SSB_THREADS), c, coords, F, f0, ca, nco, chain))) return st;
        const long long waves = atoms ? n : ((fc + WAVE - 1) / WAVE) * R;
        const dim3 egrid((unsigned)((waves + 3) / 4));
        if ((st = atoms ? be.launch(k_dssp_energy_atoms, egrid, dim3(SSE_THREADS), c, proline)
                        : be.launch(k_dssp_energy_frames, egrid, dim3(SSE_THREADS), c, proline))) return st;
        if ((st = be.launch(k_dssp_local, per_cell, blk, c))) return st;
        if ((st = be.launch(k_dssp_sheets, dim3((unsigned)((fc + SSS_THREADS - 1) / SSS_THREADS)), dim3(SSS_THREADS), c))) return st;
        if ((st = be.launch(k_dssp_helix3, per_cell, blk, c))) return st;
        if ((st = be.launch(k_dssp_finish, per_cell, blk, c, simplified, f0, out))) return st;
        if ((st = after_chunk(c, f0, fc))) return st;
    }
    return ST_OK;
}

}  // namespace mkamd
