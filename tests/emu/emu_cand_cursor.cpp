// tests/emu/emu_cand_cursor.cpp -- TEST INFRASTRUCTURE: the run cursor of the tile kernels' candidate traversal (round 9;
// kernels.h: link_candidate_runs, CandCursor, cand_issue) on the host emulation.  The emulation library's translation unit, whole, plus
// one entry point that walks a GIVEN table of 64 runs with the product's own cand_issue, one wave, and writes down what every lane of
// every chunk got.  (The kernels with fold and cursor together run through tests/emu/emu_cover_fold.cpp.)
#include "emu_capi.cpp"

namespace mkamd {
// chunks first, first + stride, ... (a team's dealing: wave `first` of `stride`), `batch` of them issued back to back as
// for_each_candidate does; `strided`: what it passes to cand_issue (batch_stride != 1: the per-chunk search instead of the cursor).  out [T][64][4] = valid, record index, code, the class word loaded from that record; meta = N, T, codable
void k_emu_cand_cursor_walk(const unsigned* r0, const unsigned* len, const float4* rec_pos, const unsigned* rec_cls, unsigned first, unsigned stride,
                            int batch, int strided, unsigned* out, unsigned* meta)
{
    const int lane = threadIdx.x & (WAVE - 1);
    CandRuns cr;
    cr.r0 = r0[lane]; cr.len = len[lane];
    link_candidate_runs(cr);
    if (lane == 0) { meta[0] = cr.N; meta[1] = cr.T; meta[2] = cr.codable ? 1u : 0u; }
    const GridDesc g{};
    const TileGeom tg{};
    const CandLoader ld{g, tg, cr, rec_pos, rec_cls};
    CandCursor cur = cand_cursor_begin(cr);
    for (unsigned t = first; t < cr.T; t += (unsigned)batch * stride) {
        for (int k = 0; k < batch; ++k) {
            const unsigned tk = t + (unsigned)k * stride;
            CandChunk ch;
            cand_issue<true>(ld, cur, strided, tk, ch);                 // (past T: a chunk of invalid lanes, as in the product's batches)
            if (tk < cr.T) {
                unsigned* o = out + ((size_t)tk * WAVE + lane) * 4;
                o[0] = ch.valid ? 1u : 0u; o[1] = ch.r; o[2] = ch.code; o[3] = ch.ids;
            }
        }
    }
}
}  // namespace mkamd

extern "C" int emu_cand_cursor_walk(const unsigned* r0, const unsigned* len, const unsigned* rec_cls, long long n_rec, unsigned first, unsigned stride,
                                    int batch, int strided, unsigned* out, unsigned* meta)
{
    std::vector<float4> pos((size_t)n_rec + 1, make_float4(0.f, 0.f, 0.f, 0.f));
    emu::launch(k_emu_cand_cursor_walk, dim3(1), dim3(64), r0, len, (const float4*)pos.data(), rec_cls, first, stride, batch, strided, out, meta);
    return 0;
}
