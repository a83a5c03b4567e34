// wrap_cell_kernels.h -- HIP kernels of the periodic wrap of TRICLINIC boxes (moleculekit wrapping/wrapping.pyx::wrap_triclinic_unitcell
// and wrap_compact_unitcell, called from Molecule.wrap when a box angle is not 90) on MI355X (gfx950): all three unit cells
// (DESIGN.md section 13).  The rectangular cell of a rectangular box stays wrap_kernels.h's.
//
// Layout: coordinates frame-major float32 [F, N, 3]; box vectors float64 [3, 3, F], row i the vector i, lower triangular
// (box[0][1] = box[0][2] = box[1][2] = 0); groups, centre selection and centre as in wrap_kernels.h.
//
// The arithmetic is the reference's to the bit, every operation rounded on its own (mk_f*_rn, mk_dadd_rn / mk_dmul_rn, IEEE division;
// nothing contracted, no reciprocal).  Per frame:
//   box_middle (float32)    bm[j] = float(double(bm[j]) + 0.5 * box[i][j])  for i (outer), j (inner)
//   every atom              xc = (x - wrap_centre) + bm   (float32; wrap_centre: k_wrap_centre's running mean over the centre selection
//                           of the UNWRAPPED frame, or the three floats given)
//   group centre (float32)  the running mean of wrap_kernels.h over xc
// MODE 2, "triclinic" (GROMACS' put_atoms_in_triclinic_unitcell): float64 shm01 = b10 / b11, shm02 = (b11 b20 - b21 b10) / (b11 b22),
//   shm12 = b21 / b22 and shift_centre = double(bm) - 0.5 * (b0 + b1 + b2), transformed in place ([0] from the untransformed [1] and [2],
//   then [1], then [2] = 0).  Per group for m = 2, 1, 0: shift = shift_centre[m] (+ shm12 gc[2] for m = 1; + (shm01 gc[1] + shm02 gc[2])
//   for m = 0), formed ONCE from the current float32 centre; while double(gc[m]) - shift < 0: gc[d] = float(double(gc[d]) + box[m][d]) for
//   d <= m; while double(gc[m]) - shift >= box[m][m]: the same with -.  Every atom: x_m = xc_m - (gc_init[m] - gc[m]) in float32.
// MODE 0 "rectangular" and MODE 1 "compact" (GROMACS' low_set_pbc and pbc_dx): per frame, in float64, hbox = box[i][i] / 2,
//   max_cutoff2 and up to 12 triclinic vectors (26 shift combinations in the order 0, -1, 1; skewness margin 1.001); per group
//   dx = double(gc - bm) (a float32 difference), moved by whole box vectors (MODE 0: by the diagonal only) into (-hbox, hbox], MODE 1:
//   then, inside the loop over the axes as the reference has it, the search over the triclinic vectors while |dx|^2 > max_cutoff2.
//   Every atom: x = float(double((xc - gc) + bm) + dx).
// Every atom of every group is written in all three modes (everything is recentred).
//
// Loops that must end: the reference's `while` loops never end for an infinite centre, or a box length that is zero, negative or
// below half an ulp of the centre.  Here every such loop stops after WRAP_CELL_MAX_STEPS steps (the reference moves one cell a step);
// the lane then writes the group with what it has and stores 1 to status[WRAP_CELL_ST_CAP].  A frame with a non-finite box vector, a
// box[1][1] or box[2][2] that is not positive, or a non-zero upper triangle is flagged by the prep kernel: the group kernels copy it
// through unchanged and store 1 to status[WRAP_CELL_ST_FRAME].  More than 12 triclinic vectors (the reference raises "Too many triclinic
// vectors!!"): the frame is flagged too and status[WRAP_CELL_ST_VECTORS] is set.  Status words are plain ints that lanes store the
// constant 1 to with ordinary stores; nobody clears them here.  No atomics of any kind: the same bits on every run.
//
//   k_wrap_cell_prep          a lane per frame: the frame's record (WrapCellFrame) into the workspace.  The triclinic vectors stay in
//                             the record and are read from memory by index (a per-lane array indexed at run time would be scratch).
//   k_wrap_cell_lanes<MODE>   a lane per (frame, group) for groups of at most `small_max` atoms.
//   k_wrap_cell_waves<MODE>   a wave per (frame, listed group): k_wrap_waves' structure -- WRAP_CHUNK atoms at a time coalesced into
//                             LDS, recentred on the way in; lanes 0..2 run the three chains; lane 0 decides (the axes are coupled);
//                             the float32 deltas (MODE 2) or the float64 dx are broadcast by readlane; the wave applies them coalesced.
#pragma once
#include "wrap_kernels.h"

namespace mkamd {

constexpr int WRAP_CELL_MAX_STEPS = 4096;
constexpr int WRAP_CELL_MAX_VECTORS = 12;
enum { WRAP_CELL_RECTANGULAR = 0, WRAP_CELL_COMPACT = 1, WRAP_CELL_TRICLINIC = 2 };
enum { WRAP_CELL_ST_CAP = 0, WRAP_CELL_ST_FRAME = 1, WRAP_CELL_ST_VECTORS = 2, WRAP_CELL_NSTATUS = 3 };

// what the group kernels need of a frame
struct WrapCellFrame {
    double b00, b10, b11, b20, b21, b22;               // the lower triangle
    double shm01, shm02, shm12, sc0, sc1;              // MODE 2 (shift_centre[2] is 0)
    double hbox[3], max_cutoff2;                       // MODE 0, 1
    double tric[WRAP_CELL_MAX_VECTORS][3];
    float bm[3];                                       // box_middle
    int ntric;
    int flag;                                          // not 0: the frame is copied through unchanged
    int pad;
};

MK_DEV double wc_dsub(double a, double b) { return mk_dadd_rn(a, -b); }            // (a - b and a + (-b) round alike)
MK_DEV double wc_ddiv(double a, double b)
{
#pragma clang fp contract(off)
    return a / b;                                                                    // IEEE division
}
MK_DEV double wc_min(double a, double b) { return a < b ? a : b; }                  // the reference's cmin / cmax, NaNs as they fall
MK_DEV double wc_max(double a, double b) { return a > b ? a : b; }
MK_DEV double wc_sq(double a) { return mk_dmul_rn(a, a); }
MK_DEV double wc_norm2(double x, double y, double z) { return mk_dadd_rn(mk_dadd_rn(wc_sq(x), wc_sq(y)), wc_sq(z)); }
MK_DEV bool wc_finite(double a) { return __builtin_fabs(a) < __builtin_inf(); }     // false for a NaN
MK_DEV float wc_recentre(float x, float wc, float bm) { return mk_fadd_rn(mk_fsub_rn(x, wc), bm); }

// the frame's box is one the reference's loops do not end on, or not lower triangular
MK_DEV bool wrap_cell_box_bad(const double (&b)[3][3])
{
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) finite = finite && wc_finite(b[i][j]);
    return !finite || !(b[1][1] > 0.0) || !(b[2][2] > 0.0) || b[0][1] != 0.0 || b[0][2] != 0.0 || b[1][2] != 0.0;
}

// Frame f's record.  mode: the triclinic vectors are the reference's get_pbc, which MODE 2 does not call.
MK_KERNEL_OCC(64, 8) void k_wrap_cell_prep(const double* __restrict__ boxv, long long F, int mode, WrapCellFrame* __restrict__ recs, int* status)
{
    const long long f = (long long)blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    WrapCellFrame* r = recs + f;
    double b[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) b[i][j] = boxv[(long long)(3 * i + j) * F + f];
    r->b00 = b[0][0]; r->b10 = b[1][0]; r->b11 = b[1][1]; r->b20 = b[2][0]; r->b21 = b[2][1]; r->b22 = b[2][2];
    r->ntric = 0;
    r->pad = 0;
    if (wrap_cell_box_bad(b)) {
        r->flag = 1;
        if (status) status[WRAP_CELL_ST_FRAME] = 1;
        return;
    }
    float bm[3] = {0.0f, 0.0f, 0.0f};
    double sc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            bm[j] = (float)mk_dadd_rn((double)bm[j], mk_dmul_rn(0.5, b[i][j]));
            sc[j] = mk_dadd_rn(sc[j], b[i][j]);
        }
    r->bm[0] = bm[0]; r->bm[1] = bm[1]; r->bm[2] = bm[2];
    const double shm01 = wc_ddiv(b[1][0], b[1][1]);
    const double shm02 = wc_ddiv(wc_dsub(mk_dmul_rn(b[1][1], b[2][0]), mk_dmul_rn(b[2][1], b[1][0])), mk_dmul_rn(b[1][1], b[2][2]));
    const double shm12 = wc_ddiv(b[2][1], b[2][2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) sc[j] = wc_dsub((double)bm[j], mk_dmul_rn(sc[j], 0.5));
    r->shm01 = shm01; r->shm02 = shm02; r->shm12 = shm12;
    r->sc0 = mk_dadd_rn(mk_dmul_rn(shm01, sc[1]), mk_dmul_rn(shm02, sc[2]));
    r->sc1 = mk_dmul_rn(shm12, sc[2]);
    double hbox[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { hbox[i] = mk_dmul_rn(b[i][i], 0.5); r->hbox[i] = hbox[i]; }
    int flag = 0, ntric = 0;
    r->max_cutoff2 = 0.0;
    if (mode != WRAP_CELL_TRICLINIC) {
        double min_hv2 = mk_dmul_rn(0.25, wc_min(wc_norm2(b[0][0], b[0][1], b[0][2]), wc_norm2(b[1][0], b[1][1], b[1][2])));
        min_hv2 = wc_min(min_hv2, mk_dmul_rn(0.25, wc_norm2(b[2][0], b[2][1], b[2][2])));
        const double min_ss = wc_min(b[0][0], wc_min(wc_dsub(b[1][1], __builtin_fabs(b[2][1])), b[2][2]));
        r->max_cutoff2 = wc_min(min_hv2, wc_sq(min_ss));
        const double margin = 1.001;
#pragma unroll 1
        for (int kk = 0; kk < 3; ++kk) {
            const int k = kk == 0 ? 0 : kk == 1 ? -1 : 1;
#pragma unroll 1
            for (int jj = 0; jj < 3; ++jj) {
                const int j = jj == 0 ? 0 : jj == 1 ? -1 : 1;
#pragma unroll 1
                for (int ii = 0; ii < 3; ++ii) {
                    const int i = ii == 0 ? 0 : ii == 1 ? -1 : 1;
                    if (!(j != 0 || k != 0)) continue;
                    // (the trial vector goes to the next free slot of the record at once and counts only if it is used: it need not
                    //  stay in registers through the checks below)
                    double d2old = 0.0, d2new = 0.0, moved[3];
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const double trial = mk_dadd_rn(mk_dadd_rn(mk_dmul_rn((double)i, b[0][d]), mk_dmul_rn((double)j, b[1][d])), mk_dmul_rn((double)k, b[2][d]));
                        const double pos = trial < 0.0 ? wc_min(hbox[d], -trial) : wc_max(-hbox[d], -trial);
                        if (ntric < WRAP_CELL_MAX_VECTORS) r->tric[ntric][d] = trial;
                        moved[d] = mk_dadd_rn(pos, trial);
                        d2old = mk_dadd_rn(d2old, wc_sq(pos));
                        d2new = mk_dadd_rn(d2new, wc_sq(moved[d]));
                    }
                    const double bound = mk_dmul_rn(margin, d2new);
                    if (!(bound < d2old)) continue;
                    bool use = true;
#pragma unroll
                    for (int dd = 0; dd < 3; ++dd) {
                        const int shift = dd == 0 ? i : dd == 1 ? j : k;
                        if (shift != 0 && use) {                                        // (`use` gone: the reference's break)
                            double d2c = 0.0;
#pragma unroll
                            for (int e = 0; e < 3; ++e) d2c = mk_dadd_rn(d2c, wc_sq(wc_dsub(moved[e], mk_dmul_rn((double)shift, b[dd][e]))));
                            if (d2c <= bound) use = false;
                        }
                    }
                    if (!use) continue;
                    if (ntric >= WRAP_CELL_MAX_VECTORS) {
                        flag = 2;
                        continue;
                    }
                    ++ntric;
                }
            }
        }
    }
    r->ntric = ntric;
    r->flag = flag;
    if (flag && status) status[WRAP_CELL_ST_VECTORS] = 1;
}

// MODE 2: the three float32 deltas gc_init[m] - gc[m] of a group whose centre is (c0, c1, c2).  Returns whether a loop hit the cap.
MK_DEV bool wrap_cell_triclinic(const WrapCellFrame* __restrict__ r, float c0, float c1, float c2, float& d0, float& d1, float& d2)
{
    float g0 = c0, g1 = c1, g2 = c2;
    bool capped = false;
    const double b00 = r->b00, b10 = r->b10, b11 = r->b11, b20 = r->b20, b21 = r->b21, b22 = r->b22;
    int steps;
    // m = 2: shift = shift_centre[2] = 0
    double shift = 0.0;
    for (steps = 0; wc_dsub((double)g2, shift) < 0.0; ++steps) {
        if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; }
        g0 = (float)mk_dadd_rn((double)g0, b20); g1 = (float)mk_dadd_rn((double)g1, b21); g2 = (float)mk_dadd_rn((double)g2, b22);
    }
    for (steps = 0; wc_dsub((double)g2, shift) >= b22; ++steps) {
        if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; }
        g0 = (float)wc_dsub((double)g0, b20); g1 = (float)wc_dsub((double)g1, b21); g2 = (float)wc_dsub((double)g2, b22);
    }
    // m = 1
    shift = mk_dadd_rn(r->sc1, mk_dmul_rn(r->shm12, (double)g2));
    for (steps = 0; wc_dsub((double)g1, shift) < 0.0; ++steps) {
        if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; }
        g0 = (float)mk_dadd_rn((double)g0, b10); g1 = (float)mk_dadd_rn((double)g1, b11);
    }
    for (steps = 0; wc_dsub((double)g1, shift) >= b11; ++steps) {
        if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; }
        g0 = (float)wc_dsub((double)g0, b10); g1 = (float)wc_dsub((double)g1, b11);
    }
    // m = 0
    shift = mk_dadd_rn(r->sc0, mk_dadd_rn(mk_dmul_rn(r->shm01, (double)g1), mk_dmul_rn(r->shm02, (double)g2)));
    for (steps = 0; wc_dsub((double)g0, shift) < 0.0; ++steps) {
        if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; }
        g0 = (float)mk_dadd_rn((double)g0, b00);
    }
    for (steps = 0; wc_dsub((double)g0, shift) >= b00; ++steps) {
        if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; }
        g0 = (float)wc_dsub((double)g0, b00);
    }
    d0 = mk_fsub_rn(c0, g0); d1 = mk_fsub_rn(c1, g1); d2 = mk_fsub_rn(c2, g2);
    return capped;
}

// MODE 1: the reference's search over the triclinic vectors, which sits inside its loop over the axes
MK_DEV void wrap_cell_search(const WrapCellFrame* __restrict__ r, double& x, double& y, double& z)
{
    const double max_cutoff2 = r->max_cutoff2;
    double d2min = wc_norm2(x, y, z);
    if (!(d2min > max_cutoff2)) return;
    const double sx = x, sy = y, sz = z;
    const int n = r->ntric;
    for (int k = 0; d2min > max_cutoff2 && k < n; ++k) {
        const double tx = mk_dadd_rn(sx, r->tric[k][0]), ty = mk_dadd_rn(sy, r->tric[k][1]), tz = mk_dadd_rn(sz, r->tric[k][2]);
        const double d2 = wc_norm2(tx, ty, tz);
        if (d2 < d2min) { x = tx; y = ty; z = tz; d2min = d2; }
    }
}

// MODE 0, 1: the reference's pbc_dx of the group centre against box_middle.  Returns whether a loop hit the cap.
template <int MODE>
MK_DEV bool wrap_cell_pbc_dx(const WrapCellFrame* __restrict__ r, float c0, float c1, float c2, double& x, double& y, double& z)
{
    x = (double)mk_fsub_rn(c0, r->bm[0]); y = (double)mk_fsub_rn(c1, r->bm[1]); z = (double)mk_fsub_rn(c2, r->bm[2]);
    const double h0 = r->hbox[0], h1 = r->hbox[1], h2 = r->hbox[2];
    const double b00 = r->b00, b11 = r->b11, b22 = r->b22;
    bool capped = false;
    int steps;
    if constexpr (MODE == WRAP_CELL_RECTANGULAR) {
        for (steps = 0; x > h0; ++steps) { if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; } x = wc_dsub(x, b00); }
        for (steps = 0; x <= -h0; ++steps) { if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; } x = mk_dadd_rn(x, b00); }
        for (steps = 0; y > h1; ++steps) { if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; } y = wc_dsub(y, b11); }
        for (steps = 0; y <= -h1; ++steps) { if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; } y = mk_dadd_rn(y, b11); }
        for (steps = 0; z > h2; ++steps) { if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; } z = wc_dsub(z, b22); }
        for (steps = 0; z <= -h2; ++steps) { if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; } z = mk_dadd_rn(z, b22); }
    } else {
        const double b10 = r->b10, b20 = r->b20, b21 = r->b21;
        // i = 2 (j = 2, 1, 0)
        for (steps = 0; z > h2; ++steps) {
            if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; }
            z = wc_dsub(z, b22); y = wc_dsub(y, b21); x = wc_dsub(x, b20);
        }
        for (steps = 0; z <= -h2; ++steps) {
            if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; }
            z = mk_dadd_rn(z, b22); y = mk_dadd_rn(y, b21); x = mk_dadd_rn(x, b20);
        }
        wrap_cell_search(r, x, y, z);
        // i = 1
        for (steps = 0; y > h1; ++steps) {
            if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; }
            y = wc_dsub(y, b11); x = wc_dsub(x, b10);
        }
        for (steps = 0; y <= -h1; ++steps) {
            if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; }
            y = mk_dadd_rn(y, b11); x = mk_dadd_rn(x, b10);
        }
        wrap_cell_search(r, x, y, z);
        // i = 0
        for (steps = 0; x > h0; ++steps) { if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; } x = wc_dsub(x, b00); }
        for (steps = 0; x <= -h0; ++steps) { if (steps == WRAP_CELL_MAX_STEPS) { capped = true; break; } x = mk_dadd_rn(x, b00); }
        wrap_cell_search(r, x, y, z);
    }
    return capped;
}

// one recentred coordinate xc of a group, wrapped.  MODE 2: xc - delta; MODE 0, 1: float(double((xc - gc) + bm) + dx)
template <int MODE>
MK_DEV float wrap_cell_apply(float xc, float delta, float gc, float bm, double dx)
{
    if constexpr (MODE == WRAP_CELL_TRICLINIC) return mk_fsub_rn(xc, delta);
    else return (float)mk_dadd_rn((double)mk_fadd_rn(mk_fsub_rn(xc, gc), bm), dx);
}

// Item i: frame i / G, group i % G.  out == xyz: in place.
template <int MODE>
MK_KERNEL(WRAP_BLOCK) void k_wrap_cell_lanes(const float* xyz, long long n_atoms, const WrapCellFrame* __restrict__ recs, long long F,
                                             const unsigned* __restrict__ starts, long long G, int small_max,
                                             const float* __restrict__ centre, float cx, float cy, float cz, float* out, int* status)
{
    const long long item = (long long)blockIdx.x * WRAP_BLOCK + threadIdx.x;
    if (item >= F * G) return;
    const long long f = item / G, g = item - f * G;
    long long b = starts[g], e = starts[g + 1];
    b = b < n_atoms ? b : n_atoms;
    e = e < n_atoms ? e : n_atoms;
    const int n = (int)(e - b);
    if (n <= 0 || e - b > small_max) return;
    const size_t base = ((size_t)f * (size_t)n_atoms + (size_t)b) * 3;
    const float* p = xyz + base;                                          // (no __restrict__: out may be xyz)
    float* o = out + base;
    const WrapCellFrame* r = recs + f;
    if (r->flag) {
        if (status) status[WRAP_CELL_ST_FRAME] = 1;
        if (out != xyz)
            for (int k = 0; k < 3 * n; ++k) o[k] = p[k];
        return;
    }
    const float w0 = wrap_box_centre(centre, f, 0, cx, cy, cz), w1 = wrap_box_centre(centre, f, 1, cx, cy, cz),
                w2 = wrap_box_centre(centre, f, 2, cx, cy, cz);
    const float m0 = r->bm[0], m1 = r->bm[1], m2 = r->bm[2];
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    for (int k = 0; k < n; ++k) {
        const float d = (float)(k + 1);
        c0 = wrap_mean_step(c0, wc_recentre(p[3 * k], w0, m0), d);
        c1 = wrap_mean_step(c1, wc_recentre(p[3 * k + 1], w1, m1), d);
        c2 = wrap_mean_step(c2, wc_recentre(p[3 * k + 2], w2, m2), d);
    }
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    bool capped;
    if constexpr (MODE == WRAP_CELL_TRICLINIC) capped = wrap_cell_triclinic(r, c0, c1, c2, d0, d1, d2);
    else capped = wrap_cell_pbc_dx<MODE>(r, c0, c1, c2, x0, x1, x2);
    if (capped && status) status[WRAP_CELL_ST_CAP] = 1;
    for (int k = 0; k < n; ++k) {
        const float x = wc_recentre(p[3 * k], w0, m0), y = wc_recentre(p[3 * k + 1], w1, m1), z = wc_recentre(p[3 * k + 2], w2, m2);
        o[3 * k] = wrap_cell_apply<MODE>(x, d0, c0, m0, x0);
        o[3 * k + 1] = wrap_cell_apply<MODE>(y, d1, c1, m1, x1);
        o[3 * k + 2] = wrap_cell_apply<MODE>(z, d2, c2, m2, x2);
    }
}

MK_DEV double wc_readlane_f64(double v, int lane)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = mk_readlane((unsigned)u, lane), hi = mk_readlane((unsigned)(u >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
MK_DEV float wc_pick(int axis, float a, float b, float c) { return axis == 0 ? a : axis == 1 ? b : c; }
MK_DEV double wc_pick(int axis, double a, double b, double c) { return axis == 0 ? a : axis == 1 ? b : c; }

// Block i (one wave): frame i / n_list, group list[i % n_list]; groups of at most small_max atoms are k_wrap_cell_lanes' and skipped.
template <int MODE>
MK_KERNEL(64) void k_wrap_cell_waves(const float* xyz, long long n_atoms, const WrapCellFrame* __restrict__ recs, long long F,
                                     const unsigned* __restrict__ starts, long long G, const unsigned* __restrict__ list, long long n_list,
                                     int small_max, const float* __restrict__ centre, float cx, float cy, float cz, float* out, int* status)
{
    __shared__ float lds[3 * WRAP_CHUNK];
    const long long i = blockIdx.x;
    const long long f = i / n_list;
    const long long g = list[i - f * n_list];
    const int lane = (int)threadIdx.x;
    if (g >= G) return;                                                   // (wave-uniform, as every return below)
    long long b = starts[g], e = starts[g + 1];
    b = b < n_atoms ? b : n_atoms;
    e = e < n_atoms ? e : n_atoms;
    const long long n = e - b;
    if (n <= small_max) return;
    const float* p = xyz + ((size_t)f * (size_t)n_atoms + (size_t)b) * 3;
    float* o = out + ((size_t)f * (size_t)n_atoms + (size_t)b) * 3;
    const WrapCellFrame* r = recs + f;
    if (r->flag) {
        if (status && lane == 0) status[WRAP_CELL_ST_FRAME] = 1;
        if (out != xyz)
            for (long long k = lane; k < 3 * n; k += WAVE) o[k] = p[k];
        return;
    }
    const float w0 = wrap_box_centre(centre, f, 0, cx, cy, cz), w1 = wrap_box_centre(centre, f, 1, cx, cy, cz),
                w2 = wrap_box_centre(centre, f, 2, cx, cy, cz);
    const float m0 = r->bm[0], m1 = r->bm[1], m2 = r->bm[2];
    // the chains: chunk by chunk through LDS, recentred on the way in
    float c = 0.0f;
    for (long long k0 = 0; k0 < n; k0 += WRAP_CHUNK) {
        const int m = (int)(n - k0 < WRAP_CHUNK ? n - k0 : WRAP_CHUNK);
        const float* q = p + 3 * (size_t)k0;
        int axis = lane % 3;                                              // of float t = lane + 64 j: (lane + j) % 3, as 64 % 3 == 1
        for (int t = lane; t < 3 * m; t += WAVE) {
            lds[t] = wc_recentre(q[t], wc_pick(axis, w0, w1, w2), wc_pick(axis, m0, m1, m2));
            axis = axis == 2 ? 0 : axis + 1;
        }
        mk_wave_sync();
        if (lane < 3)
            for (int k = 0; k < m; ++k) c = wrap_mean_step(c, lds[3 * k + lane], (float)(k0 + k + 1));
        mk_wave_sync();
    }
    const float c0 = mk_uint_as_float(mk_readlane(mk_float_bits(c), 0)), c1 = mk_uint_as_float(mk_readlane(mk_float_bits(c), 1)),
                c2 = mk_uint_as_float(mk_readlane(mk_float_bits(c), 2));
    // one lane decides: the axes are coupled
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (lane == 0) {
        bool capped;
        if constexpr (MODE == WRAP_CELL_TRICLINIC) capped = wrap_cell_triclinic(r, c0, c1, c2, d0, d1, d2);
        else capped = wrap_cell_pbc_dx<MODE>(r, c0, c1, c2, x0, x1, x2);
        if (capped && status) status[WRAP_CELL_ST_CAP] = 1;
    }
    if constexpr (MODE == WRAP_CELL_TRICLINIC) {
        d0 = mk_uint_as_float(mk_readlane(mk_float_bits(d0), 0));
        d1 = mk_uint_as_float(mk_readlane(mk_float_bits(d1), 0));
        d2 = mk_uint_as_float(mk_readlane(mk_float_bits(d2), 0));
    } else {
        x0 = wc_readlane_f64(x0, 0); x1 = wc_readlane_f64(x1, 0); x2 = wc_readlane_f64(x2, 0);
    }
    int axis = lane % 3;
    for (long long k = lane; k < 3 * n; k += WAVE) {
        const float bm = wc_pick(axis, m0, m1, m2);
        const float xc = wc_recentre(p[k], wc_pick(axis, w0, w1, w2), bm);
        o[k] = wrap_cell_apply<MODE>(xc, wc_pick(axis, d0, d1, d2), wc_pick(axis, c0, c1, c2), bm, wc_pick(axis, x0, x1, x2));
        axis = axis == 2 ? 0 : axis + 1;
    }
}

}  // namespace mkamd
