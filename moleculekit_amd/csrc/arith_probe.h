// arith_probe.h -- the device arithmetic under the bit-exact kernels, one elementwise kernel per operation (mkamd_selftest_arith).
//
// Every promise of bit-equality with the reference (distances, SASA, shell counts, dihedral terms, wrap, ring interactions, hydrogen
// bonds) rests on a few dozen small device functions: the never-contracted float32 / float64 operations of mk_device.h, its division
// and its root, the float64 detour of ring_kernels.h, the roundings, and the composites built from them (the restated acosf, the
// reciprocal shortcut of the minimum image, the wrap's decision).  The kernels reach them on a few thousand ordinary numbers per test;
// here each one is applied to arrays the caller chooses -- denormals, ties, the edges of every branch -- and the result goes back as it
// is, to be compared with an independent reference bit for bit (tests/arith_cases.py, tests/test_gpu_arith.py; the same source on the
// host emulation: tests/test_arith_cpu.py).
//
// A probe kernel CALLS the product's own function, never a copy of its body; where a kernel writes an expression inline
// (roundf(ring_div(val, b)) in ring_wdist2, __builtin_round of the widened quotient in wrap_decide) the probe writes the same expression
// here, in the translation unit of the kernels.  Element i is lane i % 64 of its wave: mk_fsqrt_rn's ballot sees the 64 consecutive
// elements of a run, and the lanes past n have left the kernel before it (they are not in the wave's execution mask).
#pragma once
#include "ring_kernels.h"
#include "dihedral_kernels.h"
#include "wrap_cell_kernels.h"

namespace mkamd {

enum {
    AP_FADD = 0,        // mk_fadd_rn(a, b)                                           f32 f32     -> f32
    AP_FSUB = 1,        // mk_fsub_rn(a, b)
    AP_FMUL = 2,        // mk_fmul_rn(a, b)
    AP_FMUL_ADD = 3,    // mk_fadd_rn(mk_fmul_rn(a, b), c)                            f32 f32 f32 -> f32
    AP_DMUL_ADD = 4,    // mk_dadd_rn(mk_dmul_rn(a, b), c)                            f64 f64 f64 -> f64
    AP_FDIV = 5,        // mk_fdiv_rn(a, b)
    AP_RING_DIV = 6,    // ring_div(a, b)
    AP_DDIV = 7,        // wc_ddiv(a, b): the float64 division of wrap_cell_kernels.h f64 f64     -> f64
    AP_FSQRT = 8,       // mk_fsqrt_rn(a): the whole function, ballot included        f32         -> f32
    AP_RING_SQRT = 9,   // ring_sqrt(a)
    AP_ROUNDF = 10,     // roundf(a)
    AP_RINT = 11,       // mk_rint(a)
    AP_DROUND = 12,     // __builtin_round((double)a)                                 f32         -> f64
    AP_ROUND_QUOT = 13, // round_quotient_exact(a, b)
    AP_MIN_IMAGE = 14,  // dist2_min_image_f32(a, 0, 0, 0, 0, 0, b, 1, 1, mk_fdiv_rn(1, b), 1, 1, true)
    AP_WRAP_DECIDE = 15,// wrap_decide(a, b, c) -> (moved ? 1 : 0, translation)       f32 f32 f32 -> 2 x f32
    AP_DIH_WRAP = 16,   // dih_wrap(a, b)
    AP_ACOSF = 17,      // ring_acosf(a)
    AP_RING_ANGLE = 18, // ring_angle(a)                                              f32         -> f64
    AP_RING_ROUND_QUOT = 19,   // roundf(ring_div(a, b)): the image integer of ring_wdist2 / hbond_wvec
    AP_MIN_IMAGE_PK = 20,      // dist2_pk<true> of the separations (a, -a) in a box b, reciprocal mk_fdiv_rn(1, b): the two d^2, then 1
                               // where the accumulated test sends the caller to dist2_min_image_f32 (else 0)  f32 f32 -> 3 x f32
    AP_NOPS = 21
};

// inputs an operation reads (1..3)
constexpr int arith_probe_arity(int op)
{
    return (op == AP_FMUL_ADD || op == AP_DMUL_ADD || op == AP_WRAP_DECIDE) ? 3
         : (op == AP_FSQRT || op == AP_RING_SQRT || op == AP_ROUNDF || op == AP_RINT || op == AP_DROUND || op == AP_ACOSF || op == AP_RING_ANGLE) ? 1
         : 2;
}

constexpr int AP_THREADS = 256;

template <int OP>
MK_KERNEL(AP_THREADS) void k_arith_probe(long long n, const void* __restrict__ pa, const void* __restrict__ pb, const void* __restrict__ pc,
                                         void* __restrict__ pout)
{
    const long long i = (long long)blockIdx.x * AP_THREADS + (long long)threadIdx.x;
    if (i >= n) return;
    if constexpr (OP == AP_DMUL_ADD || OP == AP_DDIV) {
        const double a = static_cast<const double*>(pa)[i], b = static_cast<const double*>(pb)[i];
        double* out = static_cast<double*>(pout);
        if constexpr (OP == AP_DMUL_ADD) out[i] = mk_dadd_rn(mk_dmul_rn(a, b), static_cast<const double*>(pc)[i]);
        else out[i] = wc_ddiv(a, b);
    } else {
        constexpr int arity = arith_probe_arity(OP);
        const float a = static_cast<const float*>(pa)[i];
        const float b = arity >= 2 ? static_cast<const float*>(pb)[i] : 0.0f;
        const float c = arity >= 3 ? static_cast<const float*>(pc)[i] : 0.0f;
        float* out = static_cast<float*>(pout);
        double* out64 = static_cast<double*>(pout);
        if constexpr (OP == AP_FADD) out[i] = mk_fadd_rn(a, b);
        else if constexpr (OP == AP_FSUB) out[i] = mk_fsub_rn(a, b);
        else if constexpr (OP == AP_FMUL) out[i] = mk_fmul_rn(a, b);
        else if constexpr (OP == AP_FMUL_ADD) out[i] = mk_fadd_rn(mk_fmul_rn(a, b), c);
        else if constexpr (OP == AP_FDIV) out[i] = mk_fdiv_rn(a, b);
        else if constexpr (OP == AP_RING_DIV) out[i] = ring_div(a, b);
        else if constexpr (OP == AP_FSQRT) out[i] = mk_fsqrt_rn(a);
        else if constexpr (OP == AP_RING_SQRT) out[i] = ring_sqrt(a);
        else if constexpr (OP == AP_ROUNDF) out[i] = roundf(a);
        else if constexpr (OP == AP_RINT) out[i] = mk_rint(a);
        else if constexpr (OP == AP_DROUND) out64[i] = __builtin_round((double)a);
        else if constexpr (OP == AP_ROUND_QUOT) out[i] = round_quotient_exact(a, b);
        else if constexpr (OP == AP_RING_ROUND_QUOT) out[i] = roundf(ring_div(a, b));
        else if constexpr (OP == AP_MIN_IMAGE)
            out[i] = dist2_min_image_f32(a, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, b, 1.0f, 1.0f, mk_fdiv_rn(1.0f, b), 1.0f, 1.0f, true);
        else if constexpr (OP == AP_WRAP_DECIDE) {
            float t;
            const bool moved = wrap_decide(a, b, c, t);
            out[2 * i] = moved ? 1.0f : 0.0f;
            out[2 * i + 1] = t;
        }
        else if constexpr (OP == AP_MIN_IMAGE_PK) {
            float risk = 0.0f;
            const mk_f2 z = mk_f2_splat(0.0f);
            const mk_f2 d2 = dist2_pk<true>(mk_f2{a, -a}, z, z, 0.0f, 0.0f, 0.0f, b, 1.0f, 1.0f, mk_fdiv_rn(1.0f, b), 1.0f, 1.0f, risk);
            out[3 * i] = d2[0];
            out[3 * i + 1] = d2[1];
            out[3 * i + 2] = !(risk < DRC_RISK) ? 1.0f : 0.0f;
        }
        else if constexpr (OP == AP_DIH_WRAP) out[i] = dih_wrap(a, b);
        else if constexpr (OP == AP_ACOSF) out[i] = ring_acosf(a);
        else if constexpr (OP == AP_RING_ANGLE) out64[i] = ring_angle(a);
    }
}

template <int OP, class BE>
int arith_probe_launch(BE& be, long long n, const void* a, const void* b, const void* c, void* out)
{
    return be.launch(k_arith_probe<OP>, dim3((unsigned)((n + AP_THREADS - 1) / AP_THREADS)), dim3(AP_THREADS), n, a, b, c, out);
}

// n elements of operation `op` on the backend's stream; 0, or MKAMD_EINVAL's value 1 with a message
template <class BE>
int run_arith_probe(BE& be, int op, long long n, const void* a, const void* b, const void* c, void* out, const char*& err)
{
    err = nullptr;
    if (op < 0 || op >= AP_NOPS) { err = "arithmetic probe: unknown operation"; return 1; }
    if (n < 0 || n > 0x7fffffffLL * 64) { err = "arithmetic probe: element count out of range"; return 1; }
    if (n == 0) return 0;
    const int arity = arith_probe_arity(op);
    if (!a || !out || (arity >= 2 && !b) || (arity >= 3 && !c)) { err = "arithmetic probe: an operand or the result pointer is NULL"; return 1; }
    switch (op) {
#define MK_AP_CASE(OP) case OP: return arith_probe_launch<OP>(be, n, a, b, c, out);
        MK_AP_CASE(AP_FADD) MK_AP_CASE(AP_FSUB) MK_AP_CASE(AP_FMUL) MK_AP_CASE(AP_FMUL_ADD) MK_AP_CASE(AP_DMUL_ADD) MK_AP_CASE(AP_FDIV)
        MK_AP_CASE(AP_RING_DIV) MK_AP_CASE(AP_DDIV) MK_AP_CASE(AP_FSQRT) MK_AP_CASE(AP_RING_SQRT) MK_AP_CASE(AP_ROUNDF) MK_AP_CASE(AP_RINT)
        MK_AP_CASE(AP_DROUND) MK_AP_CASE(AP_ROUND_QUOT) MK_AP_CASE(AP_MIN_IMAGE) MK_AP_CASE(AP_WRAP_DECIDE) MK_AP_CASE(AP_DIH_WRAP)
        MK_AP_CASE(AP_ACOSF) MK_AP_CASE(AP_RING_ANGLE) MK_AP_CASE(AP_RING_ROUND_QUOT) MK_AP_CASE(AP_MIN_IMAGE_PK)
#undef MK_AP_CASE
    }
    return 1;
}

}  // namespace mkamd
