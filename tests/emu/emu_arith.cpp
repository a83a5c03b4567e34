// tests/emu/emu_arith.cpp -- TEST INFRASTRUCTURE ONLY.
// The arithmetic probe kernels (moleculekit_amd/csrc/arith_probe.h) on the host SIMT emulation of emu_device.h: the product's kernel
// source, with the emulator's replacements of the device primitives (the host's a / b, sqrtf, nearbyintf).  Built into
// tests/emu/libmkamd_emu_arith.so by tests/emu_arith_build.py (-ffp-contract=off).
#include "emu_device.h"
#include "../../moleculekit_amd/csrc/arith_probe.h"

#include <cmath>
#include <string>

using namespace mkamd;

namespace {

struct ArithEmuBackend {
    template <class... KA, class... A>
    int launch(void (*kernel)(KA...), dim3 grid, dim3 block, A... args)
    {
        emu::launch(kernel, grid, block, args...);
        return 0;
    }
};

thread_local std::string g_err;

}  // namespace

extern "C" {

const char* emu_arith_last_error() { return g_err.c_str(); }
int emu_arith_nops() { return AP_NOPS; }
int emu_arith_arity(int op) { return arith_probe_arity(op); }

int emu_arith_probe(int op, long long n, const void* a, const void* b, const void* c, void* out)
{
    ArithEmuBackend be;
    const char* err = nullptr;
    const int st = run_arith_probe(be, op, n, a, b, c, out, err);
    g_err = err ? err : "";
    return st;
}

// the host C library's own acosf, elementwise (compared with the restatement where the library is the goldens' glibc)
void emu_arith_libm_acosf(long long n, const float* x, float* out)
{
    for (long long i = 0; i < n; ++i) out[i] = acosf(x[i]);
}

}  // extern "C"
