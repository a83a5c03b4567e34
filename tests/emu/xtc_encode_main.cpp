// tests/emu/xtc_encode_main.cpp -- TEST INFRASTRUCTURE ONLY: the device XTC writer's kernels under host sanitizers.
//
// A program of its own (tests/emu_xtc_encode_build.py compiles it with -fsanitize=address,undefined; tests/test_xtc_encode_cpu.py runs
// it as a child process; it is never loaded into an interpreter).  It includes the product's kernels (csrc/xtc_encode.h, on the SIMT
// emulation of emu_device.h, launched by the product's own launch plan) and runs them on case files the test writes: the named
// trajectories and the hostile inputs.  Every buffer the kernels touch is a heap block of exactly the size the two size functions
// promise, poisoned, so that an access one byte outside it is a sanitizer report.
//
// A case file (little-endian): int64 F, N; float in_scale; float precision[F], box[F * 9], time[F]; int32 step[F]; float xyz[F * N * 3];
// int32 status[F] expected; int64 n; the n bytes of the expected image.  Per case it asserts the statuses, the image up to the last
// record's end, and that nothing behind it was written (exit status 1 with the case's name; a sanitizer report ends the program too).
#include "emu_xtc_encode.cpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

static const unsigned char POISON = 0xCD;

template <class T>
static std::unique_ptr<T[]> take(FILE* f, size_t n, const char* path)
{
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    if (n && fread(p.get(), sizeof(T), n, f) != n) { fprintf(stderr, "xtc_encode_main: %s is cut short\n", path); exit(2); }
    return p;
}

static int run_case(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "xtc_encode_main: cannot open %s\n", path); exit(2); }
    const auto dims = take<long long>(f, 2, path);
    const long long F = dims[0], N = dims[1];
    const auto scale = take<float>(f, 1, path);
    const auto precision = take<float>(f, (size_t)F, path), box = take<float>(f, (size_t)F * 9, path), time = take<float>(f, (size_t)F, path);
    const auto step = take<int>(f, (size_t)F, path);
    const auto xyz = take<float>(f, (size_t)(F * N * 3), path);
    const auto want_status = take<int>(f, (size_t)F, path);
    const auto want_n = take<long long>(f, 1, path);
    const auto want = take<unsigned char>(f, (size_t)want_n[0], path);
    fclose(f);

    const uint64_t bound = emu_xtc_encode_bound(F, N), wb = emu_xtc_encode_work_bytes(F, N);
    std::unique_ptr<uint32_t[]> image(new uint32_t[bound / 4]);            // (the bound is a whole number of words)
    std::unique_ptr<uint64_t[]> work(new uint64_t[wb / 8]), offsets(new uint64_t[(size_t)F + 1]);
    std::unique_ptr<int[]> status(new int[(size_t)F]);
    if (bound % 4 || wb % 8) { fprintf(stderr, "xtc_encode_main: %s: sizes are not whole words\n", path); return 1; }
    memset(image.get(), POISON, bound);
    memset(work.get(), POISON, wb);
    memset(offsets.get(), POISON, 8 * ((size_t)F + 1));
    memset(status.get(), POISON, 4 * (size_t)F);
    unsigned char* img = reinterpret_cast<unsigned char*>(image.get());
    const int st = emu_xtc_encode(xyz.get(), scale[0], precision.get(), box.get(), time.get(), step.get(), F, N, img, bound, offsets.get(), status.get(),
                                  reinterpret_cast<unsigned char*>(work.get()), wb);
    if (st) { fprintf(stderr, "xtc_encode_main: %s: the call returned %d\n", path, st); return 1; }
    for (long long k = 0; k < F; ++k)
        if (status[(size_t)k] != want_status[(size_t)k]) { fprintf(stderr, "xtc_encode_main: %s: frame %lld has status %d, expected %d\n", path, k, status[(size_t)k], want_status[(size_t)k]); return 1; }
    for (long long k = 0; k < F; ++k)
        if (offsets[(size_t)k] > offsets[(size_t)k + 1] || (status[(size_t)k] && offsets[(size_t)k] != offsets[(size_t)k + 1])) { fprintf(stderr, "xtc_encode_main: %s: offsets out of order at frame %lld\n", path, k); return 1; }
    const uint64_t total = offsets[(size_t)F];
    if (total != (uint64_t)want_n[0] || total > bound || memcmp(img, want.get(), (size_t)total) != 0) { fprintf(stderr, "xtc_encode_main: %s: the image differs from the expected bytes (%llu bytes, expected %lld)\n", path, (unsigned long long)total, want_n[0]); return 1; }
    for (uint64_t k = total; k < bound; ++k)
        if (img[k] != POISON) { fprintf(stderr, "xtc_encode_main: %s: byte %llu behind the last record was written\n", path, (unsigned long long)k); return 1; }
    // the size checks of the call: one byte short on either buffer is refused before anything runs
    if (emu_xtc_encode(xyz.get(), scale[0], precision.get(), box.get(), time.get(), step.get(), F, N, img, bound - 1, offsets.get(), status.get(), reinterpret_cast<unsigned char*>(work.get()), wb) == 0 ||
        emu_xtc_encode(xyz.get(), scale[0], precision.get(), box.get(), time.get(), step.get(), F, N, img, bound, offsets.get(), status.get(), reinterpret_cast<unsigned char*>(work.get()), wb - 1) == 0) {
        fprintf(stderr, "xtc_encode_main: %s: a buffer one byte short is accepted\n", path);
        return 1;
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: xtc_encode_main case.bin ...\n"); return 2; }
    int bad = 0;
    for (int i = 1; i < argc; ++i) bad += run_case(argv[i]);
    printf("{\"cases\": %d, \"failed\": %d}\n", argc - 1, bad);
    return bad ? 1 : 0;
}
