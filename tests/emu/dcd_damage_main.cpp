// tests/emu/dcd_damage_main.cpp -- TEST INFRASTRUCTURE ONLY.
// The host side of the DCD path (moleculekit_amd/csrc/dcd_reader.h: header parser, frame descriptors, the host read loop) on damaged
// files, in a program of its own so that it can be built with AddressSanitizer and UBSan (tests/emu_dcd_build.py) and run as a child
// process.  Every file is parsed out of a heap copy of exactly its size, whose ends the sanitizer guards: a read past the bytes aborts.
//
//   dcd_damage_main file <path>...   one line per file: "<path> status=<0|1> frames=<n> msg=<message>"
//   dcd_damage_main truncate <path>  the file cut to every length 0 .. size: "len=<n> status=<0|1> frames=<n>"
#include "../../moleculekit_amd/csrc/dcd_reader.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

using namespace mkamd;

// everything the host path does with a file: header, descriptors of all frames, all frames and atoms read
static int run(const uint8_t* p, size_t n, long long& frames, std::string& err)
{
    dcd::Header h;
    frames = 0;
    if (dcd::parse_header(p, n, h, err)) return 1;
    frames = h.n_frames;
    std::vector<dcd::FrameDesc> desc((size_t)h.n_frames);
    std::vector<float> cell((size_t)h.n_frames * 6), xyz((size_t)h.n_frames * (size_t)h.n_atoms * 3);
    int64_t lo = 0, hi = 0;
    if (dcd::chunk_desc(p, n, h, nullptr, h.n_frames, desc.data(), &lo, &hi, cell.data(), err)) return 1;
    for (const dcd::FrameDesc& d : desc)
        if ((size_t)lo + d.z_off + 4ull * d.count > n) { err = "a descriptor reaches outside the file"; return 1; }
    if (dcd::read(p, n, h, nullptr, h.n_frames, nullptr, h.n_atoms, xyz.data(), cell.data(), err)) return 1;
    return 0;
}

static int on_copy(const std::vector<uint8_t>& all, size_t n, long long& frames, std::string& err)
{
    uint8_t* q = (uint8_t*)malloc(n ? n : 1);                   // exactly n bytes (one for an empty file: never read)
    if (n) memcpy(q, all.data(), n);
    const int st = run(q, n, frames, err);
    free(q);
    return st;
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: dcd_damage_main file <path>... | truncate <path>\n"); return 2; }
    const std::string mode = argv[1];
    for (int a = 2; a < argc; ++a) {
        std::ifstream in(argv[a], std::ios::binary);
        if (!in) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        const std::vector<uint8_t> all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        long long frames = 0;
        std::string err;
        if (mode == "truncate") {
            for (size_t n = 0; n <= all.size(); ++n) {
                err.clear();
                const int st = on_copy(all, n, frames, err);
                printf("len=%zu status=%d frames=%lld\n", n, st, frames);
            }
        } else {
            const int st = on_copy(all, all.size(), frames, err);
            printf("%s status=%d frames=%lld msg=%s\n", argv[a], st, frames, err.c_str());
        }
    }
    return 0;
}
