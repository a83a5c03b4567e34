// tests/emu/xtc_damage_main.cpp -- TEST INFRASTRUCTURE ONLY: both XTC decoders on DAMAGED files, under host sanitizers.
//
// A program of its own (tests/emu_xtc_damage_build.py compiles it with -fsanitize=address,undefined and runs it as a child process;
// it is never loaded into an interpreter).  It includes the product's sources -- the host decoder (csrc/xtc_reader.h), the header
// parser (csrc/xtc_headers.h) and the device decoder's two kernels (csrc/xtc_gpu.h, on the SIMT emulation of emu_device.h, launched as
// emu_capi.cpp::emu_xtc_decode launches them) -- and runs them on committed fixtures that it damages itself: header fields, cut
// files, flipped stream bits, runs of garbage (the table is `make_damages`; everything is derived from the fixture and from seeds
// written there).  One frame of a file is damaged at a time; its neighbours are the control.
//
// Every buffer a decoder touches is a heap block of exactly the contracted size, so that an access one byte outside it is a
// sanitizer report: the file (a view: xtc::Mapped::view), the device byte buffer (hi - lo + XTC_PAD), the group records
// (frames * (atoms + XS_SPEC)), the output (frames * atoms * 3 floats), status / ngroups / desc (one entry per frame).
//
// Per case it asserts (exit status 1 with the case printed; a sanitizer report ends the program as well):
//   * the host decoder and the parser return an error or decode; the device path gives status 0 / 1 / 2 and 2 only where the
//     documented limits say so (a number of > 64 bits, a run at smallidx > 64); ngroups is 0 and the output untouched for a refusal
//   * undamaged frames of the same call decode to the bits of the undamaged file in both decoders
//   * where both accept the damaged frame, the same bits; where the host refuses, the device does not return 0
//   * the verdict that follows from the damage (header smallidx outside the table, range 0, atom counts, nbytes past the file,
//     a cut inside the last record) is the verdict given
//   * a second run of the case gives the same bytes
// and it counts which refusal site of either decoder each case reached (MK_XTC_PROBE / MKAMD_XTC_REFUSE); the counts are printed as
// one JSON line, which tests/test_xtc_damage.py reads.
//
// Two views of a damaged file: "fresh" -- the frame index is built from the damaged bytes, as a first call on the file does; and
// "stale" (damages that keep the file's size only) -- the index of the undamaged file is used, as index_frames_cached hands it out
// when a file is rewritten in place within its timestamps' resolution.  Only the stale view reaches the nbytes checks of the parser
// and of decode_frame: a fresh index has already dropped a record whose nbytes passes the file's end.
#include <algorithm>
#include <cinttypes>
#include <map>
#include <set>
#include <string>

static void xtc_probe_dev(long long f, bool together, bool e_end, bool e_wide, bool more_atoms, bool more_bits, bool e_idx, int smallidx, int st);
static void xtc_probe_host(const char* site);
#define MK_XTC_PROBE(frame, together, e_end, e_wide, more_atoms, more_bits, e_idx, smallidx, status) \
    xtc_probe_dev(frame, together, e_end, e_wide, more_atoms, more_bits, e_idx, smallidx, status)
#define MKAMD_XTC_REFUSE(site) (xtc_probe_host(site), ::mkamd::xtc::E_FORMAT)

#include "emu_device.h"
#include "../../moleculekit_amd/csrc/xtc_gpu.h"
#include "../../moleculekit_amd/csrc/xtc_reader.h"
#include "../../moleculekit_amd/csrc/xtc_headers.h"

using namespace mkamd;

#ifndef DRIVER_PAD                       // (the mutation check of the pad's use overrides it; the product's value otherwise)
#define DRIVER_PAD XTC_PAD
#endif
#ifndef DRIVER_SPEC
#define DRIVER_SPEC XS_SPEC
#endif

// ---------------------------------------------------------------------------------------------------------------------------
// small tools
// ---------------------------------------------------------------------------------------------------------------------------
typedef std::vector<uint8_t> Bytes;

static uint64_t splitmix(uint64_t& s)
{
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static uint32_t crc32_of(const void* p, size_t n, uint32_t crc = 0)       // zlib's
{
    static uint32_t T[256];
    if (!T[1]) for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1; T[i] = c; }
    crc = ~crc;
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i) crc = T[(crc ^ b[i]) & 255] ^ (crc >> 8);
    return ~crc;
}

static void put_be32(Bytes& b, size_t off, uint32_t v) { b[off] = v >> 24; b[off + 1] = v >> 16; b[off + 2] = v >> 8; b[off + 3] = v; }
static uint32_t get_be32(const Bytes& b, size_t off) { return xtc::be32(b.data() + off); }

static std::string g_case;                                                  // what runs, for every message
[[noreturn]] static void die(const std::string& why)
{
    fprintf(stderr, "xtc_damage: FAILED: %s\n  case: %s\n", why.c_str(), g_case.c_str());
    exit(1);
}
#define CHECK(cond, why) do { if (!(cond)) die(std::string(why) + "  [" #cond "]"); } while (0)

// ---------------------------------------------------------------------------------------------------------------------------
// probes and reach
// ---------------------------------------------------------------------------------------------------------------------------
struct DevRefusal { const char* site = nullptr; bool together = false; };
static std::vector<DevRefusal> g_dev;                                       // per frame of the running launch
static std::string g_host_site;                                             // of the last host refusal
static std::map<std::string, long long> g_reach;                            // "site|damage kind" and "site" -> count
static std::string g_kind;

static void reach(const std::string& site) { ++g_reach[site]; ++g_reach[site + " | " + g_kind]; }

static void xtc_probe_dev(long long f, bool together, bool e_end, bool e_wide, bool more_atoms, bool more_bits, bool e_idx, int smallidx, int st)
{
    if (st == 0 || f < 0 || f >= (long long)g_dev.size()) return;
    g_dev[(size_t)f].site = e_end ? "dev: e_end" : e_wide ? "dev: e_wide" : more_atoms ? "dev: e_more, atom count" : more_bits ? "dev: e_more, next > tot"
                            : e_idx ? (smallidx < XTC_FIRST ? "dev: e_idx, below the table" : "dev: e_idx, above the table") : "dev: ?";
    g_dev[(size_t)f].together = together;
}
static void xtc_probe_host(const char* site) { g_host_site = site; }

// ---------------------------------------------------------------------------------------------------------------------------
// a fixture and what is known of it
// ---------------------------------------------------------------------------------------------------------------------------
struct Fixture {
    std::string name;
    Bytes bytes;
    int64_t natoms = 0;
    std::vector<size_t> offs;                                               // of its records (+ the file's size at the end)
    std::vector<std::vector<float>> frames;                                 // the host decoder's coordinates of the undamaged file [frame][atom * 3]
    std::vector<std::vector<XtcGroup>> groups;                              // the undamaged walk's records per frame (compressed frames)
    std::vector<XtcFrameDesc> desc;
    std::vector<int> dev0;                                                  // the device status of the undamaged frames (2: a file the device leaves to the host)
    bool compressed() const { return natoms > 9; }
    int F() const { return (int)frames.size(); }
};

// exactly n bytes on the heap
struct Heap {
    uint8_t* p;
    size_t n;
    explicit Heap(size_t n_) : p(new uint8_t[n_]), n(n_) {}
    Heap(const Heap&) = delete;
    ~Heap() { delete[] p; }
};

// ---------------------------------------------------------------------------------------------------------------------------
// one run of both decoders over a file's bytes and a selection
// ---------------------------------------------------------------------------------------------------------------------------
enum { V_OK = 0, V_REFUSED = 1, V_DROPPED = 2 };                             // host verdict per selected frame (dropped: not in the frame index)
struct Run {
    int index_status = 0;
    int64_t natoms = 0;
    size_t nframes = 0;                                                     // of the index
    std::vector<int> host;                                                  // per selected frame
    std::vector<std::string> host_site;
    std::vector<int> parser;                                                // per selected frame: 0 taken, 1 refused (alone), 2 dropped
    std::string parser_msg;                                                 // of the whole selection ("" = taken)
    std::vector<int> dev;                                                   // per selected frame: 0 / 1 / 2, -1 = did not get there
    std::vector<DevRefusal> dev_site;
    std::vector<uint32_t> crc_host, crc_dev;                                // of a frame's output bits (accepted frames)
    std::vector<std::vector<float>> xyz_host, xyz_dev;
    int read_status = 0;
    std::string read_err;
    uint32_t digest = 0;                                                    // of everything above: two runs are compared by it
};

static const uint32_t POISON = 0x7fa5a5a5u;                                 // (a NaN no decoder produces)
static inline uint32_t bits_of(const float& f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

static int parse(const uint8_t* base, size_t n, const xtc::FrameIndex& idx, const int64_t* sel, int64_t nsel, int64_t natoms, XtcFrameDesc* D,
                 int64_t* lo, int64_t* hi, std::string& msg)
{
    std::unique_ptr<float[]> box(new float[9 * (size_t)nsel]), time(new float[(size_t)nsel]);
    std::unique_ptr<int32_t[]> step(new int32_t[(size_t)nsel]);
    msg.clear();
    return xtc_parse_headers(base, 0, n, n, idx, sel, nsel, natoms, D, lo, hi, box.get(), time.get(), step.get(),
                             [&](const char* m) { msg = m; return 22; });
}

// stale: the frame index to use instead of the file's own (nullptr = fresh)
static Run run_file(const Bytes& file, const std::vector<int64_t>& sel_in, int64_t natoms_expected, const xtc::FrameIndex* stale)
{
    Run R;
    Heap buf(file.size());
    if (!file.empty()) memcpy(buf.p, file.data(), file.size());
    xtc::Mapped m;
    m.view(buf.p, buf.n);
    xtc::FrameIndex idx;
    if (stale) { idx.offs = stale->offs; idx.natoms = stale->natoms; }
    else {
        g_host_site.clear();
        R.index_status = xtc::index_frames(m, idx.offs, idx.natoms);
        CHECK(R.index_status == xtc::OK || R.index_status == xtc::E_FORMAT, "index_frames: neither OK nor an error of its own");
        if (R.index_status) { reach("host: " + g_host_site); idx.offs.clear(); }
    }
    R.natoms = idx.natoms;
    R.nframes = idx.offs.size();
    const size_t S = sel_in.size();
    R.host.assign(S, V_DROPPED); R.host_site.assign(S, ""); R.parser.assign(S, 2); R.dev.assign(S, -1); R.dev_site.assign(S, DevRefusal());
    R.crc_host.assign(S, 0); R.crc_dev.assign(S, 0); R.xyz_host.assign(S, {}); R.xyz_dev.assign(S, {});
    const int64_t N = idx.natoms;
    const bool whole_file_off = (N != natoms_expected) || N < 0 || N > (1ll << 22);       // (read() / chunk_desc refuse such a file as a whole)

    // ---- the host decoder, frame by frame, each into a block of exactly 3 N floats ----
    if (N >= 0 && N <= (1ll << 22))
        for (size_t j = 0; j < S; ++j) {
            if (sel_in[j] < 0 || (size_t)sel_in[j] >= R.nframes) continue;
            std::unique_ptr<float[]> c(new float[(size_t)N * 3 + 0]), box(new float[9]), t(new float[1]);
            std::unique_ptr<int32_t[]> st(new int32_t[1]);
            for (size_t i = 0; i < (size_t)N * 3; ++i) __builtin_memcpy(&c[i], &POISON, 4);
            g_host_site.clear();
            const int s = xtc::decode_frame(m, idx.offs[(size_t)sel_in[j]], N, 1, 0, c.get(), 1, 0, box.get(), t.get(), st.get());
            CHECK(s == xtc::OK || s == xtc::E_FORMAT, "decode_frame: neither OK nor E_FORMAT");
            R.host[j] = s == xtc::OK ? V_OK : V_REFUSED;
            if (s) { R.host_site[j] = g_host_site; reach("host: " + g_host_site); }
            else { R.xyz_host[j].assign(c.get(), c.get() + (size_t)N * 3); R.crc_host[j] = crc32_of(c.get(), (size_t)N * 12); }
        }
    // ---- xtc::read behind its open: the same verdict for the whole selection, the same bits ----
    {
        std::vector<int64_t> sel;
        for (size_t j = 0; j < S; ++j) if (R.host[j] != V_DROPPED) sel.push_back(sel_in[j]);
        const size_t K = sel.size();
        const size_t NN = (size_t)std::max<int64_t>(natoms_expected, 0);
        if (K && NN <= ((size_t)1 << 22)) {
            std::unique_ptr<float[]> c(new float[NN * 3 * K]), box(new float[9 * K]), t(new float[K]);
            std::unique_ptr<int32_t[]> st(new int32_t[K]);
            R.read_status = xtc::read_mapped(m, idx, sel.data(), (int64_t)K, natoms_expected, c.get(), box.get(), t.get(), st.get(), 1, R.read_err);
            bool all_ok = !whole_file_off;
            for (size_t j = 0; j < S; ++j) if (R.host[j] == V_REFUSED) all_ok = false;
            CHECK((R.read_status == xtc::OK) == all_ok, "xtc::read accepts a selection with a refused frame, or refuses one without");
            if (R.read_status) reach(std::string("host: read: ") + R.read_err);
            if (R.read_status == xtc::OK) {
                size_t k = 0;
                for (size_t j = 0; j < S; ++j) {
                    if (R.host[j] == V_DROPPED) continue;
                    for (size_t i = 0; i < NN * 3; ++i) if (bits_of(c[i * K + k]) != bits_of(R.xyz_host[j][i])) die("xtc::read and decode_frame differ");
                    ++k;
                }
            }
        }
    }
    // ---- the header parser: every selected frame alone, then the frames it takes together ----
    std::vector<int64_t> sel_dev;
    std::vector<size_t> slot;
    if (!whole_file_off) {
        for (size_t j = 0; j < S; ++j) {
            XtcFrameDesc d1;
            int64_t lo = 0, hi = 0;
            std::string msg;
            const int s = parse(buf.p, buf.n, idx, &sel_in[j], 1, N, &d1, &lo, &hi, msg);
            CHECK((s == 0) == msg.empty(), "parser: status and message disagree");
            if (s == 0) { R.parser[j] = 0; sel_dev.push_back(sel_in[j]); slot.push_back(j); continue; }
            R.parser[j] = msg == "frame index out of range" ? 2 : 1;
            CHECK((R.parser[j] == 2) == (R.host[j] == V_DROPPED), "parser: 'out of range' for an indexed frame, or not for a dropped one");
            CHECK(msg == "frame index out of range" || msg == "corrupt XTC frame", "parser: a message that no damaged file should draw: " + msg);
            if (R.parser[j] == 1) {
                // which of its three checks it was follows from the header's bytes
                const size_t r = idx.offs[(size_t)sel_in[j]];
                const char* site = "parser: range 0";
                if (xtc::be_i32(buf.p + r) != xtc::FRAME_MAGIC || xtc::be_i32(buf.p + r + 4) != N || xtc::be_i32(buf.p + r + 52) != N) site = "parser: magic or atom counts";
                else if (xtc::be_i32(buf.p + r + 88) < 0 || r + 92 + (size_t)xtc::be_i32(buf.p + r + 88) > buf.n) site = "parser: nbytes";
                reach(site);
                CHECK(R.host[j] == V_REFUSED, "the parser refuses a frame the host decoder takes");
            } else reach("parser: frame index out of range");
            if (R.parser_msg.empty()) R.parser_msg = msg;
        }
        {   // the whole selection in one call: refused with the first refused frame's message, taken if none is
            std::unique_ptr<XtcFrameDesc[]> Dall(new XtcFrameDesc[S]);
            int64_t lo = 0, hi = 0;
            std::string msg;
            const int s = S ? parse(buf.p, buf.n, idx, sel_in.data(), (int64_t)S, N, Dall.get(), &lo, &hi, msg) : 0;
            CHECK((s != 0) == !R.parser_msg.empty() && msg == R.parser_msg, "parser: the selection's verdict is not its first refused frame's");
        }
    }
    // ---- the device path over the frames the parser takes ----
    const size_t K = sel_dev.size();
    if (K) {
        std::unique_ptr<XtcFrameDesc[]> D(new XtcFrameDesc[K]);
        int64_t lo = 0, hi = 0;
        std::string msg;
        CHECK(parse(buf.p, buf.n, idx, sel_dev.data(), (int64_t)K, N, D.get(), &lo, &hi, msg) == 0, "parser refuses frames it took one by one: " + msg);
        CHECK(lo >= 0 && lo <= hi && (size_t)hi <= buf.n && lo % 4 == 0, "parser: byte range outside the file");
        Heap raw((size_t)(hi - lo) + DRIVER_PAD);
        memset(raw.p, 0, raw.n);
        memcpy(raw.p, buf.p + lo, (size_t)(hi - lo));
        const size_t NG = K * (size_t)(N + DRIVER_SPEC);
        std::unique_ptr<XtcGroup[]> groups(new XtcGroup[NG]);
        for (size_t i = 0; i < NG; ++i) groups[i] = XtcGroup{0xCDCDCDCDu, 0xCDCDCDCDu};
        std::unique_ptr<int[]> ngroups(new int[K]), status(new int[K]);
        for (size_t i = 0; i < K; ++i) { ngroups[i] = -7; status[i] = -7; }
        const size_t NO = K * (size_t)N * 3;
        std::unique_ptr<float[]> out(new float[NO]);
        for (size_t i = 0; i < NO; ++i) __builtin_memcpy(&out[i], &POISON, 4);
        g_dev.assign(K, DevRefusal());
        emu::launch(k_xtc_scan, dim3((unsigned)((K + 63) / 64)), dim3(64), (const unsigned char*)raw.p, (const XtcFrameDesc*)D.get(), (long long)K,
                    (long long)N, 1.0f, out.get(), groups.get(), ngroups.get(), status.get());
        const long long bpf = (N + 255) / 256;
        if (N < (1ll << 21) && bpf)
            emu::launch(k_xtc_expand, dim3((unsigned)(K * bpf)), dim3(256), (const unsigned char*)raw.p, (const XtcFrameDesc*)D.get(), 0ll, (long long)N,
                        1.0f, out.get(), (const XtcGroup*)groups.get(), (const int*)ngroups.get(), (int)bpf);
        for (size_t k = 0; k < K; ++k) {
            const size_t j = slot[k];
            const int st = status[k];
            const XtcFrameDesc& d = D[k];
            CHECK(st == 0 || st == 1 || st == 2, "device status is none of 0, 1, 2");
            R.dev[j] = st;
            const float* o = out.get() + k * (size_t)N * 3;
            if (st) {
                CHECK(ngroups[k] == 0, "ngroups of a refused frame is not 0");
                for (size_t i = 0; i < (size_t)N * 3; ++i) if (bits_of(o[i]) != POISON) die("a refused frame's output was written");
                const bool hdr_limit = d.triple_bits > 64 || N >= (1ll << 21) || d.nbytes >= (1u << 29) - 4u;
                const bool hdr_idx = !hdr_limit && (d.smallidx < XTC_FIRST || d.smallidx >= XTC_NMAGIC);
                DevRefusal site = g_dev[k];
                if (hdr_limit) site.site = "dev: size limits";
                else if (hdr_idx) site.site = "dev: header smallidx";
                CHECK(site.site != nullptr, "a refusal that no site reported");
                CHECK((st == 2) == (hdr_limit || std::string(site.site) == "dev: e_wide"), "status 2 outside the documented limits, or 1 inside them");
                R.dev_site[j] = site;
                reach(site.site);
                if (site.together) reach("dev: refusal while the wave looked at groups together");
            } else {
                CHECK(d.raw || ngroups[k] > 0, "an accepted frame without groups");
                for (size_t i = 0; i < (size_t)N * 3; ++i) if (bits_of(o[i]) == POISON) die("an accepted frame's output has a value nobody wrote");
                R.xyz_dev[j].assign(o, o + (size_t)N * 3);
                R.crc_dev[j] = crc32_of(o, (size_t)N * 12);
            }
        }
        // a refusal in a wave whose other lanes walked their frames to the end
        for (size_t k = 0; k < K; ++k)
            if (status[k] && g_dev[k].site) {
                bool other = false;
                for (size_t k2 = k / 64 * 64; k2 < std::min(K, k / 64 * 64 + 64); ++k2) other |= status[k2] == 0 && !D[k2].raw;
                if (other) reach("dev: refusal in a wave with live lanes");
            }
    }
    // ---- the decoders against each other ----
    for (size_t j = 0; j < S; ++j) {
        if (R.host[j] == V_REFUSED && R.dev[j] >= 0) CHECK(R.dev[j] != 0, "the host decoder refuses a frame the device decodes");
        if (R.host[j] == V_OK && R.dev[j] >= 0 && R.dev[j] != 0) CHECK(R.dev[j] == 2, "the device calls a frame corrupt that the host decoder takes");
        if (R.host[j] == V_OK && R.dev[j] == 0)
            CHECK(R.xyz_host[j].size() == R.xyz_dev[j].size() && memcmp(R.xyz_host[j].data(), R.xyz_dev[j].data(), R.xyz_dev[j].size() * 4) == 0,
                  "both decoders accept the frame and give different bits");
    }
    uint32_t dg = crc32_of(&R.index_status, 4);
    dg = crc32_of(&R.nframes, sizeof R.nframes, dg);
    for (size_t j = 0; j < S; ++j) {
        const int v[4] = {R.host[j], R.parser[j], R.dev[j], (int)R.dev_site[j].together};
        dg = crc32_of(v, sizeof v, dg);
        dg = crc32_of(&R.crc_host[j], 4, dg); dg = crc32_of(&R.crc_dev[j], 4, dg);
        dg = crc32_of(R.host_site[j].data(), R.host_site[j].size(), dg);
    }
    R.digest = dg;
    return R;
}

// ---------------------------------------------------------------------------------------------------------------------------
// fixtures
// ---------------------------------------------------------------------------------------------------------------------------
static Bytes slurp(const std::string& path)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "xtc_damage: cannot open %s\n", path.c_str()); exit(2); }
    Bytes b;
    uint8_t tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) b.insert(b.end(), tmp, tmp + n);
    fclose(f);
    return b;
}

static std::vector<int64_t> iota(int n) { std::vector<int64_t> v; for (int i = 0; i < n; ++i) v.push_back(i); return v; }

static Fixture load(const std::string& path)
{
    Fixture X;
    const size_t slash = path.find_last_of('/');
    X.name = path.substr(slash == std::string::npos ? 0 : slash + 1);
    X.name = X.name.substr(0, X.name.size() - 4);
    X.bytes = slurp(path);
    g_case = "undamaged " + X.name;
    g_kind = "undamaged";
    Heap buf(X.bytes.size());
    memcpy(buf.p, X.bytes.data(), buf.n);
    xtc::Mapped m;
    m.view(buf.p, buf.n);
    CHECK(xtc::index_frames(m, X.offs, X.natoms) == xtc::OK && !X.offs.empty(), "the fixture has no frames");
    const int F = (int)X.offs.size();
    const Run R = run_file(X.bytes, iota(F), X.natoms, nullptr);
    for (int f = 0; f < F; ++f) {
        CHECK(R.host[(size_t)f] == V_OK, "the host decoder refuses an undamaged frame");
        X.frames.push_back(R.xyz_host[(size_t)f]);
        X.dev0.push_back(R.dev[(size_t)f]);
        CHECK(R.dev[(size_t)f] == 0 || R.dev[(size_t)f] == 2, "the device calls an undamaged frame corrupt");
    }
    // the undamaged walk's records (where the flag and run bits of its groups are) and descriptors
    X.desc.resize((size_t)F);
    int64_t lo, hi;
    std::string msg;
    xtc::FrameIndex idx; idx.offs = X.offs; idx.natoms = X.natoms;
    CHECK(parse(buf.p, buf.n, idx, nullptr, F, X.natoms, X.desc.data(), &lo, &hi, msg) == 0 && lo == 0, "the parser refuses an undamaged file");
    X.groups.assign((size_t)F, {});
    if (X.compressed()) {
        Heap raw((size_t)hi + XTC_PAD);
        memset(raw.p, 0, raw.n);
        memcpy(raw.p, buf.p, (size_t)hi);
        std::vector<XtcGroup> groups((size_t)F * (size_t)(X.natoms + XS_SPEC));
        std::vector<int> ng((size_t)F), st((size_t)F);
        std::vector<float> out((size_t)F * (size_t)X.natoms * 3);
        g_dev.assign((size_t)F, DevRefusal());
        emu::launch(k_xtc_scan, dim3((unsigned)((F + 63) / 64)), dim3(64), (const unsigned char*)raw.p, (const XtcFrameDesc*)X.desc.data(), (long long)F,
                    (long long)X.natoms, 1.0f, out.data(), groups.data(), ng.data(), st.data());
        for (int f = 0; f < F; ++f)
            if (st[(size_t)f] == 0) X.groups[(size_t)f].assign(groups.begin() + f * (X.natoms + XS_SPEC), groups.begin() + f * (X.natoms + XS_SPEC) + ng[(size_t)f]);
    }
    X.offs.push_back(X.bytes.size());
    return X;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the damages
// ---------------------------------------------------------------------------------------------------------------------------
enum Expect { X_NONE, X_HDR_SMALLIDX, X_RANGE0, X_NATOMS, X_NBYTES_PAST, X_CUT_LAST, X_MAGIC };
struct Damage {
    std::string kind, label;
    int frame = 0;
    std::vector<std::pair<size_t, Bytes>> patch;                            // bytes written at an offset
    long long cut = -1;                                                     // the file's new length
    Bytes append;                                                           // bytes behind the file's end
    Expect expect = X_NONE;
    bool all_selections = true;                                            // else the damaged frame with its neighbours only
};

static Bytes be(uint32_t v) { return Bytes{(uint8_t)(v >> 24), (uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v}; }
static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static Bytes apply(const Fixture& X, const Damage& d)
{
    Bytes b = X.bytes;
    for (auto& p : d.patch) for (size_t i = 0; i < p.second.size(); ++i) b[p.first + i] = p.second[i];
    if (d.cut >= 0) b.resize((size_t)d.cut);
    b.insert(b.end(), d.append.begin(), d.append.end());
    return b;
}

static std::vector<int> damaged_frames(const Fixture& X)
{
    std::set<int> s = {0, X.F() / 2, X.F() - 1};
    return std::vector<int>(s.begin(), s.end());
}

static void make_damages(const Fixture& X, std::vector<Damage>& out)
{
    char lab[256];
    auto add = [&](const char* kind, int frame, Expect e, bool all) -> Damage& {
        Damage d; d.kind = kind; d.label = lab; d.frame = frame; d.expect = e; d.all_selections = all;
        out.push_back(d);
        return out.back();
    };
    const int64_t N = X.natoms;
    const bool big = N > 20000;                                             // (4rws_head: 75 338 atoms in one frame -- an emulated expand takes ~0.1 s)
    uint64_t seed = 0x58544331ull + (uint64_t)X.bytes.size() * 2654435761ull;   // ("XTC1" + the fixture's size)
    // ---- header fields (compressed files) ----
    if (X.compressed())
        for (int f : damaged_frames(X)) {
            const size_t r = X.offs[(size_t)f];
            const uint32_t nbytes = get_be32(X.bytes, r + 88), lo0 = get_be32(X.bytes, r + 60);
            const size_t stream_end = r + 92 + nbytes;
            snprintf(lab, sizeof lab, "magic 1996"); add("header: magic", f, X_MAGIC, true).patch = {{r, be(1996)}};
            const long long counts[] = {N - 1, N + 1, 0, 9, 10, -1, 1ll << 21};
            for (int copy = 0; copy < 2; ++copy)
                for (size_t ci = 0; ci < sizeof counts / sizeof counts[0]; ++ci) {
                    const long long c = counts[ci];
                    if (c == N || std::find(counts, counts + ci, c) != counts + ci) continue;     // (10 atoms: N - 1 is the 9 of the table)
                    snprintf(lab, sizeof lab, "atom count copy %d = %lld", copy + 1, c);
                    add("header: atom count", f, X_NATOMS, true).patch = {{r + (copy ? 52 : 4), be((uint32_t)c)}};
                }
            const std::pair<const char*, uint32_t> precs[] = {{"0", fbits(0.0f)}, {"-1", fbits(-1.0f)}, {"NaN", 0x7fc00000u}, {"+inf", 0x7f800000u}, {"denormal", 0x00000100u}};
            for (auto& p : precs) { snprintf(lab, sizeof lab, "precision %s", p.first); add("header: precision", f, X_NONE, true).patch = {{r + 56, be(p.second)}}; }
            {
                Bytes sw(X.bytes.begin() + r + 72, X.bytes.begin() + r + 84);
                sw.insert(sw.end(), X.bytes.begin() + r + 60, X.bytes.begin() + r + 72);
                snprintf(lab, sizeof lab, "lo and hi swapped"); add("header: range", f, X_NONE, true).patch = {{r + 60, sw}};
                snprintf(lab, sizeof lab, "hi = lo - 1 on x (range 0)"); add("header: range", f, X_RANGE0, true).patch = {{r + 72, be(lo0 - 1u)}};
                for (uint32_t v : {0xfffffeu, 0xffffffu, 0x1000000u}) {
                    snprintf(lab, sizeof lab, "hi - lo = 0x%x on x", v); add("header: range", f, X_NONE, true).patch = {{r + 72, be(lo0 + v)}};
                }
                for (int bits : {64, 65}) {                                   // ranges 2^21, 2^21, 2^21 or 2^22: a product of 2^63 (64 bits) or 2^64 (65)
                    Damage& d = (snprintf(lab, sizeof lab, "range product of %d bits", bits), add("header: range", f, X_NONE, true));
                    for (int k = 0; k < 3; ++k) d.patch.push_back({r + 72 + 4 * (size_t)k, be(get_be32(X.bytes, r + 60 + 4 * (size_t)k) + (1u << (k == 2 && bits == 65 ? 22 : 21)) - 1u)});
                }
            }
            for (int s : {-1, 0, 8, 9, 64, 65, 72, 73, 200}) {
                snprintf(lab, sizeof lab, "smallidx %d", s);
                add("header: smallidx", f, s < 9 || s > 72 ? X_HDR_SMALLIDX : X_NONE, true).patch = {{r + 84, be((uint32_t)s)}};
            }
            const long long to_end = (long long)X.bytes.size() - (long long)(r + 92);
            const std::pair<long long, Expect> nb[] = {{-1, X_NONE}, {0, X_NONE}, {1, X_NONE}, {(long long)nbytes - 4, X_NONE}, {(long long)nbytes - 1, X_NONE},
                                                       {(long long)nbytes + 1, X_NONE}, {(long long)nbytes + 4, X_NONE}, {to_end, X_NONE},
                                                       {to_end + 1, X_NBYTES_PAST}, {(1ll << 29) - 4, X_NBYTES_PAST}};
            for (auto& p : nb) {
                if (p.first == (long long)nbytes) continue;
                snprintf(lab, sizeof lab, "nbytes %lld (true %u, to the file's end %lld)", p.first, nbytes, to_end);
                add("header: nbytes", f, p.first > to_end ? X_NBYTES_PAST : p.second, true).patch = {{r + 88, be((uint32_t)p.first)}};
            }
            // a file with two bytes behind its last record, and a stream said to run up to them: the byte range's end is then no multiple of 4
            snprintf(lab, sizeof lab, "nbytes up to the end of a file with 2 trailing bytes");
            Damage& d = add("header: nbytes", f, X_NONE, true);
            d.patch = {{r + 88, be((uint32_t)(to_end + 2))}};
            d.append = Bytes{0xff, 0xff};
            (void)stream_end;
        }
    // ---- truncation (every fixture): around the structural boundaries of the last record, seeded places in its stream ----
    {
        const int f = X.F() - 1;
        const size_t r = X.offs[(size_t)f], end = X.bytes.size();
        std::set<long long> cuts;
        if (!X.compressed() && N <= 2) for (size_t c = r; c < end; ++c) cuts.insert((long long)c);
        for (long long c : {(long long)r, (long long)r + 56, (long long)r + 92, (long long)end - 4, (long long)end})
            for (int dlt = -1; dlt <= 1; ++dlt) cuts.insert(c + dlt);
        if (X.compressed()) for (int i = 0; i < 3; ++i) cuts.insert((long long)(r + 93 + splitmix(seed) % (end - r - 97)));
        for (long long c : cuts) {
            if (c < 0 || c >= (long long)end) continue;
            snprintf(lab, sizeof lab, "file cut to %lld of %zu bytes (last record at %zu)", c, end, r);
            // (a cut in front of the last record is inside the record before: that one is the damaged frame then)
            add("truncation", c >= (long long)r ? f : f - 1, X_CUT_LAST, true).cut = c;
        }
    }
    if (!X.compressed()) return;
    // ---- stream bits ----
    for (int f : damaged_frames(X)) {
        const size_t r = X.offs[(size_t)f], s0 = r + 92;
        const uint32_t nbytes = get_be32(X.bytes, r + 88);
        auto flip = [&](const char* kind, size_t bit, bool all) {
            if (bit >= (size_t)nbytes * 8) return;
            snprintf(lab, sizeof lab, "bit %zu of the stream flipped", bit);
            add(kind, f, X_NONE, all).patch = {{s0 + bit / 8, Bytes{(uint8_t)(X.bytes[s0 + bit / 8] ^ (0x80u >> (bit & 7)))}}};
        };
        if (nbytes <= 256) {
            for (size_t bit = 0; bit < (size_t)nbytes * 8; ++bit) flip("stream: every bit", bit, true);
        } else {
            const XtcFrameDesc& d = X.desc[(size_t)f];
            const unsigned full = d.triple_bits ? (unsigned)d.triple_bits : (unsigned)(d.field_bits[0] + d.field_bits[1] + d.field_bits[2]);
            const auto& G = X.groups[(size_t)f];
            for (size_t g = 0; g < std::min<size_t>(64, G.size()); ++g)
                for (unsigned k = 0; k < 6; ++k) flip(k ? "stream: run bit" : "stream: flag bit", G[g].pos + full + k, !big);
            for (size_t w = XS_WIN * 8; w < (size_t)nbytes * 8; w += XS_WIN * 8) { flip("stream: bit at a refill", w - 1, !big); flip("stream: bit at a refill", w, !big); }
            for (int i = 0; i < (big ? 4 : 12); ++i) flip("stream: seeded bit", (size_t)(splitmix(seed) % ((uint64_t)nbytes * 8)), !big && i % 4 == 0);
        }
        for (int len : {1, 4, 16})
            for (int fill = 0; fill < 3; ++fill) {
                if ((uint32_t)len >= nbytes) continue;
                const size_t at = (size_t)(splitmix(seed) % (nbytes - (uint32_t)len));
                Bytes g((size_t)len);
                for (auto& c : g) c = fill == 0 ? (uint8_t)splitmix(seed) : fill == 1 ? 0x00 : 0xff;
                snprintf(lab, sizeof lab, "%d bytes of %s at byte %zu of the stream", len, fill == 0 ? "garbage" : fill == 1 ? "zeros" : "ones", at);
                add("stream: garbage run", f, X_NONE, !big && len == 4).patch = {{s0 + at, g}};
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// a case: a damage, a selection, both views; twice
// ---------------------------------------------------------------------------------------------------------------------------
struct Listed {                                                            // what --list prints (tests/golden/xtc_damage_cases.json)
    std::string key;
    std::string json;
};
static std::vector<Listed> g_listed;
static std::map<std::string, int> g_listed_n;
static long long g_cases = 0, g_runs = 0;
static std::map<std::string, long long> g_kind_cases;

static std::string hex(const Bytes& b) { std::string s; char t[3]; for (uint8_t c : b) { snprintf(t, 3, "%02x", c); s += t; } return s; }

static void list_case(const std::string& key, const Fixture& X, const Damage& d, const char* selname, const std::vector<int64_t>& sel, const Run& R, long long id)
{
    if (g_listed_n[key] >= 2) return;
    ++g_listed_n[key];
    std::string j = "{\"id\": " + std::to_string(id) + ", \"key\": \"" + key + "\", \"fixture\": \"" + X.name + "\", \"frame\": " + std::to_string(d.frame) +
                    ", \"kind\": \"" + d.kind + "\", \"damage\": \"" + d.label + "\", \"patch\": [";
    for (size_t i = 0; i < d.patch.size(); ++i) j += std::string(i ? ", " : "") + "[" + std::to_string(d.patch[i].first) + ", \"" + hex(d.patch[i].second) + "\"]";
    j += "], \"cut\": " + (d.cut < 0 ? std::string("null") : std::to_string(d.cut)) + ", \"append\": \"" + hex(d.append) + "\", \"selection_name\": \"" + selname +
         "\", \"selection\": [";
    for (size_t i = 0; i < sel.size(); ++i) j += (i ? ", " : "") + std::to_string(sel[i]);
    j += "], \"frames_indexed\": " + std::to_string(R.nframes) + ", \"index_status\": " + std::to_string(R.index_status) + ", \"host\": [";
    for (size_t i = 0; i < sel.size(); ++i) j += (i ? ", " : "") + std::to_string(R.host[i]);
    j += "], \"parser\": [";
    for (size_t i = 0; i < sel.size(); ++i) j += (i ? ", " : "") + std::to_string(R.parser[i]);
    j += "], \"device\": [";
    for (size_t i = 0; i < sel.size(); ++i) j += (i ? ", " : "") + std::to_string(R.dev[i]);
    uint32_t crc = 0;
    for (size_t i = 0; i < sel.size(); ++i) if (R.dev[i] == 0) crc = crc32_of(R.xyz_dev[i].data(), R.xyz_dev[i].size() * 4, crc);
    j += "], \"crc32\": " + std::to_string(crc) + "}";
    g_listed.push_back(Listed{key, j});
}

static bool finite_bits(const std::vector<float>& v) { for (float x : v) if (!(x - x == 0.0f)) return false; return true; }

static void run_case(const Fixture& X, const Damage& d, long long id)
{
    const Bytes file = apply(X, d);
    const int F = X.F(), k = d.frame;
    g_kind = d.kind;
    ++g_kind_cases[d.kind];
    struct Sel { const char* name; std::vector<int64_t> v; };
    std::vector<Sel> sels;
    {
        std::vector<int64_t> nb;
        for (int f = std::max(0, k - 1); f <= std::min(F - 1, k + 1); ++f) nb.push_back(f);
        sels.push_back(Sel{"neighbours", nb});
        if (d.all_selections) {
            sels.push_back(Sel{"alone", {(int64_t)k}});
            // (the cost of an emulated launch grows with the atoms it decodes: 4rws_head leaves it at these two)
            if (X.natoms <= 20000) sels.push_back(Sel{"reversed", std::vector<int64_t>(nb.rbegin(), nb.rend())});
            // 65 lanes: a second wave, and live and dead lanes in the first.  An emulated launch of 65 frames of thousands of atoms costs
            // twenty launches of three: the files of more than 1 300 atoms get it on their header cases, cuts and the bits at their
            // window refills (the dead lanes' refills are about those), not on each located or seeded bit; 4rws_head not at all
            const bool structural = d.kind.compare(0, 7, "header:") == 0 || d.kind == "truncation" || d.kind == "stream: bit at a refill";
            if (X.natoms <= 1300 || (X.natoms <= 20000 && structural)) {
                std::vector<int64_t> many;
                for (int i = 0; i < 65; ++i) many.push_back((k + i) % F);
                if (F == 1) many.assign(65, 0);
                sels.push_back(Sel{"65 frames", many});
            }
        }
    }
    for (size_t a = sels.size(); a-- > 1;)                                  // (a one-frame file: 'alone' and 'reversed' are 'neighbours')
        for (size_t b = 0; b < a; ++b) if (sels[a].v == sels[b].v) { sels.erase(sels.begin() + (long)a); break; }
    xtc::FrameIndex stale;
    stale.offs.assign(X.offs.begin(), X.offs.end() - 1);
    stale.natoms = X.natoms;
    for (const Sel& s : sels)
        for (int view = 0; view < 2; ++view) {
            // (a stale index on a shorter file points outside it: not a state index_frames_cached can be in; and a damaged stream
            //  leaves the index as it was: the two views are the same run; the stale view is run on the first selection)
            const bool first_sel = &s == &sels[0];
            if (view == 1 && (file.size() < X.bytes.size() || d.kind.compare(0, 7, "stream:") == 0 || !first_sel)) continue;
            g_case = X.name + ", frame " + std::to_string(k) + ": " + d.kind + ": " + d.label + "; selection '" + s.name + "', " + (view ? "stale" : "fresh") + " index";
            const Run R = run_file(file, s.v, X.natoms, view ? &stale : nullptr);
            const std::map<std::string, long long> after = g_reach;
            ++g_runs;
            // (4rws_head, 75 338 atoms and 275 windows per walk: its header cases only)
            // (every selection of the header cases, cuts, exhaustive and refill bits of the files of up to 2 000 atoms; the first
            //  selection of everything else; 4rws_head, 75 338 atoms and 275 windows per walk: of its header cases only)
            const bool located = d.kind == "stream: flag bit" || d.kind == "stream: run bit" || d.kind == "stream: seeded bit" || d.kind == "stream: garbage run";
            if (view == 0 && ((X.natoms <= 2000 && !located) || (first_sel && (X.natoms <= 20000 || d.kind.compare(0, 7, "header:") == 0)))) {                                   // the case once more: the same verdicts, sites and bits
                const Run R2 = run_file(file, s.v, X.natoms, nullptr);
                g_reach = after;                                            // (the second run is not counted)
                CHECK(R.digest == R2.digest, "two runs of the case differ");
                ++g_runs;
            }
            const bool file_off = R.natoms != X.natoms || R.index_status != 0;
            // ---- the control: undamaged frames decode to the undamaged file's bits, in both decoders ----
            bool index_moved = false;                                       // (a damaged length field: the records behind are no longer where they were)
            for (size_t j = 0; j < s.v.size(); ++j) {
                const int f = (int)s.v[j];
                if (f == k) continue;
                if (d.kind == "truncation" && f > k) continue;
                if (view == 0 && f > k && (R.nframes != (size_t)F)) { index_moved = true; continue; }
                if (file_off) continue;
                CHECK(R.host[j] == V_OK && memcmp(R.xyz_host[j].data(), X.frames[(size_t)f].data(), X.frames[(size_t)f].size() * 4) == 0,
                      "host decoder: an undamaged frame of the call does not decode to its bits");
                CHECK(R.dev[j] == X.dev0[(size_t)f], "device decoder: an undamaged frame of the call does not get its status");
                if (X.dev0[(size_t)f] == 0)
                    CHECK(memcmp(R.xyz_dev[j].data(), X.frames[(size_t)f].data(), X.frames[(size_t)f].size() * 4) == 0,
                          "device decoder: an undamaged frame of the call does not decode to its bits");
            }
            (void)index_moved;
            // ---- the verdict the damage implies ----
            for (size_t j = 0; j < s.v.size(); ++j) {
                if ((int)s.v[j] != k) continue;
                switch (d.expect) {
                case X_NONE: break;
                case X_HDR_SMALLIDX:
                    CHECK(R.host[j] == V_REFUSED && R.host_site[j] == "frame: header smallidx", "header smallidx outside 9..72: the host decoder does not refuse it for that");
                    CHECK(R.parser[j] == 0 && (R.dev[j] == 1 || (R.dev[j] == 2 && X.desc[(size_t)k].triple_bits > 64)), "header smallidx outside 9..72: device status is not 1");
                    if (R.dev[j] == 1) CHECK(std::string(R.dev_site[j].site) == "dev: header smallidx", "header smallidx outside 9..72: refused elsewhere");
                    break;
                case X_RANGE0:
                    CHECK(R.host[j] == V_REFUSED && R.host_site[j] == "frame: range 0" && R.parser[j] == 1 && R.dev[j] == -1, "range 0: not refused by the host decoder and the parser for that");
                    break;
                case X_NATOMS:
                    if (view == 0 && k == 0 && R.natoms != X.natoms) { CHECK(R.read_status == xtc::E_RANGE || R.index_status || R.nframes == 0, "a file whose first atom count changed is read"); break; }
                    CHECK(R.host[j] != V_OK && R.dev[j] == -1, "differing atom counts: the frame is decoded");
                    if (R.host[j] == V_REFUSED) CHECK(R.parser[j] == 1 && (R.host_site[j] == "frame: first atom count" || R.host_site[j] == "frame: second atom count"), "differing atom counts: refused for something else");
                    break;
                case X_NBYTES_PAST:
                    if (view == 0) CHECK(R.host[j] == V_DROPPED && R.nframes == (size_t)k && R.parser[j] == 2, "nbytes past the file: the record is still in the frame index");
                    else CHECK(R.host[j] == V_REFUSED && R.host_site[j] == "frame: nbytes" && R.parser[j] == 1 && R.dev[j] == -1, "nbytes past the file: not refused by the host decoder and the parser for that");
                    break;
                case X_CUT_LAST:
                    CHECK(R.host[j] == V_DROPPED && R.nframes == (size_t)k && R.parser[j] == 2 && R.dev[j] == -1, "a cut inside the record: the record is still in the frame index");
                    break;
                case X_MAGIC:
                    if (view == 0) CHECK(R.host[j] == V_DROPPED && R.nframes == (size_t)k && (k > 0 || R.index_status == xtc::E_FORMAT), "wrong magic: the record is still in the frame index");
                    else CHECK(R.host[j] == V_REFUSED && R.host_site[j] == "frame: magic" && R.parser[j] == 1, "wrong magic: not refused for that");
                    break;
                }
            }
            // ---- what goes into the list for the GPU tier: fresh view, neighbours (or the named selections), small output ----
            if (view == 0 && !file_off) {
                for (size_t j = 0; j < s.v.size(); ++j) {
                    if ((int)s.v[j] != k) continue;
                    const bool nb = std::string(s.name) == "neighbours";
                    if (R.dev[j] > 0) {
                        if (nb) list_case(std::string(R.dev_site[j].site), X, d, s.name, s.v, R, id);
                        // (refused BY the damage: a frame the device leaves to the host as it is -- triple65 -- is not listed under its damages' kinds)
                        if (nb && X.dev0[(size_t)k] == 0) list_case("kind " + d.kind + " refused", X, d, s.name, s.v, R, id);
                        if (R.dev_site[j].together) list_case("refusal while together", X, d, s.name, s.v, R, id);
                        if (std::string(s.name) == "65 frames") list_case("refusal in a mixed wave", X, d, s.name, s.v, R, id);
                    } else if (nb && R.parser[j] == 1) list_case("parser refuses: " + d.kind, X, d, s.name, s.v, R, id);
                    else if (nb && R.parser[j] == 2) list_case("dropped from the index: " + d.kind, X, d, s.name, s.v, R, id);
                    else if (nb && R.dev[j] == 0 && R.host[j] == V_OK && finite_bits(R.xyz_dev[j]) &&
                             memcmp(R.xyz_dev[j].data(), X.frames[(size_t)k].data(), R.xyz_dev[j].size() * 4) != 0)
                        list_case("accepted by both: " + d.kind, X, d, s.name, s.v, R, id);
                    break;
                }
            }
        }
    ++g_cases;
}

int main(int argc, char** argv)
{
    int shard = 0, nshards = 1;
    bool list = false;
    std::vector<std::string> paths;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--shard" && i + 2 < argc) { shard = atoi(argv[i + 1]); nshards = atoi(argv[i + 2]); i += 2; }
        else if (a == "--list") list = true;
        else paths.push_back(a);
    }
    if (paths.empty() || nshards < 1 || shard < 0 || shard >= nshards) { fprintf(stderr, "usage: xtc_damage [--shard I N] [--list] fixture.xtc ...\n"); return 2; }
    long long id = 0;
    for (const std::string& p : paths) {
        const Fixture X = load(p);
        std::vector<Damage> table;
        make_damages(X, table);
        for (const Damage& d : table) {
            if (id % nshards == shard) run_case(X, d, id);
            ++id;
        }
    }
    if (shard == 0) {
        // the host's errors that no file's contents draw: a path that does not open
        std::string err;
        int64_t na, nf;
        g_kind = "no file";
        if (xtc::info("/nonexistent/x.xtc", na, nf, err) == xtc::E_OPEN) reach("host: info: cannot open");
        float c[3], b[9], t[1]; int32_t s[1];
        if (xtc::read("/nonexistent/x.xtc", nullptr, 1, 1, c, b, t, s, 1, err) == xtc::E_OPEN) reach("host: read: cannot open");
    }
    printf("{\"cases\": %lld, \"runs\": %lld, \"kinds\": {", g_cases, g_runs);
    bool first = true;
    for (auto& kv : g_kind_cases) { printf("%s\"%s\": %lld", first ? "" : ", ", kv.first.c_str(), kv.second); first = false; }
    printf("}, \"reach\": {");
    first = true;
    for (auto& kv : g_reach) { printf("%s\"%s\": %lld", first ? "" : ", ", kv.first.c_str(), kv.second); first = false; }
    printf("}, \"listed\": [");
    if (list) for (size_t i = 0; i < g_listed.size(); ++i) printf("%s%s", i ? ", " : "", g_listed[i].json.c_str());
    printf("]}\n");
    return 0;
}
