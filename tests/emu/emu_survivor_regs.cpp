// tests/emu/emu_survivor_regs.cpp -- TEST INFRASTRUCTURE: the survivors a tile keeps in registers between its histogram pass and its
// placement pass (round 10), on the host emulation.  The translation unit of tests/emu/emu_cover_fold.cpp, whole (its entry point runs
// a handle call with the fold on or off), plus the receiver of MK_SURV_PROBE (csrc/mk_diagnostics.h): per tile of the SURV_LIST
// instances the candidates, the survivors the cull pass counted, the path taken, and which x-reach values the lanes hold in which of
// their eight survivor registers.  Built twice by tests/emu_survivor_regs_build.py: as it is, and with -DMK_DIAG=256 (the placement
// reads register 1's x-reach for register 0: the mutation the tests must catch).
#include <map>
#include <utility>

namespace {
struct SurvTile { unsigned N = 0, nsurv = 0, use_list = 0, xr_seen = 0; };
std::map<std::pair<unsigned, int>, SurvTile> g_surv_tiles;                  // (tile of the launch, channel group) -> what its lanes said
}
// called by every lane of a tile's wave behind the histogram pass; xr_word: two bits per survivor register of this lane
static void mk_surv_probe(unsigned lt, int gq, int thread, unsigned N, unsigned nsurv, bool use_list, unsigned xr_word)
{
    SurvTile& t = g_surv_tiles[std::make_pair(lt, gq)];
    t.N = N; t.nsurv = nsurv; t.use_list = use_list ? 1u : 0u;
    const unsigned lane = (unsigned)thread & 63u;
    if (use_list)
        for (unsigned j = 0; j < 8u; ++j)
            if (64u * j + lane < nsurv) t.xr_seen |= 1u << (3u * j + ((xr_word >> (2u * j)) & 3u));     // bit 3 j + xr
}

#include "emu_cover_fold.cpp"

extern "C" {
void emu_surv_probe_reset() { g_surv_tiles.clear(); }
int emu_surv_probe_count() { return (int)g_surv_tiles.size(); }
// rows of (tile, group, N, nsurv, use_list, xr_seen)
void emu_surv_probe_read(unsigned* out)
{
    for (const auto& kv : g_surv_tiles) {
        *out++ = kv.first.first; *out++ = (unsigned)kv.first.second;
        *out++ = kv.second.N; *out++ = kv.second.nsurv; *out++ = kv.second.use_list; *out++ = kv.second.xr_seen;
    }
}
}
