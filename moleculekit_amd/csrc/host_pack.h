// host_pack.h -- the atoms a HOST call of the trajectory metrics selects, packed before the upload.
// The reference's drivers hand every call the whole trajectory (projections/util.py:40-70: mol.coords) and selections that are
// usually a few hundred atoms of a solvated system: MetricDistance's protein C-alpha x ligand call reads 330 of 30 000 atoms --
// 8 MB of a 737-MB array -- and the host entry points uploaded all of it, 15 ms in front of a 36-us kernel.  The rows of an atom
// are contiguous in the reference's layout ([atom][3][frame]), so packing is one memcpy per selected atom (gather_rows); selections,
// group atom lists, chain ids and masses are rewritten to the packed numbering, and what comes back as atom indices (contact lists)
// is translated back.  PackedAtoms::finish packs where it pays (the distance, shell and dihedral calls) or always (group moments);
// the surface-area call gathers its kept atoms in the caller's order with gather_rows alone.
// Plain C++ (no HIP): compiled into the library's host entry points (capi.hip: HostStage) and, for the tests, into the emulator.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace mkamd {

// rows idx[0..n) of coords ([N][3][F]) into out ([n][3][F], grown as needed): in the order given, repeats included
template <class T>
inline void gather_rows(const float* coords, int64_t F, const T* idx, int64_t n, std::vector<float>& out)
{
    const size_t row = (size_t)3 * (size_t)F;
    if (out.size() < (size_t)n * row) out.resize((size_t)n * row);
    for (int64_t k = 0; k < n; ++k) std::memcpy(out.data() + (size_t)k * row, coords + (size_t)idx[k] * row, row * sizeof(float));
}

struct PackedAtoms {
    bool on = false;                     // false: the call uploads the array as it is
    std::vector<uint32_t> uniq;          // packed index -> atom (ascending)

    template <class T>
    void collect(const T* idx, int64_t n) { for (int64_t i = 0; i < n; ++i) uniq.push_back((uint32_t)idx[i]); }

    // Decide, and pack the coordinates into `out` ([M, 3, F], grown as needed): worth it when the selected atoms are at most a quarter
    // of the array's and the array is more than a megabyte; `always`: whatever their number and the array's size
    bool finish(const float* coords, int64_t N, int64_t F, std::vector<float>& out, bool always = false)
    {
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        const size_t M = uniq.size();
        on = always || (M > 0 && M * 4 <= (size_t)N && (size_t)N * 3 * (size_t)F * 4 > ((size_t)1 << 20));
        if (on) gather_rows(coords, F, uniq.data(), (int64_t)M, out);
        return on;
    }
    int64_t size() const { return (int64_t)uniq.size(); }
    uint32_t packed(uint32_t atom) const { return (uint32_t)(std::lower_bound(uniq.begin(), uniq.end(), atom) - uniq.begin()); }
    template <class T>
    std::vector<T> remap(const T* idx, int64_t n) const
    {
        std::vector<T> r((size_t)n);
        for (int64_t i = 0; i < n; ++i) r[(size_t)i] = (T)packed((uint32_t)idx[i]);
        return r;
    }
    template <class T>
    std::vector<T> gather(const T* per_atom) const               // chain ids, masses: one value per atom of the array
    {
        std::vector<T> r(uniq.size());
        for (size_t k = 0; k < uniq.size(); ++k) r[k] = per_atom[uniq[k]];
        return r;
    }
    void unpack_in_place(uint32_t* atoms, size_t n) const { for (size_t i = 0; i < n; ++i) atoms[i] = uniq[atoms[i]]; }
};

}  // namespace mkamd
