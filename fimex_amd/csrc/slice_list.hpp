// The slices of a list launch of the second staged form (staged2_list.hip, staged2_list_typed.hip): a launch regrids the slices of
// several variables, each an array of its own, and its kernels count LOGICAL slices 0 .. total - 1 -- the variables' levels one
// variable after the other.  The z chunks cut the logical slices as they cut one array, so a chunk may begin and end inside a
// variable.  Here: which variable and level a logical slice is, as a cursor that is seeded once per workgroup and then moved one
// slice at a time; and how a list of more variables than a launch takes is cut into launches.  Plain arithmetic without a HIP
// include, as staged_layout.hpp: the launchers build the table on the host, the kernels move cursors on the device, and
// tests/test_slice_list.py compiles it with g++ and checks it on the CPU -- a cursor that is wrong by one makes a base pointer
// of a foreign allocation.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define FA_SLICES_HD __host__ __device__ __forceinline__
#else
#define FA_SLICES_HD inline
#endif

namespace fimex_amd {

// Variables of one launch (FIMEX_AMD_REGRID_MULTI_MAX_VARS): the tables travel in the kernel arguments, 4 KiB in all, beside
// Staged2Args (about 300 bytes) -- two pointers and an end per variable, for stored types a fill value as float and as double
// too: 64 * 32 = 2 KiB.  128 variables would not fit the stored-type kernel.
constexpr uint32_t kSliceListMaxVars = 64;

// ends[i] = nz[0] + ... + nz[i] over the nvar variables of the launch, every nz[i] > 0 (build_slice_ends drops the others)
struct SliceEnds {
    uint32_t nvar;
    uint32_t ends[kSliceListMaxVars];
};

// A logical slice: level `level` of variable `var`, of which `left` levels remain, this one included.  left == 0: the cursor has
// been moved beyond the last slice of the launch; it then still names the last slice, never a variable that does not exist.
struct SliceCursor {
    uint32_t var, level, left;
};

// Host: the table of up to kSliceListMaxVars variables with nz[i] slices.  Variables without slices are left out; index[k] is the
// caller's variable behind entry k, total the number of logical slices.  false: more than kSliceListMaxVars variables with
// slices, or more than 2^32 - 1 slices.
inline bool build_slice_ends(const size_t* nz, size_t nvar, SliceEnds& e, uint32_t* index, size_t& total)
{
    e = SliceEnds{};
    total = 0;
    for (size_t i = 0; i < nvar; ++i) {
        if (nz[i] == 0) continue;
        if (e.nvar == kSliceListMaxVars || nz[i] > 0xFFFFFFFFu - total) return false;
        total += nz[i];
        index[e.nvar] = (uint32_t)i;
        e.ends[e.nvar++] = (uint32_t)total;
    }
    return true;
}

// Host: the slices of a list, 0 where there are more than a launch counts
inline size_t list_slices(const size_t* nz, size_t nvar)
{
    size_t total = 0;
    for (size_t i = 0; i < nvar; ++i) {
        if (nz[i] > 0xFFFFFFFFu - total) return 0;
        total += nz[i];
    }
    return total;
}

// Host: a list of more variables than a launch takes is cut -- launch(first, count) on runs of the list that hold at most
// kSliceListMaxVars variables with slices, so that build_slice_ends takes each of them
template <class Launch>
inline void for_list_launches(const size_t* nz, size_t nvar, Launch&& launch)
{
    size_t first = 0, held = 0;
    for (size_t i = 0; i < nvar; ++i) {
        if (nz[i] == 0) continue;
        if (held == kSliceListMaxVars) {
            launch(first, i - first);
            first = i;
            held = 0;
        }
        ++held;
    }
    if (held) launch(first, nvar - first);
}

// the cursor at logical slice l < ends[nvar - 1]: a scan over at most kSliceListMaxVars prefix sums
FA_SLICES_HD SliceCursor slice_seek(const uint32_t* ends, uint32_t nvar, uint32_t l)
{
    uint32_t var = 0;
    while (var + 1 < nvar && ends[var] <= l) ++var;
    const uint32_t begin = var ? ends[var - 1] : 0u;
    SliceCursor c;
    c.var = var;
    if (l < ends[var]) {
        c.level = l - begin;
        c.left = ends[var] - l;
    } else {  // beyond the last slice
        c.level = ends[var] - begin - 1;
        c.left = 0;
    }
    return c;
}

// one slice further
FA_SLICES_HD void slice_advance(const uint32_t* ends, uint32_t nvar, SliceCursor& c)
{
    if (c.left > 1) {
        ++c.level;
        --c.left;
    } else if (c.var + 1 < nvar) {
        c.left = ends[c.var + 1] - ends[c.var];
        ++c.var;
        c.level = 0;
    } else {
        c.left = 0;
    }
}

}  // namespace fimex_amd
