// fimex_amd/csrc/slice_list.hpp for the CPU tests (tests/test_slice_list.py, through tests/slice_list_host.py): the table of a list
// launch, the cutting of a list into launches, and the two cursors of a workgroup walked over a z chunk the way SliceRing
// (staged2_ring.hpp) walks them.
#include "slice_list.hpp"

using namespace fimex_amd;

extern "C" {

uint32_t sl_max_vars() { return kSliceListMaxVars; }

// the table of nz[nvar]: ends[] and index[] (kSliceListMaxVars entries each), *held variables with slices, *total slices;
// returns 0 where build_slice_ends refuses the list
int sl_build(const uint64_t* nz, uint64_t nvar, uint32_t* ends, uint32_t* index, uint32_t* held, uint64_t* total)
{
    SliceEnds e;
    size_t t = 0;
    size_t n[4096];
    if (nvar > 4096) return 0;
    for (uint64_t i = 0; i < nvar; ++i) n[i] = (size_t)nz[i];
    const bool ok = build_slice_ends(n, (size_t)nvar, e, index, t);
    for (uint32_t k = 0; k < kSliceListMaxVars; ++k) ends[k] = e.ends[k];
    *held = e.nvar;
    *total = t;
    return ok ? 1 : 0;
}

// list_slices of nz[nvar]
uint64_t sl_list_slices(const uint64_t* nz, uint64_t nvar)
{
    size_t n[4096];
    if (nvar > 4096) return 0;
    for (uint64_t i = 0; i < nvar; ++i) n[i] = (size_t)nz[i];
    return list_slices(n, (size_t)nvar);
}

// The launches for_list_launches cuts nz[nvar] into: first[k], count[k] of launch k (room for `room` of them), accepted[k] whether
// build_slice_ends takes nz[first[k] .. first[k] + count[k]).  Returns the number of launches, -1 where there is no room.
int sl_launches(const uint64_t* nz, uint64_t nvar, uint64_t* first, uint64_t* count, int32_t* accepted, int room)
{
    size_t n[4096];
    if (nvar > 4096) return -1;
    for (uint64_t i = 0; i < nvar; ++i) n[i] = (size_t)nz[i];
    int made = 0;
    bool full = false;
    for_list_launches(n, (size_t)nvar, [&](size_t f, size_t c) {
        if (made == room) {
            full = true;
            return;
        }
        SliceEnds e;
        uint32_t index[kSliceListMaxVars];
        size_t total = 0;
        first[made] = f;
        count[made] = c;
        accepted[made++] = build_slice_ends(n + f, c, e, index, total) ? 1 : 0;
    });
    return full ? -1 : made;
}

// One workgroup's walk over the logical slices [z0, z1) of the list with a ring of `depth` slots: both cursors seeded at z0, the
// first depth - 1 slices fetched ahead of the loop, then per trip i the fetch of slice z0 + i + depth - 1 (where the chunk has
// it) before slice z0 + i is worked on.  fetch*[k]: the k-th fetch (variable as the caller counts them, level, the trip that
// issued it, -1 ahead of the loop); work*[i]: the slice of trip i.  Returns the number of fetches, or -1 as soon as a cursor
// names a variable or a level that does not exist.
int sl_walk(const uint64_t* nz, uint64_t nvar, uint32_t z0, uint32_t z1, uint32_t depth, int32_t* fetchVar, int32_t* fetchLevel, int32_t* fetchTrip,
            int32_t* workVar, int32_t* workLevel)
{
    SliceEnds e;
    uint32_t index[kSliceListMaxVars];
    size_t total = 0;
    size_t n[64];
    if (nvar > 64) return -1;
    for (uint64_t i = 0; i < nvar; ++i) n[i] = (size_t)nz[i];
    if (!build_slice_ends(n, (size_t)nvar, e, index, total) || z1 > total || z0 >= z1) return -1;
    auto exists = [&](const SliceCursor& c) { return c.var < e.nvar && c.level < n[index[c.var]]; };
    SliceCursor cur = slice_seek(e.ends, e.nvar, z0), src = cur;
    if (!exists(cur)) return -1;
    int fetches = 0;
    auto fetch = [&](int trip) {
        fetchVar[fetches] = (int32_t)index[src.var];
        fetchLevel[fetches] = (int32_t)src.level;
        fetchTrip[fetches++] = trip;
        slice_advance(e.ends, e.nvar, src);
        return exists(src);
    };
    const uint32_t nzl = z1 - z0;
    for (uint32_t i = 0; i + 1 < depth && i < nzl; ++i)
        if (!fetch(-1)) return -1;
    for (uint32_t i = 0; i < nzl; ++i) {
        if (i + depth - 1 < nzl && !fetch((int)i)) return -1;
        workVar[i] = (int32_t)index[cur.var];
        workLevel[i] = (int32_t)cur.level;
        slice_advance(e.ends, e.nvar, cur);
        if (!exists(cur)) return -1;
    }
    return fetches;
}

}  // extern "C"
