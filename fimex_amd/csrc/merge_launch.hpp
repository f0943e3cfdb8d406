// Launch geometry shared by the merge kernels on float arrays (merge.hip), on stored types (merge_typed.hip), on float vector
// pairs (merge_vector.hip) and on packed vector pairs (merge_vector_typed.hip): the tile of a workgroup, the slices in flight per
// lane, the grid over tiles and chunks of slices, the stencil size of a backward plan, for the two float files a plan's arrays as
// kernel arguments and the call's scratch, and for the two pair files the pair-slices in flight and a rotation's lazy read.
#pragma once

#include "gather_entry.hpp"
#include "plan.hpp"

namespace fimex_amd {
namespace merge_launch {

constexpr int kTileX = 64, kTileY = 4;  // a wave per row
static_assert(kTileX * kTileY == kBlock, "a tile is one workgroup");
constexpr int kAhead = 4;               // slices whose loads are in flight together

// ---- the kernels on a vector pair (merge_vector.hip, merge_vector_typed.hip)
// pair-slices in flight per lane: a bicubic entry holds 2 x 16 taps per pair-slice and combines them in double
template <int STENCIL>
constexpr int ahead_of() { return STENCIL == 4 ? 1 : STENCIL == 2 ? 2 : 4; }
static_assert(kAhead % ahead_of<1>() == 0 && kAhead % ahead_of<2>() == 0, "a z chunk is a whole number of groups");

// (m0, m1) of one cell of a rotation, read at first use
struct LazyMatrix {
    const double2* cs;
    uint32_t cell;
    bool have = false;
    double2 m = {0., 0.};
    __device__ __forceinline__ const double2& get()
    {
        if (!have) {
            m = cs[cell];
            have = true;
        }
        return m;
    }
};

// tiles of one slice in x and y, chunks of slices in z: enough workgroups to fill the device, chunks long enough to amortise the
// per-cell set-up (class, plan entries)
inline dim3 tile_grid(size_t nx, size_t ny, size_t nz, uint32_t& zPerBlock)
{
    FA_REQUIRE(nx * ny <= kMaxSliceCells, "a slice must have fewer than 2^30 cells");
    FA_REQUIRE(nz <= 0xFFFFFFFFu, "too many slices");
    const size_t tilesX = ceil_div(nx, kTileX), tilesY = ceil_div(ny, kTileY);
    FA_REQUIRE(tilesY <= 65535, "grid too tall for one launch");
    const size_t wantBlocks = 256 * 8 * 4;
    size_t chunks = ceil_div(wantBlocks, tilesX * tilesY);
    if (chunks > nz) chunks = nz;
    size_t zpb = ceil_div(nz, chunks);
    zpb = ceil_div(zpb, kAhead) * kAhead;
    if (ceil_div(nz, zpb) > 65535) zpb = ceil_div(nz, (size_t)65535);
    zPerBlock = (uint32_t)zpb;
    return dim3((uint32_t)tilesX, (uint32_t)tilesY, (uint32_t)ceil_div(nz, zpb));
}

inline int stencil_of(const fimex_amd_regrid_plan& p)
{
    switch (p.kind) {
    case PlanKind::Nearest: return 1;
    case PlanKind::Bilinear: return 2;
    case PlanKind::Bicubic: return 4;
    default: throw Error("merge: not a backward plan");
    }
}

// ---- a backward plan's arrays on float slices; an entry is decoded once per cell and evaluated slice by slice (gather_entry.hpp:
// an undefined entry issues loads that are dropped and gives NaN, so the lane stays on the common path)
struct PlanRef {
    const uint32_t* pos;
    const float *xf, *yf;
    const double *xfd, *yfd;
    uint32_t ix;       // source row length
    uint32_t inBytes;  // bytes of a source slice
    size_t inLayer;    // cells of a source slice

    template <int STENCIL>
    __device__ __forceinline__ GatherEntry<STENCIL, float> entry(uint32_t cell) const
    {
        if constexpr (STENCIL == 4) return {pos[cell], xfd[cell], yfd[cell], ix};
        else if constexpr (STENCIL == 2) return {pos[cell], xf[cell], yf[cell], ix};
        else return {pos[cell], 0.f, 0.f, ix};
    }
};

inline PlanRef plan_ref(const fimex_amd_regrid_plan& p)
{
    PlanRef r{};
    r.pos = p.pos.get();
    r.xf = p.xf.get();
    r.yf = p.yf.get();
    r.xfd = p.xfd.get();
    r.yfd = p.yfd.get();
    r.ix = (uint32_t)p.inX;
    r.inLayer = p.inX * p.inY;
    r.inBytes = (uint32_t)(r.inLayer * 4);
    return r;
}

// stream-ordered float scratch of one call, freed on the stream behind the kernels that use it
class FloatScratch {
public:
    FloatScratch(size_t floats, hipStream_t stream) : stream_(stream)
    {
        if (floats) FA_HIP(hipMallocAsync(reinterpret_cast<void**>(&p_), floats * sizeof(float), stream));
    }
    ~FloatScratch() { if (p_) (void)hipFreeAsync(p_, stream_); }
    FloatScratch(const FloatScratch&) = delete;
    FloatScratch& operator=(const FloatScratch&) = delete;
    float* get() const { return p_; }

private:
    float* p_ = nullptr;
    hipStream_t stream_;
};

}  // namespace merge_launch
}  // namespace fimex_amd
