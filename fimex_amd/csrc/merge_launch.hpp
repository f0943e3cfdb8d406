// Launch geometry shared by the merge kernels on float arrays (merge.hip) and on stored types (merge_typed.hip): the tile of a
// workgroup, the slices in flight per lane, the grid over tiles and chunks of slices, and the stencil size of a backward plan.
#pragma once

#include "plan.hpp"

namespace fimex_amd {
namespace merge_launch {

constexpr int kTileX = 64, kTileY = 4;  // a wave per row
static_assert(kTileX * kTileY == kBlock, "a tile is one workgroup");
constexpr int kAhead = 4;               // slices whose loads are in flight together

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

}  // namespace merge_launch
}  // namespace fimex_amd
