// The shell of the merge kernels on float arrays (merge.hip), on stored types (merge_typed.hip), on float vector pairs
// (merge_vector.hip) and on packed vector pairs (merge_vector_typed.hip).  Host side: the tile of a workgroup, the grid over tiles
// and chunks of slices, the tile and smoothing arguments, the stencil dispatch, a backward plan's arrays as kernel arguments and the
// call's scratch.  Device side: a lane's cell and z chunk, the z loop over groups of slices in flight, and a rotation's lazy read.
// Each of the four files keeps its argument structs, its loads and stores, its call into its *_math.hpp, its dispatch rule and
// its chain.
#pragma once

#include "gather_entry.hpp"
#include "plan.hpp"

#include <type_traits>

namespace fimex_amd {
namespace merge_launch {

constexpr int kTileX = 64, kTileY = 4;  // a wave per row
static_assert(kTileX * kTileY == kBlock, "a tile is one workgroup");
constexpr int kAhead = 4;               // slices whose loads are in flight together

// pair-slices in flight per lane of the kernels on a vector pair: a bicubic entry holds 2 x 16 taps per pair-slice and combines
// them in double
template <int STENCIL>
constexpr int ahead_of() { return STENCIL == 4 ? 1 : STENCIL == 2 ? 2 : 4; }
static_assert(kAhead % ahead_of<1>() == 0 && kAhead % ahead_of<2>() == 0, "a z chunk is a whole number of groups");

// ---- kernel arguments every tile kernel has, and the smoothing kernels' own
struct Tile {
    uint32_t nx, ny, nz, zPerBlock;
};
struct Smoothing {
    uint64_t tw, bw;
    int useOuter;
};
inline Smoothing smoothing(size_t transitionWidth, size_t borderWidth, bool useOuter) { return {transitionWidth, borderWidth, useOuter ? 1 : 0}; }

// tiles of one slice in x and y, chunks of slices in z: enough workgroups to fill the device, chunks long enough to amortise the
// per-cell set-up (class, plan entries)
inline dim3 tile_grid(size_t nx, size_t ny, size_t nz, Tile& t)
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
    t = {(uint32_t)nx, (uint32_t)ny, (uint32_t)nz, (uint32_t)zpb};
    return dim3((uint32_t)tilesX, (uint32_t)tilesY, (uint32_t)ceil_div(nz, zpb));
}
inline dim3 tile_block() { return dim3(kTileX, kTileY, 1); }

// f(std::integral_constant<int, S>) with S the stencil size of a backward plan
template <typename F>
void with_stencil(const fimex_amd_regrid_plan& p, F&& f)
{
    switch (p.kind) {
    case PlanKind::Nearest: return f(std::integral_constant<int, 1>());
    case PlanKind::Bilinear: return f(std::integral_constant<int, 2>());
    case PlanKind::Bicubic: return f(std::integral_constant<int, 4>());
    default: throw Error("merge: not a backward plan");
    }
}

// ---- a backward plan's arrays on slices of T; an entry is decoded once per cell and evaluated slice by slice (gather_entry.hpp:
// an undefined entry issues loads that are dropped and gives NaN, so the lane stays on the common path)
struct PlanArrays {
    const uint32_t* pos;
    const float *xf, *yf;
    const double *xfd, *yfd;
    uint32_t ix;       // source row length
    uint32_t inBytes;  // bytes of a source slice
    size_t inLayer;    // cells of a source slice
};
// the source's fill value as data2InterpolationArray takes it, per field read through the plan: none for float slices, one for a
// scalar stored type, two (u, v) for a pair, whose entries differ in their Element<T> only
template <typename T, int FIELDS>
struct ElementParams {
    typename Element<T>::Params p[FIELDS];
    __device__ __forceinline__ Element<T> element(int k) const { return Element<T>(p[k]); }
};
template <typename T>
struct ElementParams<T, 0> {
    __device__ __forceinline__ Element<T> element(int) const { return Element<T>(); }
};

template <typename T, int FIELDS>
struct PlanRef : PlanArrays, ElementParams<T, FIELDS> {
    template <int STENCIL>
    __device__ __forceinline__ GatherEntry<STENCIL, T> entry(uint32_t cell) const
    {
        const Element<T> e = this->element(0);
        if constexpr (STENCIL == 4) return {pos[cell], xfd[cell], yfd[cell], ix, e};
        else if constexpr (STENCIL == 2) return {pos[cell], xf[cell], yf[cell], ix, e};
        else return {pos[cell], 0.f, 0.f, ix, e};
    }
    // the decoded entry of the pair's first field with the second field's element
    template <int STENCIL>
    __device__ __forceinline__ GatherEntry<STENCIL, T> second(GatherEntry<STENCIL, T> u) const
    {
        u.el = this->element(1);
        return u;
    }
    __device__ __forceinline__ rsrc_t slice(const T* in, uint32_t z) const { return make_rsrc(in + (size_t)z * inLayer, inBytes); }
};
static_assert(sizeof(PlanRef<float, 0>) == sizeof(PlanArrays), "a plan on float slices carries no element parameters");

// the element parameters are those of launch_typed_gather: the fill value narrowed to float, none where that is NaN
template <typename T>
typename Element<T>::Params element_params(double fill)
{
    const float bad = (float)fill;
    return typename Element<T>::Params{bad, !(bad != bad), fill};
}

// fills: the fill value of every field read through the plan
template <typename T, typename... Fill>
PlanRef<T, (int)sizeof...(Fill)> plan_ref(const fimex_amd_regrid_plan& p, Fill... fills)
{
    PlanRef<T, (int)sizeof...(Fill)> r{};
    static_cast<PlanArrays&>(r) = {p.pos.get(), p.xf.get(), p.yf.get(), p.xfd.get(), p.yfd.get(), (uint32_t)p.inX, (uint32_t)(p.inX * p.inY * sizeof(T)),
                                   p.inX * p.inY};
    if constexpr (sizeof...(Fill) > 0) {
        int k = 0;
        ((r.p[k++] = element_params<T>(fills)), ...);
    }
    return r;
}

// stream-ordered scratch of one call, freed on the stream behind the kernels that use it
class Scratch {
public:
    Scratch(size_t bytes, hipStream_t stream) : stream_(stream)
    {
        if (bytes) FA_HIP(hipMallocAsync(&p_, bytes, stream));
    }
    ~Scratch() { if (p_) (void)hipFreeAsync(p_, stream_); }
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    template <typename T = void>
    T* get() const { return static_cast<T*>(p_); }

private:
    void* p_ = nullptr;
    hipStream_t stream_;
};

inline bool aligned_to(const void* p, size_t elem) { return reinterpret_cast<uintptr_t>(p) % elem == 0; }

// ---- device side
// a lane's cell of its tile and its chunk of slices
struct Cell {
    uint32_t x, y, cell, z0, z1;
    size_t plane;  // cells of a slice
    bool inside;
    __device__ __forceinline__ explicit Cell(const Tile& t)
        : x(blockIdx.x * kTileX + threadIdx.x), y(blockIdx.y * kTileY + threadIdx.y), cell(y * t.nx + x), z0(blockIdx.z * t.zPerBlock),
          z1(min(t.nz, z0 + t.zPerBlock)), plane((size_t)t.nx * t.ny), inside(x < t.nx && y < t.ny)
    {
    }
    // the lane's byte offset in a slice of T, and the slice's buffer descriptor
    template <typename T>
    __device__ __forceinline__ uint32_t offset() const { return cell * (uint32_t)sizeof(T); }
    template <typename T>
    __device__ __forceinline__ rsrc_t slice(const T* field, uint32_t z) const { return make_rsrc(field + (size_t)z * plane, (uint32_t)plane * (uint32_t)sizeof(T)); }
};

// body(z, std::integral_constant<int, N>) on the slices [z, z + N) for whole groups of AHEAD slices, then slice by slice
template <int AHEAD, typename Body>
__device__ __forceinline__ void for_z_groups(uint32_t z, uint32_t z1, Body&& body)
{
    for (; z + AHEAD <= z1; z += AHEAD) body(z, std::integral_constant<int, AHEAD>());
    if constexpr (AHEAD > 1)
        for (; z < z1; ++z) body(z, std::integral_constant<int, 1>());
}

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

}  // namespace merge_launch
}  // namespace fimex_amd
