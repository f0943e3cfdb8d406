// Backward-mapping regrid for gfx950, the per-lane gather kernels: nearest / bilinear / bicubic on float slices and on a
// variable's stored type.  Short batches, plans without a staged form and int32 slices take them (backward_plan.hip chooses).
//
// Replaces the per-cell function-pointer loop of CachedInterpolation::interpolateValues
// (src/CachedInterpolation.cc:118-147) around mifi_get_values_f / _bilinear_f / _bicubic_f
// (src/interpolation.c:862-1028).
//
// Mapping to the machine (HBM-bound gather, no MFMA):
//  * one lane per output cell, 256-lane workgroups over 256 consecutive output cells, so every
//    store instruction of a wave writes 256 contiguous bytes and neighbouring lanes gather from
//    neighbouring source cells (the same few 128-B lines);
//  * the z loop (time x level slices) runs inside the lane: the plan entry is read once and kept
//    in registers, and ZC slices are in flight per lane (4*ZC independent loads for bilinear)
//    to cover HBM latency;
//  * workgroups are dealt round-robin over the 8 XCDs, each with a private L2; the tile index is
//    remapped so that one XCD owns a contiguous band of output rows and the source rows shared by
//    vertically adjacent tiles are fetched into one L2 only;
//  * outputs are written once and never re-read: non-temporal stores keep them out of the way of
//    the source lines in L2.
//
// Built with -ffp-contract=off: every multiply and add is a separate IEEE operation in
// the same type and order as the reference, so results are bit-identical to the CPU path.
#include "gather_entry.hpp"
#include "plan.hpp"

#include <algorithm>
#include <type_traits>

namespace fimex_amd {

namespace {

struct ApplyArgs {
    const void* in;
    void* out;
    uint32_t nOut;         // cells per output slice
    uint32_t ix;           // source row length
    size_t inLayer;        // cells per source slice
    uint32_t nz;
    uint32_t zPerBlock;    // slices handled by one workgroup (blockIdx.y selects the chunk)
    uint32_t nTiles;       // workgroup-sized tiles per slice
    uint32_t tilesPerXcd;  // ceil(nTiles / 8)
    uint32_t outX, outY;   // output grid
    uint32_t tilesX;       // tiles per output row
    uint32_t tileWLog2;    // tile = 2^tileWLog2 x (256 >> tileWLog2) output cells, lanes row-major inside it
    uint32_t xcdRemap;     // 1: contiguous band of tiles per XCD
};

// blockIdx.x -> tile so that each XCD (blockIdx.x % 8 under round-robin dispatch) works on a
// contiguous band of the output.  Placement only affects speed, never results.
__device__ __forceinline__ bool tile_cell(const ApplyArgs& a, uint32_t& cell)
{
    const uint32_t b = blockIdx.x;
    const uint32_t tile = a.xcdRemap ? (b % kXcds) * a.tilesPerXcd + b / kXcds : b;
    if (tile >= a.nTiles) return false;
    const uint32_t tx = tile % a.tilesX, ty = tile / a.tilesX;
    const uint32_t x = (tx << a.tileWLog2) + (threadIdx.x & ((1u << a.tileWLog2) - 1));
    const uint32_t y = ty * (kBlock >> a.tileWLog2) + (threadIdx.x >> a.tileWLog2);
    cell = y * a.outX + x;
    return x < a.outX && y < a.outY;
}

// STENCIL 1 nearest, 2 bilinear, 4 bicubic, on slices of T (gather_entry.hpp).  A z chunk is walked with ZC slices in flight behind
// one descriptor (a chunk of ZC slices must span < 4 GiB, checked on the host), then slice by slice.  A bilinear border entry has
// zero steps for the neighbours it lacks (src/interpolation.c:903-948) and takes the same loop as an interior one.
template <int STENCIL, int ZC, typename T, bool NT = true>
__global__ void __launch_bounds__(kBlock) gather_apply(ApplyArgs a, typename Element<T>::Params elementParams, const uint32_t* __restrict__ pos,
                                                       const frac_t<STENCIL>* __restrict__ xfrac, const frac_t<STENCIL>* __restrict__ yfrac)
{
    uint32_t cell;
    if (!tile_cell(a, cell)) return;
    const uint32_t z0 = blockIdx.y * a.zPerBlock;
    const uint32_t z1 = min(a.nz, z0 + a.zPerBlock);
    const Element<T> el(elementParams);
    const GatherEntry<STENCIL, T> e(pos[cell], STENCIL == 1 ? 0 : xfrac[cell], STENCIL == 1 ? 0 : yfrac[cell], a.ix, el);
    const uint32_t inBytes = (uint32_t)a.inLayer * (uint32_t)sizeof(T), outBytes = a.nOut * (uint32_t)sizeof(T), cb = cell * (uint32_t)sizeof(T);
    const char* src = static_cast<const char*>(a.in) + (size_t)z0 * inBytes;
    char* o = static_cast<char*>(a.out) + (size_t)z0 * outBytes;
    uint32_t z = z0;
    if (!e.valid()) {
        for (; z < z1; ++z, o += outBytes) el.store(make_rsrc(o, outBytes), cb, 0, undefined_f());
        return;
    }
    for (; z + ZC <= z1; z += ZC, src += (size_t)ZC * inBytes, o += (size_t)ZC * outBytes) {
        const rsrc_t rs = make_rsrc(src, inBytes * ZC), ro = make_rsrc(o, outBytes * ZC);
        float taps[ZC][STENCIL][STENCIL];
#pragma unroll
        for (int k = 0; k < ZC; ++k) e.fetch(rs, inBytes * k, taps[k]);
#pragma unroll
        for (int k = 0; k < ZC; ++k) el.template store<NT>(ro, cb, outBytes * k, e.combine(taps[k]));
    }
    for (; z < z1; ++z, src += inBytes, o += outBytes) el.store(make_rsrc(o, outBytes), cb, 0, e.value(make_rsrc(src, inBytes)));
}

// ONE slice per call: one time step of a variable without levels, the reference's call pattern for surface fields
// (src/CDMInterpolator.cc:251-259).  There is no slice loop to keep loads in flight across, and a lane with
// one output cell spends its life in two dependent round trips to memory (plan entry, then stencil).  Here a lane takes CELLS
// output cells of a 64 x (4 * CELLS) tile (rows y, y + 4, ...): the plan entries of all of them are loaded first, then all
// their stencil values -- four times the bytes in flight per lane; border and undefined cells are computed by selection
// (every form evaluated, src/interpolation.c:899-948; the loads of an undefined entry are dropped), so that no lane leaves the
// common path.  STENCIL 1: nearest (:869-876).
template <int STENCIL, int CELLS>
__global__ void __launch_bounds__(kBlock) apply_few(ApplyArgs a, const uint32_t* __restrict__ pos, const float* __restrict__ xfrac,
                                                    const float* __restrict__ yfrac, uint32_t tilesX, uint32_t nTiles, uint32_t tilesPerXcd)
{
    const uint32_t b = blockIdx.x;
    const uint32_t tile = (b % kXcds) * tilesPerXcd + b / kXcds;  // a contiguous band of tile rows per XCD
    if (tile >= nTiles) return;
    const uint32_t tx = tile % tilesX, ty = tile / tilesX;
    const uint32_t x = tx * 64u + (threadIdx.x & 63u);
    const uint32_t y0 = ty * (4u * CELLS) + (threadIdx.x >> 6);
    uint32_t cb[CELLS];
    GatherEntry<STENCIL, float> e[CELLS];
#pragma unroll
    for (int k = 0; k < CELLS; ++k) {
        const uint32_t y = y0 + 4u * k;
        const bool mine = x < a.outX && y < a.outY;
        const uint32_t cell = y * a.outX + x;
        cb[k] = mine ? cell * 4u : 0xFFFFFFFFu;  // beyond the slice: the store is dropped
        e[k] = GatherEntry<STENCIL, float>(mine ? pos[cell] : kInvalidPos, (mine && STENCIL == 2) ? xfrac[cell] : 0.f,
                                           (mine && STENCIL == 2) ? yfrac[cell] : 0.f, a.ix);
    }
    const uint32_t inBytes = (uint32_t)a.inLayer * 4u, outBytes = a.nOut * 4u;
    for (uint32_t z = 0; z < a.nz; ++z) {
        const rsrc_t rs = make_rsrc(static_cast<const float*>(a.in) + (size_t)z * a.inLayer, inBytes);
        const rsrc_t ro = make_rsrc(static_cast<float*>(a.out) + (size_t)z * a.nOut, outBytes);
        float taps[CELLS][STENCIL][STENCIL];
#pragma unroll
        for (int k = 0; k < CELLS; ++k) e[k].fetch(rs, 0, taps[k]);
#pragma unroll
        for (int k = 0; k < CELLS; ++k) st_stream(ro, cb[k], 0, e[k].combine(taps[k]));
    }
}

ApplyArgs make_args(const fimex_amd_regrid_plan& plan, const void* d_in, size_t nz, void* d_out, dim3& grid)
{
    ApplyArgs a{};
    a.in = d_in;
    a.out = d_out;
    a.nOut = (uint32_t)(plan.outX * plan.outY);
    a.ix = (uint32_t)plan.inX;
    a.inLayer = plan.inX * plan.inY;
    a.nz = (uint32_t)nz;
    a.outX = (uint32_t)plan.outX;
    a.outY = (uint32_t)plan.outY;
    // tile shape: 2^k x (256 >> k) output cells per workgroup
    uint32_t k = (uint32_t)tuning("TILEW_LOG2", 6);
    if (k > 8) k = 8;
    a.tileWLog2 = k;
    a.tilesX = (uint32_t)ceil_div(plan.outX, (size_t)1 << k);
    a.nTiles = a.tilesX * (uint32_t)ceil_div(plan.outY, (size_t)(kBlock >> k));
    a.xcdRemap = tuning("XCD", 1) ? 1 : 0;
    a.tilesPerXcd = (uint32_t)ceil_div(a.nTiles, kXcds);
    // slices per workgroup: long enough to amortise the plan read, short enough that the grid
    // still holds several waves of workgroups per CU
    uint32_t zpb = (uint32_t)tuning("ZPB", 0);
    if (zpb == 0) {
        const size_t wantBlocks = 256 * 8 * 4;
        size_t chunks = ceil_div(wantBlocks, (size_t)a.nTiles);
        if (chunks > nz) chunks = nz;
        if (chunks < 1) chunks = 1;
        zpb = (uint32_t)ceil_div(nz, chunks);
        const uint32_t zpbMax = (uint32_t)tuning("ZPB_MAX", 40);
        if (zpb > zpbMax) zpb = zpbMax;
    }
    if (zpb > nz) zpb = (uint32_t)nz;
    a.zPerBlock = zpb;
    const size_t chunks = ceil_div(nz, (size_t)zpb);
    FA_REQUIRE(chunks <= 65535, "too many z chunks for one launch");
    grid = dim3(a.tilesPerXcd * kXcds, (uint32_t)chunks, 1);
    return a;
}

// the plan's fractions in the type the stencil reads: xf / yf, xfd / yfd, none for nearest
template <int STENCIL>
const frac_t<STENCIL>* fractions(const fimex_amd_regrid_plan& plan, bool y)
{
    if constexpr (STENCIL == 4) return y ? plan.yfd.get() : plan.xfd.get();
    else if constexpr (STENCIL == 2) return y ? plan.yf.get() : plan.xf.get();
    else return nullptr;
}

template <int STENCIL, int ZC, typename T, bool NT = true>
void launch_gather(const fimex_amd_regrid_plan& plan, const ApplyArgs& a, typename Element<T>::Params ep, dim3 grid, hipStream_t stream)
{
    gather_apply<STENCIL, ZC, T, NT><<<grid, kBlock, 0, stream>>>(a, ep, plan.pos.get(), fractions<STENCIL>(plan, false), fractions<STENCIL>(plan, true));
}

template <typename T>
void launch_typed_t(const fimex_amd_regrid_plan& plan, const ApplyArgs& a, typename Element<T>::Params ep, dim3 grid, hipStream_t stream)
{
    switch (plan.kind) {  // 8 slices behind one descriptor (checked by the caller); bicubic: 16 loads per slice, one slice at a time
    case PlanKind::Nearest: launch_gather<1, 8, T>(plan, a, ep, grid, stream); break;
    case PlanKind::Bilinear: launch_gather<2, 8, T>(plan, a, ep, grid, stream); break;
    case PlanKind::Bicubic: launch_gather<4, 1, T>(plan, a, ep, grid, stream); break;
    default: throw Error("typed apply: not a backward plan");
    }
    FA_HIP(hipGetLastError());
}

}  // namespace

// The per-lane gather kernels on any backward plan (short batches, plans without a staged form, and the cross-check of
// fimex_amd_regrid_apply_gather_device).
void launch_backward_gather(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, float* d_out, hipStream_t stream)
{
    if (nz == 0) return;
    FA_REQUIRE(nz <= 0xFFFFFFFFu, "too many slices");
    dim3 grid;
    const ApplyArgs a = make_args(plan, d_in, nz, d_out, grid);
    if (nz == 1 && plan.kind != PlanKind::Bicubic && tuning("FEW", 1) != 0) {
        // one slice: several output cells per lane (apply_few).  Measured cold, a different slice pair every call
        // (profiles/r03_sweep_few_cells*.log): 2 / 4 / 8 cells per lane 24.4 / 25.5 / 28.0 us against 29.4 us for one cell per lane;
        // with two or three slices the kernel above, which keeps the slices of a cell in flight together, is ahead again
        // (40.4 against 42 us, 52 against 59 us).
        const int cells = tuning("FEW_CELLS", 2);
        auto go = [&](auto cellsTag) {
            constexpr int kCells = decltype(cellsTag)::value;
            const uint32_t tilesX = (uint32_t)ceil_div(plan.outX, (size_t)64), tilesY = (uint32_t)ceil_div(plan.outY, (size_t)(4 * kCells));
            const uint32_t nTiles = tilesX * tilesY, perXcd = (uint32_t)ceil_div(nTiles, kXcds);
            const dim3 g(perXcd * kXcds);
            if (plan.kind == PlanKind::Nearest) apply_few<1, kCells><<<g, kBlock, 0, stream>>>(a, plan.pos.get(), nullptr, nullptr, tilesX, nTiles, perXcd);
            else apply_few<2, kCells><<<g, kBlock, 0, stream>>>(a, plan.pos.get(), plan.xf.get(), plan.yf.get(), tilesX, nTiles, perXcd);
        };
        if (cells == 2) go(std::integral_constant<int, 2>());
        else if (cells == 8) go(std::integral_constant<int, 8>());
        else go(std::integral_constant<int, 4>());
        FA_HIP(hipGetLastError());
        return;
    }
    // a chunk of ZC slices is addressed through one 32-bit buffer range: fall back to ZC = 1 for huge slices
    const size_t sliceBytes = 4 * (a.inLayer > a.nOut ? a.inLayer : (size_t)a.nOut);
    auto fits = [&](size_t zc) { return sliceBytes * zc <= 0xFFFFFFFFull; };
    const Element<float>::Params ep;
    switch (plan.kind) {
    case PlanKind::Nearest:
        if (fits(16)) launch_gather<1, 16, float>(plan, a, ep, grid, stream);
        else launch_gather<1, 1, float>(plan, a, ep, grid, stream);
        break;
    case PlanKind::Bilinear: {
        const int zc = tuning("BILINEAR_ZC", 8);
        const bool nt = tuning("NT", 1) != 0;
        if (zc >= 16 && fits(16)) {
            if (nt) launch_gather<2, 16, float, true>(plan, a, ep, grid, stream);
            else launch_gather<2, 16, float, false>(plan, a, ep, grid, stream);
        } else if (zc >= 8 && fits(8)) {
            if (nt) launch_gather<2, 8, float, true>(plan, a, ep, grid, stream);
            else launch_gather<2, 8, float, false>(plan, a, ep, grid, stream);
        } else if (zc >= 4 && fits(4)) {
            if (nt) launch_gather<2, 4, float, true>(plan, a, ep, grid, stream);
            else launch_gather<2, 4, float, false>(plan, a, ep, grid, stream);
        } else if (zc >= 2 && fits(2)) {
            launch_gather<2, 2, float>(plan, a, ep, grid, stream);
        } else {
            launch_gather<2, 1, float>(plan, a, ep, grid, stream);
        }
        break;
    }
    case PlanKind::Bicubic:
        if (fits(2)) launch_gather<4, 2, float>(plan, a, ep, grid, stream);
        else launch_gather<4, 1, float>(plan, a, ep, grid, stream);
        break;
    default:
        throw Error("launch_backward_apply: not a backward plan");
    }
    FA_HIP(hipGetLastError());
}

// The same kernel on a variable's stored type, for 1- and 2-byte integer types and int32 (everything else runs the three-pass
// sequence: to float, regrid, from float).
void launch_typed_gather(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double badValue, void* d_out,
                         hipStream_t stream)
{
    if (nz == 0) return;
    FA_REQUIRE(nz <= 0xFFFFFFFFu, "too many slices");
    FA_REQUIRE((dispatch::staged_elem_bytes(cdmType) != 0 || cdmType == FIMEX_AMD_CDM_INT) &&
                   8 * 4 * std::max(plan.inX * plan.inY, plan.outX * plan.outY) <= 0xFFFFFFFFull,  // 8 slices behind one descriptor
               "typed gather: not a call of this kernel (typed_gather, backward_dispatch.hpp)");
    dim3 grid;
    const ApplyArgs a = make_args(plan, d_in, nz, d_out, grid);
    const float bad = (float)badValue;
    auto go = [&](auto t) {
        using T = decltype(t);
        launch_typed_t<T>(plan, a, typename Element<T>::Params{bad, !(bad != bad), badValue}, grid, stream);
    };
    switch (cdmType) {
    case FIMEX_AMD_CDM_CHAR: go((signed char)0); break;
    case FIMEX_AMD_CDM_UCHAR: go((unsigned char)0); break;
    case FIMEX_AMD_CDM_SHORT: go((short)0); break;
    case FIMEX_AMD_CDM_USHORT: go((unsigned short)0); break;
    default: go((int)0); break;
    }
}

}  // namespace fimex_amd
