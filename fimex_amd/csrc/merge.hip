// Grid merging: the arithmetic of CDMMerger, that is CDMBorderSmoothing::getDataSlice (src/CDMBorderSmoothing.cc:
// 129-139) with CDMBorderSmoothing_Linear::operator() (src/CDMBorderSmoothing_Linear.cc:41-85) and CDMOverlay::getDataSlice
// (src/CDMOverlay.cc:82-86), between the three regrids of CDMMergerPrivate::makeCDM (src/CDMMerger.cc:212-227).  DESIGN.md 6.8.
//   border_smooth_kernel  S = smooth(I, OI) on a batch of slices, one alias-safe pass
//   overlay_kernel        out = isnan(top) ? base : top, one alias-safe pass
//   merge_smooth_kernel   steps 1 and 2 fused: a lane per inner cell evaluates the outer->inner plan entry only where the smoothing
//                         reads the outer (frame, transition band, undefined inner) and writes S
//   merge_overlay_kernel  steps 3 and 4 fused: a lane per target cell evaluates the inner->target entry on S and the outer->target
//                         entry on O only where S does not reach
// A lane owns one cell of a kTileX x kTileY tile and keeps its class (smoothing) or its plan entries (regrid) in registers over the
// z loop; kAhead slices are in flight per lane (tile, cell and z loop: merge_launch.hpp).  Every slice has its own buffer
// descriptor, so a batch of any length is addressed with 32-bit lane offsets (a slice holds fewer than 2^30 cells, plan.hpp).  The
// plan entries and the stencil arithmetic are those of stencil_math.hpp, the cell classes and the blend those of merge_math.hpp.
// Built with -ffp-contract=off: I + alpha * diff is a multiply and an add, as in the reference.
#include "gather_entry.hpp"
#include "merge_launch.hpp"
#include "merge_math.hpp"
#include "plan.hpp"

#include <cmath>

namespace fimex_amd {

namespace {

using namespace merge_launch;
using FloatPlan = PlanRef<float, 0>;

// CDMBorderSmoothing_Linear::operator() on float interpolation arrays: the cell classes and the blend of merge_math.hpp
using merge_math::SmoothClass;
using merge_math::smooth_class;

__device__ __forceinline__ bool needs_outer(const SmoothClass& c, float inner, bool useOuter) { return merge_math::needs_outer<float>(c, inner, useOuter); }
__device__ __forceinline__ float smooth_value(const SmoothClass& c, float inner, float outer, bool useOuter)
{
    return merge_math::smooth_value<float>(c, inner, outer, useOuter);
}

struct SmoothArgs {
    const float *inner, *outer;  // [nz][ny][nx]
    float* out;
    Tile tile;
    Smoothing sm;
};

// every lane reads its cell of both inputs before it writes it: out may be either of them
__global__ void __launch_bounds__(kBlock) border_smooth_kernel(const SmoothArgs a)
{
    const Cell c(a.tile);
    if (!c.inside) return;
    const SmoothClass cls = smooth_class(c.x, c.y, a.tile.nx, a.tile.ny, a.sm.tw, a.sm.bw);
    const bool useOuter = a.sm.useOuter != 0;
    const uint32_t cb = c.offset<float>();
    for_z_groups<kAhead>(c.z0, c.z1, [&](uint32_t z, auto n) {
        constexpr int N = decltype(n)::value;
        float vi[N], vo[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            vi[k] = ld(c.slice(a.inner, z + k), cb);
            vo[k] = ld(c.slice(a.outer, z + k), cb);
        }
#pragma unroll
        for (int k = 0; k < N; ++k) st_plain(c.slice(a.out, z + k), cb, 0, smooth_value(cls, vi[k], vo[k], useOuter));
    });
}

// CDMOverlay.cc:82-86.  A workgroup takes kAhead * kBlock consecutive values; a lane reads its values before it writes them.
__global__ void __launch_bounds__(kBlock) overlay_kernel(const float* top, const float* base, float* out, size_t n)
{
    const size_t i0 = (size_t)blockIdx.x * (kAhead * kBlock) + threadIdx.x;
    float t[kAhead], b[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
        const size_t i = i0 + (size_t)k * kBlock;
        t[k] = i < n ? top[i] : 0.f;
        b[k] = i < n ? base[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
        const size_t i = i0 + (size_t)k * kBlock;
        if (i < n) out[i] = t[k] != t[k] ? b[k] : t[k];
    }
}

struct MergeSmoothArgs {
    FloatPlan oi;         // outer -> inner grid
    const float *inner;   // [nz][ny][nx]
    const float *outer;   // [nz] source slices of oi
    float* s;             // [nz][ny][nx]
    Tile tile;
    Smoothing sm;
};

// steps 1 and 2: S = smooth(I, regrid(O -> inner grid)), the regrid evaluated only where the smoothing reads it
template <int STENCIL>
__global__ void __launch_bounds__(kBlock) merge_smooth_kernel(const MergeSmoothArgs a)
{
    const Cell c(a.tile);
    if (!c.inside) return;
    const SmoothClass cls = smooth_class(c.x, c.y, a.tile.nx, a.tile.ny, a.sm.tw, a.sm.bw);
    const GatherEntry<STENCIL, float> e = a.oi.entry<STENCIL>(c.cell);
    const bool useOuter = a.sm.useOuter != 0;
    const uint32_t cb = c.offset<float>();
    for_z_groups<kAhead>(c.z0, c.z1, [&](uint32_t z, auto n) {
        constexpr int N = decltype(n)::value;
        float vi[N], vo[N];
#pragma unroll
        for (int k = 0; k < N; ++k) vi[k] = ld(c.slice(a.inner, z + k), cb);
#pragma unroll
        for (int k = 0; k < N; ++k) vo[k] = needs_outer(cls, vi[k], useOuter) ? e.value(a.oi.slice(a.outer, z + k)) : 0.f;
#pragma unroll
        for (int k = 0; k < N; ++k) st_plain(c.slice(a.s, z + k), cb, 0, smooth_value(cls, vi[k], vo[k], useOuter));
    });
}

struct MergeOverlayArgs {
    FloatPlan st;        // smoothed inner -> target
    FloatPlan ot;        // outer -> target
    const float *s;      // [nz] source slices of st
    const float *outer;  // [nz] source slices of ot
    float* out;          // [nz][ny][nx]
    Tile tile;
};

// steps 3 and 4: out = regrid(S -> target) where that is defined, else regrid(O -> target); an invalid inner -> target entry
// issues no load from S, and the outer -> target entry is evaluated only where the first value is NaN
template <int ST, int OT>
__global__ void __launch_bounds__(kBlock) merge_overlay_kernel(const MergeOverlayArgs a)
{
    const Cell c(a.tile);
    if (!c.inside) return;
    const GatherEntry<ST, float> es = a.st.entry<ST>(c.cell);
    const GatherEntry<OT, float> eo = a.ot.entry<OT>(c.cell);
    const uint32_t cb = c.offset<float>();
    for_z_groups<kAhead>(c.z0, c.z1, [&](uint32_t z, auto n) {
        constexpr int N = decltype(n)::value;
        float v[N];
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = es.value(a.st.slice(a.s, z + k));
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (v[k] != v[k]) v[k] = eo.value(a.ot.slice(a.outer, z + k));
#pragma unroll
        for (int k = 0; k < N; ++k) st_stream(c.slice(a.out, z + k), cb, 0, v[k]);
    });
}

}  // namespace

// every argument has been checked (capi.hip)
void launch_border_smooth(const float* d_inner, const float* d_outerOnInner, float* d_out, size_t nx, size_t ny, size_t nz, size_t transitionWidth,
                          size_t borderWidth, bool useOuter, hipStream_t stream)
{
    if (nz == 0) return;
    SmoothArgs a{d_inner, d_outerOnInner, d_out, {}, smoothing(transitionWidth, borderWidth, useOuter)};
    const dim3 grid = tile_grid(nx, ny, nz, a.tile);
    border_smooth_kernel<<<grid, tile_block(), 0, stream>>>(a);
    FA_HIP(hipGetLastError());
}

void launch_overlay(const float* d_top, const float* d_base, float* d_out, size_t n, hipStream_t stream)
{
    if (n == 0) return;
    const size_t blocks = ceil_div(n, (size_t)kAhead * kBlock);
    FA_REQUIRE(blocks <= 0x7fffffffu, "too many values for one launch");
    overlay_kernel<<<(uint32_t)blocks, kBlock, 0, stream>>>(d_top, d_base, d_out, n);
    FA_HIP(hipGetLastError());
}

void launch_merge_fused(const fimex_amd_merge_plan& m, const float* d_inner, const float* d_outer, size_t nz, float* d_out, hipStream_t stream)
{
    if (nz == 0) return;
    const fimex_amd_regrid_plan &oi = *m.outerToInner, &st = *m.innerToTarget, &ot = *m.outerToTarget;
    Scratch s(nz * oi.outX * oi.outY * sizeof(float), stream);
    {
        MergeSmoothArgs a{plan_ref<float>(oi), d_inner, d_outer, s.get<float>(), {}, smoothing(m.transitionWidth, m.borderWidth, m.useOuter)};
        const dim3 grid = tile_grid(oi.outX, oi.outY, nz, a.tile);
        with_stencil(oi, [&](auto stencil) { merge_smooth_kernel<decltype(stencil)::value><<<grid, tile_block(), 0, stream>>>(a); });
        FA_HIP(hipGetLastError());
    }
    MergeOverlayArgs a{plan_ref<float>(st), plan_ref<float>(ot), s.get<float>(), d_outer, d_out, {}};
    const dim3 grid = tile_grid(st.outX, st.outY, nz, a.tile);
    with_stencil(st, [&](auto sts) {
        with_stencil(ot, [&](auto ots) { merge_overlay_kernel<decltype(sts)::value, decltype(ots)::value><<<grid, tile_block(), 0, stream>>>(a); });
    });
    FA_HIP(hipGetLastError());
}

// The same four steps as the reference runs them: three full applies and the two elementwise kernels on temporaries
void launch_merge_chain(const fimex_amd_merge_plan& m, const float* d_inner, const float* d_outer, size_t nz, float* d_out, hipStream_t stream)
{
    if (nz == 0) return;
    const fimex_amd_regrid_plan &oi = *m.outerToInner, &st = *m.innerToTarget, &ot = *m.outerToTarget;
    const size_t innerCells = oi.outX * oi.outY, targetCells = st.outX * st.outY;
    Scratch sBytes(nz * innerCells * sizeof(float), stream), topBytes(nz * targetCells * sizeof(float), stream);
    float *s = sBytes.get<float>(), *top = topBytes.get<float>();
    apply_plan_device(oi, d_outer, nz, s, stream);                                                               // step 1
    launch_border_smooth(d_inner, s, s, oi.outX, oi.outY, nz, m.transitionWidth, m.borderWidth, m.useOuter, stream);  // step 2
    apply_plan_device(st, s, nz, top, stream);                                                                   // step 3
    apply_plan_device(ot, d_outer, nz, d_out, stream);
    launch_overlay(top, d_out, d_out, nz * targetCells, stream);                                                 // step 4
}

}  // namespace fimex_amd
