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
// z loop; kAhead slices are in flight per lane.  Every slice has its own buffer descriptor, so a batch of any length is addressed
// with 32-bit lane offsets (a slice holds fewer than 2^30 cells, plan.hpp).  The plan entries and the stencil arithmetic are those
// of stencil_math.hpp, the cell classes and the blend those of merge_math.hpp.  Built with -ffp-contract=off: I + alpha * diff is a
// multiply and an add, as in the reference.
#include "gather_entry.hpp"
#include "merge_launch.hpp"
#include "merge_math.hpp"
#include "plan.hpp"

#include <cmath>

namespace fimex_amd {

namespace {

using merge_launch::FloatScratch;
using merge_launch::kAhead;
using merge_launch::kTileX;
using merge_launch::kTileY;
using merge_launch::plan_ref;
using merge_launch::PlanRef;
using merge_launch::stencil_of;
using merge_launch::tile_grid;

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
    uint32_t nx, ny, nz, zPerBlock;
    uint64_t tw, bw;
    int useOuter;
};

// every lane reads its cell of both inputs before it writes it: out may be either of them
__global__ void __launch_bounds__(kBlock) border_smooth_kernel(const SmoothArgs a)
{
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= a.nx || y >= a.ny) return;
    const SmoothClass c = smooth_class(x, y, a.nx, a.ny, a.tw, a.bw);
    const bool useOuter = a.useOuter != 0;
    const size_t plane = (size_t)a.nx * a.ny;
    const uint32_t planeBytes = (uint32_t)plane * 4u, cb = (y * a.nx + x) * 4u;
    uint32_t z = blockIdx.z * a.zPerBlock;
    const uint32_t z1 = min(a.nz, z + a.zPerBlock);
    for (; z + kAhead <= z1; z += kAhead) {
        float vi[kAhead], vo[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            vi[k] = ld(make_rsrc(a.inner + (size_t)(z + k) * plane, planeBytes), cb);
            vo[k] = ld(make_rsrc(a.outer + (size_t)(z + k) * plane, planeBytes), cb);
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) st_plain(make_rsrc(a.out + (size_t)(z + k) * plane, planeBytes), cb, 0, smooth_value(c, vi[k], vo[k], useOuter));
    }
    for (; z < z1; ++z) {
        const float vi = ld(make_rsrc(a.inner + (size_t)z * plane, planeBytes), cb), vo = ld(make_rsrc(a.outer + (size_t)z * plane, planeBytes), cb);
        st_plain(make_rsrc(a.out + (size_t)z * plane, planeBytes), cb, 0, smooth_value(c, vi, vo, useOuter));
    }
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
    PlanRef oi;           // outer -> inner grid
    const float *inner;   // [nz][ny][nx]
    const float *outer;   // [nz] source slices of oi
    float* s;             // [nz][ny][nx]
    uint32_t nx, ny, nz, zPerBlock;
    uint64_t tw, bw;
    int useOuter;
};

// steps 1 and 2: S = smooth(I, regrid(O -> inner grid)), the regrid evaluated only where the smoothing reads it
template <int STENCIL>
__global__ void __launch_bounds__(kBlock) merge_smooth_kernel(const MergeSmoothArgs a)
{
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= a.nx || y >= a.ny) return;
    const uint32_t cell = y * a.nx + x, cb = cell * 4u;
    const SmoothClass c = smooth_class(x, y, a.nx, a.ny, a.tw, a.bw);
    const GatherEntry<STENCIL, float> e = a.oi.entry<STENCIL>(cell);
    const bool useOuter = a.useOuter != 0;
    const size_t plane = (size_t)a.nx * a.ny;
    const uint32_t planeBytes = (uint32_t)plane * 4u;
    uint32_t z = blockIdx.z * a.zPerBlock;
    const uint32_t z1 = min(a.nz, z + a.zPerBlock);
    for (; z + kAhead <= z1; z += kAhead) {
        float vi[kAhead], vo[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) vi[k] = ld(make_rsrc(a.inner + (size_t)(z + k) * plane, planeBytes), cb);
#pragma unroll
        for (int k = 0; k < kAhead; ++k)
            vo[k] = needs_outer(c, vi[k], useOuter) ? e.value(make_rsrc(a.outer + (size_t)(z + k) * a.oi.inLayer, a.oi.inBytes)) : 0.f;
#pragma unroll
        for (int k = 0; k < kAhead; ++k) st_plain(make_rsrc(a.s + (size_t)(z + k) * plane, planeBytes), cb, 0, smooth_value(c, vi[k], vo[k], useOuter));
    }
    for (; z < z1; ++z) {
        const float vi = ld(make_rsrc(a.inner + (size_t)z * plane, planeBytes), cb);
        const float vo = needs_outer(c, vi, useOuter) ? e.value(make_rsrc(a.outer + (size_t)z * a.oi.inLayer, a.oi.inBytes)) : 0.f;
        st_plain(make_rsrc(a.s + (size_t)z * plane, planeBytes), cb, 0, smooth_value(c, vi, vo, useOuter));
    }
}

struct MergeOverlayArgs {
    PlanRef st;          // smoothed inner -> target
    PlanRef ot;          // outer -> target
    const float *s;      // [nz] source slices of st
    const float *outer;  // [nz] source slices of ot
    float* out;          // [nz][ny][nx]
    uint32_t nx, ny, nz, zPerBlock;
};

// steps 3 and 4: out = regrid(S -> target) where that is defined, else regrid(O -> target); an invalid inner -> target entry
// issues no load from S, and the outer -> target entry is evaluated only where the first value is NaN
template <int ST, int OT>
__global__ void __launch_bounds__(kBlock) merge_overlay_kernel(const MergeOverlayArgs a)
{
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= a.nx || y >= a.ny) return;
    const uint32_t cell = y * a.nx + x, cb = cell * 4u;
    const GatherEntry<ST, float> es = a.st.entry<ST>(cell);
    const GatherEntry<OT, float> eo = a.ot.entry<OT>(cell);
    const size_t plane = (size_t)a.nx * a.ny;
    const uint32_t planeBytes = (uint32_t)plane * 4u;
    uint32_t z = blockIdx.z * a.zPerBlock;
    const uint32_t z1 = min(a.nz, z + a.zPerBlock);
    for (; z + kAhead <= z1; z += kAhead) {
        float v[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) v[k] = es.value(make_rsrc(a.s + (size_t)(z + k) * a.st.inLayer, a.st.inBytes));
#pragma unroll
        for (int k = 0; k < kAhead; ++k)
            if (v[k] != v[k]) v[k] = eo.value(make_rsrc(a.outer + (size_t)(z + k) * a.ot.inLayer, a.ot.inBytes));
#pragma unroll
        for (int k = 0; k < kAhead; ++k) st_stream(make_rsrc(a.out + (size_t)(z + k) * plane, planeBytes), cb, 0, v[k]);
    }
    for (; z < z1; ++z) {
        float v = es.value(make_rsrc(a.s + (size_t)z * a.st.inLayer, a.st.inBytes));
        if (v != v) v = eo.value(make_rsrc(a.outer + (size_t)z * a.ot.inLayer, a.ot.inBytes));
        st_stream(make_rsrc(a.out + (size_t)z * plane, planeBytes), cb, 0, v);
    }
}

template <int ST>
void launch_overlay_st(int ot, dim3 grid, const MergeOverlayArgs& a, hipStream_t stream)
{
    const dim3 block(kTileX, kTileY, 1);
    if (ot == 1) merge_overlay_kernel<ST, 1><<<grid, block, 0, stream>>>(a);
    else if (ot == 2) merge_overlay_kernel<ST, 2><<<grid, block, 0, stream>>>(a);
    else merge_overlay_kernel<ST, 4><<<grid, block, 0, stream>>>(a);
}

}  // namespace

// every argument has been checked (capi.hip)
void launch_border_smooth(const float* d_inner, const float* d_outerOnInner, float* d_out, size_t nx, size_t ny, size_t nz, size_t transitionWidth,
                          size_t borderWidth, bool useOuter, hipStream_t stream)
{
    if (nz == 0) return;
    SmoothArgs a{};
    const dim3 grid = tile_grid(nx, ny, nz, a.zPerBlock);
    a.inner = d_inner;
    a.outer = d_outerOnInner;
    a.out = d_out;
    a.nx = (uint32_t)nx;
    a.ny = (uint32_t)ny;
    a.nz = (uint32_t)nz;
    a.tw = transitionWidth;
    a.bw = borderWidth;
    a.useOuter = useOuter ? 1 : 0;
    border_smooth_kernel<<<grid, dim3(kTileX, kTileY, 1), 0, stream>>>(a);
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
    const size_t innerCells = oi.outX * oi.outY;
    FloatScratch s(nz * innerCells, stream);
    const dim3 block(kTileX, kTileY, 1);
    {
        MergeSmoothArgs a{};
        const dim3 grid = tile_grid(oi.outX, oi.outY, nz, a.zPerBlock);
        a.oi = plan_ref(oi);
        a.inner = d_inner;
        a.outer = d_outer;
        a.s = s.get();
        a.nx = (uint32_t)oi.outX;
        a.ny = (uint32_t)oi.outY;
        a.nz = (uint32_t)nz;
        a.tw = m.transitionWidth;
        a.bw = m.borderWidth;
        a.useOuter = m.useOuter ? 1 : 0;
        switch (stencil_of(oi)) {
        case 1: merge_smooth_kernel<1><<<grid, block, 0, stream>>>(a); break;
        case 2: merge_smooth_kernel<2><<<grid, block, 0, stream>>>(a); break;
        default: merge_smooth_kernel<4><<<grid, block, 0, stream>>>(a); break;
        }
        FA_HIP(hipGetLastError());
    }
    MergeOverlayArgs a{};
    const dim3 grid = tile_grid(st.outX, st.outY, nz, a.zPerBlock);
    a.st = plan_ref(st);
    a.ot = plan_ref(ot);
    a.s = s.get();
    a.outer = d_outer;
    a.out = d_out;
    a.nx = (uint32_t)st.outX;
    a.ny = (uint32_t)st.outY;
    a.nz = (uint32_t)nz;
    const int otStencil = stencil_of(ot);
    switch (stencil_of(st)) {
    case 1: launch_overlay_st<1>(otStencil, grid, a, stream); break;
    case 2: launch_overlay_st<2>(otStencil, grid, a, stream); break;
    default: launch_overlay_st<4>(otStencil, grid, a, stream); break;
    }
    FA_HIP(hipGetLastError());
}

// The same four steps as the reference runs them: three full applies and the two elementwise kernels on temporaries
void launch_merge_chain(const fimex_amd_merge_plan& m, const float* d_inner, const float* d_outer, size_t nz, float* d_out, hipStream_t stream)
{
    if (nz == 0) return;
    const fimex_amd_regrid_plan &oi = *m.outerToInner, &st = *m.innerToTarget, &ot = *m.outerToTarget;
    const size_t innerCells = oi.outX * oi.outY, targetCells = st.outX * st.outY;
    FloatScratch s(nz * innerCells, stream), top(nz * targetCells, stream);
    apply_plan_device(oi, d_outer, nz, s.get(), stream);                                                               // step 1
    launch_border_smooth(d_inner, s.get(), s.get(), oi.outX, oi.outY, nz, m.transitionWidth, m.borderWidth, m.useOuter, stream);  // step 2
    apply_plan_device(st, s.get(), nz, top.get(), stream);                                                             // step 3
    apply_plan_device(ot, d_outer, nz, d_out, stream);
    launch_overlay(top.get(), d_out, d_out, nz * targetCells, stream);                                                 // step 4
}

}  // namespace fimex_amd
