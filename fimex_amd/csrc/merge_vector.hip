// Grid merging of an x/y vector pair: CDMMerger's four steps (src/CDMMerger.cc:212-227) on a pair
// such as x_wind / y_wind, where each of the merger's three interpolators rotates the pair behind its regrid
// (src/CDMInterpolator.cc:259-283, mifi_vector_reproject_values_by_matrix_f):
//   merge_smooth_vector_kernel   steps 1 and 2: a lane per inner cell evaluates the one outer->inner entry on Ou and Ov and rotates
//                                the pair by R_oi only where the smoothing of either component reads the outer, and writes Su, Sv
//   merge_overlay_vector_kernel  steps 3 and 4: a lane per target cell evaluates the inner->target entry on Su and Sv and rotates by
//                                R_st; where either rotated component is NaN it evaluates the outer->target entry on Ou and Ov,
//                                rotates by R_ot, and chooses component by component
// The shape is merge.hip's: a lane owns one cell of a kTileX x kTileY tile and keeps its class and its plan entries, decoded once
// for both components, in registers over the z loop; every slice has its own buffer descriptor.  (m0, m1) of a rotation is read
// once per cell and z chunk, at the first slice that needs it.  The per-cell arithmetic is merge_vector_math.hpp's and nothing
// else.  Built with -ffp-contract=off.
#include "gather_entry.hpp"
#include "merge_launch.hpp"
#include "merge_vector_math.hpp"
#include "plan.hpp"

namespace fimex_amd {

namespace {

using merge_launch::ahead_of;
using merge_launch::FloatScratch;
using merge_launch::kTileX;
using merge_launch::kTileY;
using merge_launch::LazyMatrix;
using merge_launch::plan_ref;
using merge_launch::PlanRef;
using merge_launch::stencil_of;
using merge_launch::tile_grid;
using merge_math::Pair;
using merge_math::SmoothClass;

// both components of one slice through one decoded entry, rotated
template <int STENCIL>
__device__ __forceinline__ Pair regrid_rotate(const GatherEntry<STENCIL, float>& e, rsrc_t u, rsrc_t v, const double2& m)
{
    const float ru = e.value(u), rv = e.value(v);
    return merge_math::rotate_pair_values(ru, rv, m.x, m.y);
}

struct MergeSmoothVectorArgs {
    PlanRef oi;                    // outer -> inner grid
    const double2* rotOI;          // [ny][nx] (m0, m1) of R_oi
    const float *innerU, *innerV;  // [nz][ny][nx]
    const float *outerU, *outerV;  // [nz] source slices of oi
    float *su, *sv;                // [nz][ny][nx]
    uint32_t nx, ny, nz, zPerBlock;
    uint64_t tw, bw;
    int useOuter;
};

// steps 1 and 2: (Su, Sv) = smooth((Iu, Iv), rot(R_oi; regrid(Ou), regrid(Ov))), the regrid and the rotation evaluated only
// where the smoothing of either component reads them
template <int STENCIL>
__global__ void __launch_bounds__(kBlock) merge_smooth_vector_kernel(const MergeSmoothVectorArgs a)
{
    constexpr int AHEAD = ahead_of<STENCIL>();
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= a.nx || y >= a.ny) return;
    const uint32_t cell = y * a.nx + x, cb = cell * 4u;
    const SmoothClass c = merge_math::smooth_class(x, y, a.nx, a.ny, a.tw, a.bw);
    const GatherEntry<STENCIL, float> e = a.oi.entry<STENCIL>(cell);
    LazyMatrix rot{a.rotOI, cell};
    const bool useOuter = a.useOuter != 0;
    const size_t plane = (size_t)a.nx * a.ny;
    const uint32_t planeBytes = (uint32_t)plane * 4u;
    auto smooth = [&](uint32_t zz, float iu, float iv) {
        return merge_math::smooth_pair(c, iu, iv, [&] {
            return regrid_rotate<STENCIL>(e, make_rsrc(a.outerU + (size_t)zz * a.oi.inLayer, a.oi.inBytes),
                                          make_rsrc(a.outerV + (size_t)zz * a.oi.inLayer, a.oi.inBytes), rot.get());
        }, useOuter);
    };
    uint32_t z = blockIdx.z * a.zPerBlock;
    const uint32_t z1 = min(a.nz, z + a.zPerBlock);
    for (; z + AHEAD <= z1; z += AHEAD) {
        float iu[AHEAD], iv[AHEAD];
        Pair s[AHEAD];
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) {
            iu[k] = ld(make_rsrc(a.innerU + (size_t)(z + k) * plane, planeBytes), cb);
            iv[k] = ld(make_rsrc(a.innerV + (size_t)(z + k) * plane, planeBytes), cb);
        }
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) s[k] = smooth(z + k, iu[k], iv[k]);
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) {
            st_plain(make_rsrc(a.su + (size_t)(z + k) * plane, planeBytes), cb, 0, s[k].u);
            st_plain(make_rsrc(a.sv + (size_t)(z + k) * plane, planeBytes), cb, 0, s[k].v);
        }
    }
    for (; z < z1; ++z) {
        const float iu = ld(make_rsrc(a.innerU + (size_t)z * plane, planeBytes), cb), iv = ld(make_rsrc(a.innerV + (size_t)z * plane, planeBytes), cb);
        const Pair s = smooth(z, iu, iv);
        st_plain(make_rsrc(a.su + (size_t)z * plane, planeBytes), cb, 0, s.u);
        st_plain(make_rsrc(a.sv + (size_t)z * plane, planeBytes), cb, 0, s.v);
    }
}

struct MergeOverlayVectorArgs {
    PlanRef st;                    // smoothed inner -> target
    PlanRef ot;                    // outer -> target
    const double2 *rotST, *rotOT;  // [ny][nx] (m0, m1) of R_st and R_ot
    const float *su, *sv;          // [nz] source slices of st
    const float *outerU, *outerV;  // [nz] source slices of ot
    float *outU, *outV;            // [nz][ny][nx]
    uint32_t nx, ny, nz, zPerBlock;
};

// steps 3 and 4: out = rot(R_st; regrid(Su), regrid(Sv)) where that is defined, component by component, else
// rot(R_ot; regrid(Ou), regrid(Ov)); the outer -> target entry and R_ot are touched only where a component of the first pair is NaN
template <int ST, int OT>
__global__ void __launch_bounds__(kBlock) merge_overlay_vector_kernel(const MergeOverlayVectorArgs a)
{
    constexpr int AHEAD = ahead_of<(ST > OT ? ST : OT)>();
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= a.nx || y >= a.ny) return;
    const uint32_t cell = y * a.nx + x, cb = cell * 4u;
    const GatherEntry<ST, float> es = a.st.entry<ST>(cell);
    const GatherEntry<OT, float> eo = a.ot.entry<OT>(cell);
    const double2 mS = a.rotST[cell];
    LazyMatrix rotO{a.rotOT, cell};
    const size_t plane = (size_t)a.nx * a.ny;
    const uint32_t planeBytes = (uint32_t)plane * 4u;
    auto top = [&](uint32_t zz) {
        return regrid_rotate<ST>(es, make_rsrc(a.su + (size_t)zz * a.st.inLayer, a.st.inBytes), make_rsrc(a.sv + (size_t)zz * a.st.inLayer, a.st.inBytes),
                                 mS);
    };
    auto overlay = [&](uint32_t zz, const Pair& t) {
        return merge_math::overlay_pair(t, [&] {
            return regrid_rotate<OT>(eo, make_rsrc(a.outerU + (size_t)zz * a.ot.inLayer, a.ot.inBytes),
                                     make_rsrc(a.outerV + (size_t)zz * a.ot.inLayer, a.ot.inBytes), rotO.get());
        });
    };
    uint32_t z = blockIdx.z * a.zPerBlock;
    const uint32_t z1 = min(a.nz, z + a.zPerBlock);
    for (; z + AHEAD <= z1; z += AHEAD) {
        Pair p[AHEAD];
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) p[k] = top(z + k);
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) p[k] = overlay(z + k, p[k]);
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) {
            st_stream(make_rsrc(a.outU + (size_t)(z + k) * plane, planeBytes), cb, 0, p[k].u);
            st_stream(make_rsrc(a.outV + (size_t)(z + k) * plane, planeBytes), cb, 0, p[k].v);
        }
    }
    for (; z < z1; ++z) {
        const Pair p = overlay(z, top(z));
        st_stream(make_rsrc(a.outU + (size_t)z * plane, planeBytes), cb, 0, p.u);
        st_stream(make_rsrc(a.outV + (size_t)z * plane, planeBytes), cb, 0, p.v);
    }
}

template <int ST>
void launch_overlay_st(int ot, dim3 grid, const MergeOverlayVectorArgs& a, hipStream_t stream)
{
    const dim3 block(kTileX, kTileY, 1);
    if (ot == 1) merge_overlay_vector_kernel<ST, 1><<<grid, block, 0, stream>>>(a);
    else if (ot == 2) merge_overlay_vector_kernel<ST, 2><<<grid, block, 0, stream>>>(a);
    else merge_overlay_vector_kernel<ST, 4><<<grid, block, 0, stream>>>(a);
}

}  // namespace

// every argument has been checked (capi_merge_vector.hip)
void launch_merge_vector_fused(const fimex_amd_merge_plan& m, const fimex_amd_vector_plan& rotOI, const fimex_amd_vector_plan& rotST,
                               const fimex_amd_vector_plan& rotOT, const float* d_innerU, const float* d_innerV, const float* d_outerU,
                               const float* d_outerV, size_t nz, float* d_outU, float* d_outV, hipStream_t stream)
{
    if (nz == 0) return;
    const fimex_amd_regrid_plan &oi = *m.outerToInner, &st = *m.innerToTarget, &ot = *m.outerToTarget;
    const size_t innerCells = oi.outX * oi.outY;
    FloatScratch s(2 * nz * innerCells, stream);  // Su, then Sv
    float *su = s.get(), *sv = s.get() + nz * innerCells;
    const dim3 block(kTileX, kTileY, 1);
    {
        MergeSmoothVectorArgs a{};
        const dim3 grid = tile_grid(oi.outX, oi.outY, nz, a.zPerBlock);
        a.oi = plan_ref(oi);
        a.rotOI = rotOI.cossin.get();
        a.innerU = d_innerU;
        a.innerV = d_innerV;
        a.outerU = d_outerU;
        a.outerV = d_outerV;
        a.su = su;
        a.sv = sv;
        a.nx = (uint32_t)oi.outX;
        a.ny = (uint32_t)oi.outY;
        a.nz = (uint32_t)nz;
        a.tw = m.transitionWidth;
        a.bw = m.borderWidth;
        a.useOuter = m.useOuter ? 1 : 0;
        switch (stencil_of(oi)) {
        case 1: merge_smooth_vector_kernel<1><<<grid, block, 0, stream>>>(a); break;
        case 2: merge_smooth_vector_kernel<2><<<grid, block, 0, stream>>>(a); break;
        default: merge_smooth_vector_kernel<4><<<grid, block, 0, stream>>>(a); break;
        }
        FA_HIP(hipGetLastError());
    }
    MergeOverlayVectorArgs a{};
    const dim3 grid = tile_grid(st.outX, st.outY, nz, a.zPerBlock);
    a.st = plan_ref(st);
    a.ot = plan_ref(ot);
    a.rotST = rotST.cossin.get();
    a.rotOT = rotOT.cossin.get();
    a.su = su;
    a.sv = sv;
    a.outerU = d_outerU;
    a.outerV = d_outerV;
    a.outU = d_outU;
    a.outV = d_outV;
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

// The same four steps as the reference runs them, on temporaries: three regrids of the pair, each with its rotation (one launch
// each where the pair kernel serves, else three: apply_vector_pair), the smoothing and the overlay once per component
void launch_merge_vector_chain(const fimex_amd_merge_plan& m, const fimex_amd_vector_plan& rotOI, const fimex_amd_vector_plan& rotST,
                               const fimex_amd_vector_plan& rotOT, const float* d_innerU, const float* d_innerV, const float* d_outerU,
                               const float* d_outerV, size_t nz, float* d_outU, float* d_outV, hipStream_t stream)
{
    if (nz == 0) return;
    const fimex_amd_regrid_plan &oi = *m.outerToInner, &st = *m.innerToTarget, &ot = *m.outerToTarget;
    const size_t innerN = nz * oi.outX * oi.outY, targetN = nz * st.outX * st.outY;
    FloatScratch s(2 * innerN, stream), top(2 * targetN, stream);
    float *su = s.get(), *sv = s.get() + innerN, *topU = top.get(), *topV = top.get() + targetN;
    apply_vector_pair(oi, rotOI, d_outerU, d_outerV, nz, su, sv, stream);                                                    // step 1
    launch_border_smooth(d_innerU, su, su, oi.outX, oi.outY, nz, m.transitionWidth, m.borderWidth, m.useOuter, stream);       // step 2
    launch_border_smooth(d_innerV, sv, sv, oi.outX, oi.outY, nz, m.transitionWidth, m.borderWidth, m.useOuter, stream);
    apply_vector_pair(st, rotST, su, sv, nz, topU, topV, stream);                                                            // step 3
    apply_vector_pair(ot, rotOT, d_outerU, d_outerV, nz, d_outU, d_outV, stream);
    launch_overlay(topU, d_outU, d_outU, targetN, stream);                                                                     // step 4
    launch_overlay(topV, d_outV, d_outV, targetN, stream);
}

}  // namespace fimex_amd
