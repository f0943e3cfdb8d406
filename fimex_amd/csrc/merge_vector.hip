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

using namespace merge_launch;
using FloatPlan = PlanRef<float, 0>;
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
    FloatPlan oi;                  // outer -> inner grid
    const double2* rotOI;          // [ny][nx] (m0, m1) of R_oi
    const float *innerU, *innerV;  // [nz][ny][nx]
    const float *outerU, *outerV;  // [nz] source slices of oi
    float *su, *sv;                // [nz][ny][nx]
    Tile tile;
    Smoothing sm;
};

// steps 1 and 2: (Su, Sv) = smooth((Iu, Iv), rot(R_oi; regrid(Ou), regrid(Ov))), the regrid and the rotation evaluated only
// where the smoothing of either component reads them
template <int STENCIL>
__global__ void __launch_bounds__(kBlock) merge_smooth_vector_kernel(const MergeSmoothVectorArgs a)
{
    const Cell c(a.tile);
    if (!c.inside) return;
    const SmoothClass cls = merge_math::smooth_class(c.x, c.y, a.tile.nx, a.tile.ny, a.sm.tw, a.sm.bw);
    const GatherEntry<STENCIL, float> e = a.oi.entry<STENCIL>(c.cell);
    LazyMatrix rot{a.rotOI, c.cell};
    const bool useOuter = a.sm.useOuter != 0;
    const uint32_t cb = c.offset<float>();
    for_z_groups<ahead_of<STENCIL>()>(c.z0, c.z1, [&](uint32_t z, auto n) {
        constexpr int N = decltype(n)::value;
        float iu[N], iv[N];
        Pair s[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            iu[k] = ld(c.slice(a.innerU, z + k), cb);
            iv[k] = ld(c.slice(a.innerV, z + k), cb);
        }
#pragma unroll
        for (int k = 0; k < N; ++k)
            s[k] = merge_math::smooth_pair(cls, iu[k], iv[k], [&] {
                return regrid_rotate<STENCIL>(e, a.oi.slice(a.outerU, z + k), a.oi.slice(a.outerV, z + k), rot.get());
            }, useOuter);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            st_plain(c.slice(a.su, z + k), cb, 0, s[k].u);
            st_plain(c.slice(a.sv, z + k), cb, 0, s[k].v);
        }
    });
}

struct MergeOverlayVectorArgs {
    FloatPlan st;                  // smoothed inner -> target
    FloatPlan ot;                  // outer -> target
    const double2 *rotST, *rotOT;  // [ny][nx] (m0, m1) of R_st and R_ot
    const float *su, *sv;          // [nz] source slices of st
    const float *outerU, *outerV;  // [nz] source slices of ot
    float *outU, *outV;            // [nz][ny][nx]
    Tile tile;
};

// steps 3 and 4: out = rot(R_st; regrid(Su), regrid(Sv)) where that is defined, component by component, else
// rot(R_ot; regrid(Ou), regrid(Ov)); the outer -> target entry and R_ot are touched only where a component of the first pair is NaN
template <int ST, int OT>
__global__ void __launch_bounds__(kBlock) merge_overlay_vector_kernel(const MergeOverlayVectorArgs a)
{
    const Cell c(a.tile);
    if (!c.inside) return;
    const GatherEntry<ST, float> es = a.st.entry<ST>(c.cell);
    const GatherEntry<OT, float> eo = a.ot.entry<OT>(c.cell);
    const double2 mS = a.rotST[c.cell];
    LazyMatrix rotO{a.rotOT, c.cell};
    const uint32_t cb = c.offset<float>();
    for_z_groups<ahead_of<(ST > OT ? ST : OT)>()>(c.z0, c.z1, [&](uint32_t z, auto n) {
        constexpr int N = decltype(n)::value;
        Pair p[N];
#pragma unroll
        for (int k = 0; k < N; ++k) p[k] = regrid_rotate<ST>(es, a.st.slice(a.su, z + k), a.st.slice(a.sv, z + k), mS);
#pragma unroll
        for (int k = 0; k < N; ++k)
            p[k] = merge_math::overlay_pair(p[k], [&] {
                return regrid_rotate<OT>(eo, a.ot.slice(a.outerU, z + k), a.ot.slice(a.outerV, z + k), rotO.get());
            });
#pragma unroll
        for (int k = 0; k < N; ++k) {
            st_stream(c.slice(a.outU, z + k), cb, 0, p[k].u);
            st_stream(c.slice(a.outV, z + k), cb, 0, p[k].v);
        }
    });
}

}  // namespace

// every argument has been checked (capi_merge_vector.hip)
void launch_merge_vector_fused(const fimex_amd_merge_plan& m, const fimex_amd_vector_plan& rotOI, const fimex_amd_vector_plan& rotST,
                               const fimex_amd_vector_plan& rotOT, const float* d_innerU, const float* d_innerV, const float* d_outerU,
                               const float* d_outerV, size_t nz, float* d_outU, float* d_outV, hipStream_t stream)
{
    if (nz == 0) return;
    const fimex_amd_regrid_plan &oi = *m.outerToInner, &st = *m.innerToTarget, &ot = *m.outerToTarget;
    const size_t innerN = nz * oi.outX * oi.outY;
    Scratch s(2 * innerN * sizeof(float), stream);  // Su, then Sv
    float *su = s.get<float>(), *sv = su + innerN;
    {
        MergeSmoothVectorArgs a{plan_ref<float>(oi), rotOI.cossin.get(), d_innerU, d_innerV, d_outerU, d_outerV, su, sv, {},
                                smoothing(m.transitionWidth, m.borderWidth, m.useOuter)};
        const dim3 grid = tile_grid(oi.outX, oi.outY, nz, a.tile);
        with_stencil(oi, [&](auto stencil) { merge_smooth_vector_kernel<decltype(stencil)::value><<<grid, tile_block(), 0, stream>>>(a); });
        FA_HIP(hipGetLastError());
    }
    MergeOverlayVectorArgs a{plan_ref<float>(st), plan_ref<float>(ot), rotST.cossin.get(), rotOT.cossin.get(), su, sv, d_outerU, d_outerV, d_outU, d_outV, {}};
    const dim3 grid = tile_grid(st.outX, st.outY, nz, a.tile);
    with_stencil(st, [&](auto sts) {
        with_stencil(ot, [&](auto ots) { merge_overlay_vector_kernel<decltype(sts)::value, decltype(ots)::value><<<grid, tile_block(), 0, stream>>>(a); });
    });
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
    Scratch s(2 * innerN * sizeof(float), stream), top(2 * targetN * sizeof(float), stream);
    float *su = s.get<float>(), *sv = su + innerN, *topU = top.get<float>(), *topV = topU + targetN;
    apply_vector_pair(oi, rotOI, d_outerU, d_outerV, nz, su, sv, stream);                                                    // step 1
    launch_border_smooth(d_innerU, su, su, oi.outX, oi.outY, nz, m.transitionWidth, m.borderWidth, m.useOuter, stream);       // step 2
    launch_border_smooth(d_innerV, sv, sv, oi.outX, oi.outY, nz, m.transitionWidth, m.borderWidth, m.useOuter, stream);
    apply_vector_pair(st, rotST, su, sv, nz, topU, topV, stream);                                                            // step 3
    apply_vector_pair(ot, rotOT, d_outerU, d_outerV, nz, d_outU, d_outV, stream);
    launch_overlay(topU, d_outU, d_outU, targetN, stream);                                                                     // step 4
    launch_overlay(topV, d_outV, d_outV, targetN, stream);
}

}  // namespace fimex_amd
