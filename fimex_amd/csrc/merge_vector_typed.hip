// Grid merging of an x/y vector pair in its stored types: CDMMerger's four steps
// (src/CDMMerger.cc:212-227) on a pair such as x_wind / y_wind whose four fields -- inner u, inner v, outer u, outer v -- are packed
// integers, each with its own fimex_amd_packing.  Every CDMInterpolator of the merger reads both components as raw counts with the
// own fill value as NaN, regrids them, rotates the counts and writes each back in its own type (src/CDMInterpolator.cc:255-285);
// the smoothing and the overlay unpack, work in double and pack with the inner component's packing (6.15).
//   merge_smooth_vector_typed_kernel<STENCIL, T>    steps 1 and 2: a lane per inner cell evaluates the one outer -> inner entry on
//                                                   Ou and Ov, each with its own fill value, and rotates by R_oi only where the
//                                                   smoothing of either component reads the outer; writes Su and Sv in T
//   merge_overlay_vector_typed_kernel<ST, OT, T>    steps 3 and 4: a lane per target cell evaluates the inner -> target entry on Su
//                                                   and Sv and rotates by R_st; where either rounded component is its fill value
//                                                   it evaluates the outer -> target entry on Ou and Ov and rotates by R_ot
// The shape is merge_typed.hip's crossed with merge_vector.hip's: a lane owns one cell of a kTileX x kTileY tile, keeps its class
// and its plan entries -- decoded once for both components, which differ in their Element<T> only -- in registers over the z loop;
// every slice has its own buffer descriptor; (m0, m1) of a rotation is read at the first slice that needs it.  The fused pair serves
// T = short and unsigned short with all four fields of one type; everything else takes the chain of seven steps below.  The
// per-cell arithmetic is merge_vector_typed_math.hpp's and nothing else.  Built with -ffp-contract=off.
#include "gather_entry.hpp"
#include "merge_launch.hpp"
#include "merge_vector_typed_math.hpp"
#include "plan.hpp"

namespace fimex_amd {

namespace {

namespace mm = merge_math;

using namespace merge_launch;
// the entry is decoded once per cell; the second component's entry is the first with the other element, that is the other fill value
template <typename T>
using PairPlan = PlanRef<T, 2>;

// both components of one slice through the one decoded entry, as counts with the own fill value as NaN, rotated
template <int STENCIL, typename T>
__device__ __forceinline__ mm::Pair regrid_rotate(const GatherEntry<STENCIL, T>& eu, const GatherEntry<STENCIL, T>& ev, rsrc_t u, rsrc_t v,
                                                  const double2& m)
{
    const float ru = eu.value(u), rv = ev.value(v);
    return mm::rotate_pair_values(ru, rv, m.x, m.y);
}

template <typename T>
struct MergeSmoothVectorTypedArgs {
    PairPlan<T> oi;            // outer -> inner grid
    const double2* rotOI;      // [ny][nx] (m0, m1) of R_oi
    const T *innerU, *innerV;  // [nz][ny][nx]
    const T *outerU, *outerV;  // [nz] source slices of oi
    T *su, *sv;                // [nz][ny][nx]
    Tile tile;
    Smoothing sm;
    T fillOu, fillOv;          // what interpolationArray2Data writes for an undefined outer component
    mm::ComponentOps<T> opsU, opsV;
};

// steps 1 and 2: (Su, Sv) = smooth((Iu, Iv), round(rot(R_oi; regrid(Ou), regrid(Ov)))), the regrid and the rotation evaluated only
// where the smoothing of either component reads them
template <int STENCIL, typename T>
__global__ void __launch_bounds__(kBlock) merge_smooth_vector_typed_kernel(const MergeSmoothVectorTypedArgs<T> a)
{
    const Cell c(a.tile);
    if (!c.inside) return;
    const mm::SmoothClass cls = mm::smooth_class(c.x, c.y, a.tile.nx, a.tile.ny, a.sm.tw, a.sm.bw);
    const GatherEntry<STENCIL, T> eu = a.oi.template entry<STENCIL>(c.cell);
    const GatherEntry<STENCIL, T> ev = a.oi.template second<STENCIL>(eu);
    LazyMatrix rot{a.rotOI, c.cell};
    const bool useOuter = a.sm.useOuter != 0;
    const uint32_t cb = c.offset<T>();
    for_z_groups<ahead_of<STENCIL>()>(c.z0, c.z1, [&](uint32_t z, auto n) {
        constexpr int N = decltype(n)::value;
        T iu[N], iv[N];
        mm::StoredPair<T> s[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            iu[k] = ld_raw<T>(c.slice(a.innerU, z + k), cb);
            iv[k] = ld_raw<T>(c.slice(a.innerV, z + k), cb);
        }
#pragma unroll
        for (int k = 0; k < N; ++k)
            s[k] = mm::smooth_pair_typed<T>(cls, iu[k], iv[k], [&] {
                return regrid_rotate<STENCIL, T>(eu, ev, a.oi.slice(a.outerU, z + k), a.oi.slice(a.outerV, z + k), rot.get());
            }, a.fillOu, a.fillOv, a.opsU, a.opsV, useOuter);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            st_raw<T, false>(c.slice(a.su, z + k), cb, 0, s[k].u);
            st_raw<T, false>(c.slice(a.sv, z + k), cb, 0, s[k].v);
        }
    });
}

template <typename T>
struct MergeOverlayVectorTypedArgs {
    PairPlan<T> st;                // smoothed inner -> target
    PairPlan<T> ot;                // outer -> target
    const double2 *rotST, *rotOT;  // [ny][nx] (m0, m1) of R_st and R_ot
    const T *su, *sv;              // [nz] source slices of st
    const T *outerU, *outerV;      // [nz] source slices of ot
    T *outU, *outV;                // [nz][ny][nx]
    Tile tile;
    T fillIu, fillIv, fillOu, fillOv;
    mm::ComponentOps<T> opsU, opsV;
};

// steps 3 and 4: the outer -> target entry and R_ot are touched only where a rounded component of the first pair is its fill value
template <int ST, int OT, typename T>
__global__ void __launch_bounds__(kBlock) merge_overlay_vector_typed_kernel(const MergeOverlayVectorTypedArgs<T> a)
{
    const Cell c(a.tile);
    if (!c.inside) return;
    const GatherEntry<ST, T> esu = a.st.template entry<ST>(c.cell);
    const GatherEntry<ST, T> esv = a.st.template second<ST>(esu);
    const GatherEntry<OT, T> eou = a.ot.template entry<OT>(c.cell);
    const GatherEntry<OT, T> eov = a.ot.template second<OT>(eou);
    const double2 mS = a.rotST[c.cell];
    LazyMatrix rotO{a.rotOT, c.cell};
    const uint32_t cb = c.offset<T>();
    for_z_groups<ahead_of<(ST > OT ? ST : OT)>()>(c.z0, c.z1, [&](uint32_t z, auto n) {
        constexpr int N = decltype(n)::value;
        mm::Pair t[N];
        mm::StoredPair<T> p[N];
#pragma unroll
        for (int k = 0; k < N; ++k) t[k] = regrid_rotate<ST, T>(esu, esv, a.st.slice(a.su, z + k), a.st.slice(a.sv, z + k), mS);
#pragma unroll
        for (int k = 0; k < N; ++k)
            p[k] = mm::regrid_overlay_pair_typed<T>(t[k], a.fillIu, a.fillIv, [&] {
                return regrid_rotate<OT, T>(eou, eov, a.ot.slice(a.outerU, z + k), a.ot.slice(a.outerV, z + k), rotO.get());
            }, a.fillOu, a.fillOv, a.opsU, a.opsV);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            st_raw<T, true>(c.slice(a.outU, z + k), cb, 0, p[k].u);
            st_raw<T, true>(c.slice(a.outV, z + k), cb, 0, p[k].v);
        }
    });
}

template <typename T>
mm::ComponentOps<T> component_ops(const fimex_amd_packing& pi, const fimex_amd_packing& po)
{
    return mm::make_component_ops<T>(pi.fill, pi.scale, pi.offset, po.fill, po.scale, po.offset);
}

template <typename T>
void merge_fused_t(const fimex_amd_merge_plan& m, const fimex_amd_vector_plan& rotOI, const fimex_amd_vector_plan& rotST,
                   const fimex_amd_vector_plan& rotOT, const PackedVectorFields& in, size_t nz, void* d_outU, void* d_outV, hipStream_t stream)
{
    const fimex_amd_regrid_plan &oi = *m.outerToInner, &st = *m.innerToTarget, &ot = *m.outerToTarget;
    const fimex_amd_packing &pIu = in.innerUPacking, &pIv = in.innerVPacking, &pOu = in.outerUPacking, &pOv = in.outerVPacking;
    const size_t innerN = nz * oi.outX * oi.outY;
    Scratch s(2 * innerN * sizeof(T), stream);  // Su, then Sv
    T *su = s.get<T>(), *sv = su + innerN;
    const T *innerU = static_cast<const T*>(in.d_innerU), *innerV = static_cast<const T*>(in.d_innerV);
    const T *outerU = static_cast<const T*>(in.d_outerU), *outerV = static_cast<const T*>(in.d_outerV);
    const mm::ComponentOps<T> opsU = component_ops<T>(pIu, pOu), opsV = component_ops<T>(pIv, pOv);
    const T fillIu = static_cast<T>(pIu.fill), fillIv = static_cast<T>(pIv.fill), fillOu = static_cast<T>(pOu.fill), fillOv = static_cast<T>(pOv.fill);
    {
        MergeSmoothVectorTypedArgs<T> a{plan_ref<T>(oi, pOu.fill, pOv.fill), rotOI.cossin.get(), innerU, innerV, outerU, outerV, su, sv, {},
                                        smoothing(m.transitionWidth, m.borderWidth, m.useOuter), fillOu, fillOv, opsU, opsV};
        const dim3 grid = tile_grid(oi.outX, oi.outY, nz, a.tile);
        with_stencil(oi, [&](auto stencil) { merge_smooth_vector_typed_kernel<decltype(stencil)::value, T><<<grid, tile_block(), 0, stream>>>(a); });
        FA_HIP(hipGetLastError());
    }
    MergeOverlayVectorTypedArgs<T> a{plan_ref<T>(st, pIu.fill, pIv.fill), plan_ref<T>(ot, pOu.fill, pOv.fill), rotST.cossin.get(), rotOT.cossin.get(), su, sv,
                                     outerU, outerV, static_cast<T*>(d_outU), static_cast<T*>(d_outV), {}, fillIu, fillIv, fillOu, fillOv, opsU, opsV};
    const dim3 grid = tile_grid(st.outX, st.outY, nz, a.tile);
    with_stencil(st, [&](auto sts) {
        with_stencil(ot, [&](auto ots) {
            merge_overlay_vector_typed_kernel<decltype(sts)::value, decltype(ots)::value, T><<<grid, tile_block(), 0, stream>>>(a);
        });
    });
    FA_HIP(hipGetLastError());
}

}  // namespace

// The dispatch rule of the fused pair: all four fields short, or all unsigned short; the six buffers aligned to
// their element; all four fill values representable in the type, so that the kernels' casts of them are those of the chain; not
// switched off in the tuning build.  false: not served, nothing launched.  Every argument has been checked
// (capi_merge_vector_typed.hip).
bool launch_merge_vector_typed_fused(const fimex_amd_merge_plan& m, const fimex_amd_vector_plan& rotOI, const fimex_amd_vector_plan& rotST,
                                     const fimex_amd_vector_plan& rotOT, const PackedVectorFields& in, size_t nz, void* d_outU, void* d_outV,
                                     hipStream_t stream)
{
    const fimex_amd_packing* packings[4] = {&in.innerUPacking, &in.innerVPacking, &in.outerUPacking, &in.outerVPacking};
    const int type = packings[0]->type;
    if (type != FIMEX_AMD_CDM_SHORT && type != FIMEX_AMD_CDM_USHORT) return false;
    for (const fimex_amd_packing* p : packings)
        if (p->type != type || !scaled_fill_representable(p->type, p->fill)) return false;
    for (const void* p : {in.d_innerU, in.d_innerV, in.d_outerU, in.d_outerV, (const void*)d_outU, (const void*)d_outV})
        if (!aligned_to(p, 2)) return false;
    if (tuning("MERGE_VECTOR_TYPED_FUSED", 1) == 0) return false;
    if (nz == 0) return true;
    if (type == FIMEX_AMD_CDM_SHORT) merge_fused_t<short>(m, rotOI, rotST, rotOT, in, nz, d_outU, d_outV, stream);
    else merge_fused_t<unsigned short>(m, rotOI, rotST, rotOT, in, nz, d_outU, d_outV, stream);
    return true;
}

// The same four steps as the reference runs them, on stream-ordered temporaries of the stored types: three regrids of the pair,
// each with its rotation on the counts (apply_vector_pair_typed), the typed smoothing and the typed overlay once per component.
// Serves all ten numeric types and components of different types.
void launch_merge_vector_typed_chain(const fimex_amd_merge_plan& m, const fimex_amd_vector_plan& rotOI, const fimex_amd_vector_plan& rotST,
                                     const fimex_amd_vector_plan& rotOT, const PackedVectorFields& in, size_t nz, void* d_outU, void* d_outV,
                                     hipStream_t stream)
{
    if (nz == 0) return;
    const fimex_amd_regrid_plan &oi = *m.outerToInner, &st = *m.innerToTarget, &ot = *m.outerToTarget;
    const fimex_amd_packing &pIu = in.innerUPacking, &pIv = in.innerVPacking, &pOu = in.outerUPacking, &pOv = in.outerVPacking;
    const size_t innerN = nz * oi.outX * oi.outY, targetN = nz * st.outX * st.outY;
    const size_t sizeIu = cdm_type_size(pIu.type), sizeIv = cdm_type_size(pIv.type), sizeOu = cdm_type_size(pOu.type), sizeOv = cdm_type_size(pOv.type);
    Scratch oiU(innerN * sizeOu, stream), oiV(innerN * sizeOv, stream), su(innerN * sizeIu, stream), sv(innerN * sizeIv, stream);
    Scratch topU(targetN * sizeIu, stream), topV(targetN * sizeIv, stream), baseU(targetN * sizeOu, stream), baseV(targetN * sizeOv, stream);
    apply_vector_pair_typed(oi, rotOI, in.d_outerU, pOu.type, pOu.fill, in.d_outerV, pOv.type, pOv.fill, nz, oiU.get(), oiV.get(), stream);   // step 1
    launch_border_smooth_typed(in.d_innerU, pIu, oiU.get(), pOu, su.get(), oi.outX, oi.outY, nz, m.transitionWidth, m.borderWidth, m.useOuter,
                               stream);                                                                                                    // step 2
    launch_border_smooth_typed(in.d_innerV, pIv, oiV.get(), pOv, sv.get(), oi.outX, oi.outY, nz, m.transitionWidth, m.borderWidth, m.useOuter,
                               stream);
    apply_vector_pair_typed(st, rotST, su.get(), pIu.type, pIu.fill, sv.get(), pIv.type, pIv.fill, nz, topU.get(), topV.get(), stream);       // step 3
    apply_vector_pair_typed(ot, rotOT, in.d_outerU, pOu.type, pOu.fill, in.d_outerV, pOv.type, pOv.fill, nz, baseU.get(), baseV.get(), stream);
    launch_overlay_typed(topU.get(), pIu, baseU.get(), pOu, d_outU, targetN, stream);                                                       // step 4
    launch_overlay_typed(topV.get(), pIv, baseV.get(), pOv, d_outV, targetN, stream);
}

}  // namespace fimex_amd
