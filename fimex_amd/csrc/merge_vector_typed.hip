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

using merge_launch::ahead_of;
using merge_launch::kTileX;
using merge_launch::kTileY;
using merge_launch::LazyMatrix;
using merge_launch::stencil_of;
using merge_launch::tile_grid;

// ---- a backward plan's arrays on slices of T that hold the two components of a pair: the entry is decoded once per cell; the
// second component's entry is the first with the other element, that is the other fill value
template <typename T>
struct PairPlanRef {
    const uint32_t* pos;
    const float *xf, *yf;
    const double *xfd, *yfd;
    uint32_t ix;       // source row length
    uint32_t inBytes;  // bytes of a source slice
    size_t inLayer;    // cells of a source slice
    typename Element<T>::Params elU, elV;  // each source component's fill value, as data2InterpolationArray takes it

    template <int STENCIL>
    __device__ __forceinline__ GatherEntry<STENCIL, T> entry_u(uint32_t cell) const
    {
        const Element<T> e(elU);
        if constexpr (STENCIL == 4) return {pos[cell], xfd[cell], yfd[cell], ix, e};
        else if constexpr (STENCIL == 2) return {pos[cell], xf[cell], yf[cell], ix, e};
        else return {pos[cell], 0.f, 0.f, ix, e};
    }
    template <int STENCIL>
    __device__ __forceinline__ GatherEntry<STENCIL, T> entry_v(const GatherEntry<STENCIL, T>& u) const
    {
        GatherEntry<STENCIL, T> v = u;
        v.el = Element<T>(elV);
        return v;
    }
};

// the element parameters are those of launch_typed_gather: the fill value narrowed to float, none where that is NaN
template <typename T>
typename Element<T>::Params element_params(double fill)
{
    const float bad = (float)fill;
    return typename Element<T>::Params{bad, !(bad != bad), fill};
}

template <typename T>
PairPlanRef<T> pair_plan_ref(const fimex_amd_regrid_plan& p, double fillU, double fillV)
{
    PairPlanRef<T> r{};
    r.pos = p.pos.get();
    r.xf = p.xf.get();
    r.yf = p.yf.get();
    r.xfd = p.xfd.get();
    r.yfd = p.yfd.get();
    r.ix = (uint32_t)p.inX;
    r.inLayer = p.inX * p.inY;
    r.inBytes = (uint32_t)(r.inLayer * sizeof(T));
    r.elU = element_params<T>(fillU);
    r.elV = element_params<T>(fillV);
    return r;
}

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
    PairPlanRef<T> oi;         // outer -> inner grid
    const double2* rotOI;      // [ny][nx] (m0, m1) of R_oi
    const T *innerU, *innerV;  // [nz][ny][nx]
    const T *outerU, *outerV;  // [nz] source slices of oi
    T *su, *sv;                // [nz][ny][nx]
    uint32_t nx, ny, nz, zPerBlock;
    uint64_t tw, bw;
    int useOuter;
    T fillOu, fillOv;          // what interpolationArray2Data writes for an undefined outer component
    mm::ComponentOps<T> opsU, opsV;
};

// steps 1 and 2: (Su, Sv) = smooth((Iu, Iv), round(rot(R_oi; regrid(Ou), regrid(Ov)))), the regrid and the rotation evaluated only
// where the smoothing of either component reads them
template <int STENCIL, typename T>
__global__ void __launch_bounds__(kBlock) merge_smooth_vector_typed_kernel(const MergeSmoothVectorTypedArgs<T> a)
{
    constexpr int AHEAD = ahead_of<STENCIL>();
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= a.nx || y >= a.ny) return;
    const uint32_t cell = y * a.nx + x, cb = cell * (uint32_t)sizeof(T);
    const mm::SmoothClass c = mm::smooth_class(x, y, a.nx, a.ny, a.tw, a.bw);
    const GatherEntry<STENCIL, T> eu = a.oi.template entry_u<STENCIL>(cell);
    const GatherEntry<STENCIL, T> ev = a.oi.template entry_v<STENCIL>(eu);
    LazyMatrix rot{a.rotOI, cell};
    const bool useOuter = a.useOuter != 0;
    const size_t plane = (size_t)a.nx * a.ny;
    const uint32_t planeBytes = (uint32_t)plane * (uint32_t)sizeof(T);
    auto smooth = [&](uint32_t zz, T iu, T iv) {
        return mm::smooth_pair_typed<T>(c, iu, iv, [&] {
            return regrid_rotate<STENCIL, T>(eu, ev, make_rsrc(a.outerU + (size_t)zz * a.oi.inLayer, a.oi.inBytes),
                                             make_rsrc(a.outerV + (size_t)zz * a.oi.inLayer, a.oi.inBytes), rot.get());
        }, a.fillOu, a.fillOv, a.opsU, a.opsV, useOuter);
    };
    uint32_t z = blockIdx.z * a.zPerBlock;
    const uint32_t z1 = min(a.nz, z + a.zPerBlock);
    for (; z + AHEAD <= z1; z += AHEAD) {
        T iu[AHEAD], iv[AHEAD];
        mm::StoredPair<T> s[AHEAD];
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) {
            iu[k] = ld_raw<T>(make_rsrc(a.innerU + (size_t)(z + k) * plane, planeBytes), cb);
            iv[k] = ld_raw<T>(make_rsrc(a.innerV + (size_t)(z + k) * plane, planeBytes), cb);
        }
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) s[k] = smooth(z + k, iu[k], iv[k]);
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) {
            st_raw<T, false>(make_rsrc(a.su + (size_t)(z + k) * plane, planeBytes), cb, 0, s[k].u);
            st_raw<T, false>(make_rsrc(a.sv + (size_t)(z + k) * plane, planeBytes), cb, 0, s[k].v);
        }
    }
    for (; z < z1; ++z) {
        const T iu = ld_raw<T>(make_rsrc(a.innerU + (size_t)z * plane, planeBytes), cb);
        const T iv = ld_raw<T>(make_rsrc(a.innerV + (size_t)z * plane, planeBytes), cb);
        const mm::StoredPair<T> s = smooth(z, iu, iv);
        st_raw<T, false>(make_rsrc(a.su + (size_t)z * plane, planeBytes), cb, 0, s.u);
        st_raw<T, false>(make_rsrc(a.sv + (size_t)z * plane, planeBytes), cb, 0, s.v);
    }
}

template <typename T>
struct MergeOverlayVectorTypedArgs {
    PairPlanRef<T> st;             // smoothed inner -> target
    PairPlanRef<T> ot;             // outer -> target
    const double2 *rotST, *rotOT;  // [ny][nx] (m0, m1) of R_st and R_ot
    const T *su, *sv;              // [nz] source slices of st
    const T *outerU, *outerV;      // [nz] source slices of ot
    T *outU, *outV;                // [nz][ny][nx]
    uint32_t nx, ny, nz, zPerBlock;
    T fillIu, fillIv, fillOu, fillOv;
    mm::ComponentOps<T> opsU, opsV;
};

// steps 3 and 4: the outer -> target entry and R_ot are touched only where a rounded component of the first pair is its fill value
template <int ST, int OT, typename T>
__global__ void __launch_bounds__(kBlock) merge_overlay_vector_typed_kernel(const MergeOverlayVectorTypedArgs<T> a)
{
    constexpr int AHEAD = ahead_of<(ST > OT ? ST : OT)>();
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= a.nx || y >= a.ny) return;
    const uint32_t cell = y * a.nx + x, cb = cell * (uint32_t)sizeof(T);
    const GatherEntry<ST, T> esu = a.st.template entry_u<ST>(cell);
    const GatherEntry<ST, T> esv = a.st.template entry_v<ST>(esu);
    const GatherEntry<OT, T> eou = a.ot.template entry_u<OT>(cell);
    const GatherEntry<OT, T> eov = a.ot.template entry_v<OT>(eou);
    const double2 mS = a.rotST[cell];
    LazyMatrix rotO{a.rotOT, cell};
    const size_t plane = (size_t)a.nx * a.ny;
    const uint32_t planeBytes = (uint32_t)plane * (uint32_t)sizeof(T);
    auto top = [&](uint32_t zz) {
        return regrid_rotate<ST, T>(esu, esv, make_rsrc(a.su + (size_t)zz * a.st.inLayer, a.st.inBytes),
                                    make_rsrc(a.sv + (size_t)zz * a.st.inLayer, a.st.inBytes), mS);
    };
    auto overlay = [&](uint32_t zz, const mm::Pair& t) {
        return mm::regrid_overlay_pair_typed<T>(t, a.fillIu, a.fillIv, [&] {
            return regrid_rotate<OT, T>(eou, eov, make_rsrc(a.outerU + (size_t)zz * a.ot.inLayer, a.ot.inBytes),
                                        make_rsrc(a.outerV + (size_t)zz * a.ot.inLayer, a.ot.inBytes), rotO.get());
        }, a.fillOu, a.fillOv, a.opsU, a.opsV);
    };
    uint32_t z = blockIdx.z * a.zPerBlock;
    const uint32_t z1 = min(a.nz, z + a.zPerBlock);
    for (; z + AHEAD <= z1; z += AHEAD) {
        mm::Pair t[AHEAD];
        mm::StoredPair<T> p[AHEAD];
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) t[k] = top(z + k);
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) p[k] = overlay(z + k, t[k]);
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) {
            st_raw<T, true>(make_rsrc(a.outU + (size_t)(z + k) * plane, planeBytes), cb, 0, p[k].u);
            st_raw<T, true>(make_rsrc(a.outV + (size_t)(z + k) * plane, planeBytes), cb, 0, p[k].v);
        }
    }
    for (; z < z1; ++z) {
        const mm::StoredPair<T> p = overlay(z, top(z));
        st_raw<T, true>(make_rsrc(a.outU + (size_t)z * plane, planeBytes), cb, 0, p.u);
        st_raw<T, true>(make_rsrc(a.outV + (size_t)z * plane, planeBytes), cb, 0, p.v);
    }
}

template <int ST, typename T>
void launch_overlay_st(int ot, dim3 grid, const MergeOverlayVectorTypedArgs<T>& a, hipStream_t stream)
{
    const dim3 block(kTileX, kTileY, 1);
    if (ot == 1) merge_overlay_vector_typed_kernel<ST, 1, T><<<grid, block, 0, stream>>>(a);
    else if (ot == 2) merge_overlay_vector_typed_kernel<ST, 2, T><<<grid, block, 0, stream>>>(a);
    else merge_overlay_vector_typed_kernel<ST, 4, T><<<grid, block, 0, stream>>>(a);
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
    void* get() const { return p_; }

private:
    void* p_ = nullptr;
    hipStream_t stream_;
};

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
    const size_t innerCells = oi.outX * oi.outY;
    Scratch s(2 * nz * innerCells * sizeof(T), stream);  // Su, then Sv
    T *su = static_cast<T*>(s.get()), *sv = su + nz * innerCells;
    const dim3 block(kTileX, kTileY, 1);
    const mm::ComponentOps<T> opsU = component_ops<T>(in.innerUPacking, in.outerUPacking), opsV = component_ops<T>(in.innerVPacking, in.outerVPacking);
    const T fillIu = static_cast<T>(in.innerUPacking.fill), fillIv = static_cast<T>(in.innerVPacking.fill);
    const T fillOu = static_cast<T>(in.outerUPacking.fill), fillOv = static_cast<T>(in.outerVPacking.fill);
    {
        MergeSmoothVectorTypedArgs<T> a{};
        const dim3 grid = tile_grid(oi.outX, oi.outY, nz, a.zPerBlock);
        a.oi = pair_plan_ref<T>(oi, in.outerUPacking.fill, in.outerVPacking.fill);
        a.rotOI = rotOI.cossin.get();
        a.innerU = static_cast<const T*>(in.d_innerU);
        a.innerV = static_cast<const T*>(in.d_innerV);
        a.outerU = static_cast<const T*>(in.d_outerU);
        a.outerV = static_cast<const T*>(in.d_outerV);
        a.su = su;
        a.sv = sv;
        a.nx = (uint32_t)oi.outX;
        a.ny = (uint32_t)oi.outY;
        a.nz = (uint32_t)nz;
        a.tw = m.transitionWidth;
        a.bw = m.borderWidth;
        a.useOuter = m.useOuter ? 1 : 0;
        a.fillOu = fillOu;
        a.fillOv = fillOv;
        a.opsU = opsU;
        a.opsV = opsV;
        switch (stencil_of(oi)) {
        case 1: merge_smooth_vector_typed_kernel<1, T><<<grid, block, 0, stream>>>(a); break;
        case 2: merge_smooth_vector_typed_kernel<2, T><<<grid, block, 0, stream>>>(a); break;
        default: merge_smooth_vector_typed_kernel<4, T><<<grid, block, 0, stream>>>(a); break;
        }
        FA_HIP(hipGetLastError());
    }
    MergeOverlayVectorTypedArgs<T> a{};
    const dim3 grid = tile_grid(st.outX, st.outY, nz, a.zPerBlock);
    a.st = pair_plan_ref<T>(st, in.innerUPacking.fill, in.innerVPacking.fill);
    a.ot = pair_plan_ref<T>(ot, in.outerUPacking.fill, in.outerVPacking.fill);
    a.rotST = rotST.cossin.get();
    a.rotOT = rotOT.cossin.get();
    a.su = su;
    a.sv = sv;
    a.outerU = static_cast<const T*>(in.d_outerU);
    a.outerV = static_cast<const T*>(in.d_outerV);
    a.outU = static_cast<T*>(d_outU);
    a.outV = static_cast<T*>(d_outV);
    a.nx = (uint32_t)st.outX;
    a.ny = (uint32_t)st.outY;
    a.nz = (uint32_t)nz;
    a.fillIu = fillIu;
    a.fillIv = fillIv;
    a.fillOu = fillOu;
    a.fillOv = fillOv;
    a.opsU = opsU;
    a.opsV = opsV;
    const int otStencil = stencil_of(ot);
    switch (stencil_of(st)) {
    case 1: launch_overlay_st<1, T>(otStencil, grid, a, stream); break;
    case 2: launch_overlay_st<2, T>(otStencil, grid, a, stream); break;
    default: launch_overlay_st<4, T>(otStencil, grid, a, stream); break;
    }
    FA_HIP(hipGetLastError());
}

bool aligned_to(const void* p, size_t elem) { return reinterpret_cast<uintptr_t>(p) % elem == 0; }

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
