// Grid merging on variables in their stored types: what CDMBorderSmoothing::getDataSlice and
// CDMOverlay::getDataSlice compute on packed variables.  Both fields are read through getScaledDataSlice, each with its own scale,
// offset and fill value, blended in double and packed with the inner (top) variable's packing; the three regrids run on the raw
// counts as floats between data2InterpolationArray and interpolationArray2Data.  The per-cell arithmetic is merge_math.hpp's.
//   border_smooth_typed_kernel<TI, TO>   S = pack(smooth(unpack(I), unpack(OI))) on a batch of slices, one alias-safe pass
//   overlay_typed_kernel<TI, TO>         out = pack(isnan(unpack(top)) ? unpack(base) : unpack(top)), one alias-safe pass
//   merge_smooth_typed_kernel<STENCIL, T>    steps 1 and 2 fused: a lane per inner cell evaluates the outer -> inner plan entry only
//                                            where the smoothing reads the outer, rounds it to T, blends and writes S in T
//   merge_overlay_typed_kernel<ST, OT, T>    steps 3 and 4 fused: a lane per target cell evaluates the inner -> target entry on S and
//                                            the outer -> target entry on O only where the first gives the fill value
// The fused pair serves T = short and unsigned short; every other pair of types takes the chain of five launches.  Tile, slices in
// flight, per-slice buffer descriptors and dropped loads of invalid entries are those of merge.hip.  The elementwise kernels index
// plain pointers: their elements are up to 8 bytes wide, beyond what a 32-bit buffer range holds of a slice.
// Built with -ffp-contract=off.
#include "gather_entry.hpp"
#include "merge_launch.hpp"
#include "merge_math.hpp"
#include "plan.hpp"

namespace fimex_amd {

namespace {

namespace mm = merge_math;

using namespace merge_launch;
template <typename T>
using TypedPlan = PlanRef<T, 1>;  // one source field: its fill value as data2InterpolationArray takes it

template <typename TI, typename TO>
struct CellOps {
    mm::Unpack<TI> unI;
    mm::Unpack<TO> unO;
    mm::Pack<TI> pack;
};

template <typename TI, typename TO>
CellOps<TI, TO> cell_ops(const fimex_amd_packing& pi, const fimex_amd_packing& po)
{
    return {mm::make_unpack<TI>(pi.fill, pi.scale, pi.offset), mm::make_unpack<TO>(po.fill, po.scale, po.offset),
            mm::make_pack<TI>(pi.fill, pi.scale, pi.offset)};
}

template <typename TI, typename TO>
struct SmoothTypedArgs {
    const TI* inner;  // [nz][ny][nx]
    const TO* outer;
    TI* out;
    Tile tile;
    Smoothing sm;
    CellOps<TI, TO> ops;
};

// every lane reads its cell of both inputs before it writes it: out may be inner, or outer where the element sizes agree
template <typename TI, typename TO>
__global__ void __launch_bounds__(kBlock) border_smooth_typed_kernel(const SmoothTypedArgs<TI, TO> a)
{
    const Cell c(a.tile);
    if (!c.inside) return;
    const mm::SmoothClass cls = mm::smooth_class(c.x, c.y, a.tile.nx, a.tile.ny, a.sm.tw, a.sm.bw);
    const bool useOuter = a.sm.useOuter != 0;
    for_z_groups<kAhead>(c.z0, c.z1, [&](uint32_t z, auto n) {
        constexpr int N = decltype(n)::value;
        TI vi[N];
        TO vo[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            vi[k] = a.inner[(size_t)(z + k) * c.plane + c.cell];
            vo[k] = a.outer[(size_t)(z + k) * c.plane + c.cell];
        }
#pragma unroll
        for (int k = 0; k < N; ++k)
            a.out[(size_t)(z + k) * c.plane + c.cell] = mm::smooth_cell_typed<TI, TO>(cls, vi[k], vo[k], a.ops.unI, a.ops.unO, a.ops.pack, useOuter);
    });
}

// A workgroup takes kAhead * kBlock consecutive values; a lane reads its values before it writes them.
template <typename TI, typename TO>
__global__ void __launch_bounds__(kBlock) overlay_typed_kernel(const TI* top, const TO* base, TI* out, size_t n, const CellOps<TI, TO> ops)
{
    const size_t i0 = (size_t)blockIdx.x * (kAhead * kBlock) + threadIdx.x;
    TI t[kAhead];
    TO b[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
        const size_t i = i0 + (size_t)k * kBlock;
        t[k] = i < n ? top[i] : TI(0);
        b[k] = i < n ? base[i] : TO(0);
    }
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
        const size_t i = i0 + (size_t)k * kBlock;
        if (i < n) out[i] = mm::overlay_cell_typed<TI, TO>(t[k], b[k], ops.unI, ops.unO, ops.pack);
    }
}

template <typename T>
struct MergeSmoothTypedArgs {
    TypedPlan<T> oi;     // outer -> inner grid
    const T* inner;      // [nz][ny][nx]
    const T* outer;      // [nz] source slices of oi
    T* s;                // [nz][ny][nx]
    Tile tile;
    Smoothing sm;
    T fillO;             // what interpolationArray2Data writes for an undefined outer value
    CellOps<T, T> ops;
};

// steps 1 and 2: the regrid's float result is rounded to the stored type, as regridT leaves it
template <int STENCIL, typename T>
__global__ void __launch_bounds__(kBlock) merge_smooth_typed_kernel(const MergeSmoothTypedArgs<T> a)
{
    const Cell c(a.tile);
    if (!c.inside) return;
    const mm::SmoothClass cls = mm::smooth_class(c.x, c.y, a.tile.nx, a.tile.ny, a.sm.tw, a.sm.bw);
    const GatherEntry<STENCIL, T> e = a.oi.template entry<STENCIL>(c.cell);
    const bool useOuter = a.sm.useOuter != 0;
    const uint32_t cb = c.offset<T>();
    for_z_groups<kAhead>(c.z0, c.z1, [&](uint32_t z, auto n) {
        constexpr int N = decltype(n)::value;
        T vi[N], s[N];
#pragma unroll
        for (int k = 0; k < N; ++k) vi[k] = ld_raw<T>(c.slice(a.inner, z + k), cb);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const bool need = mm::needs_outer<double>(cls, a.ops.unI(vi[k]), useOuter);
            const float f = need ? e.value(a.oi.slice(a.outer, z + k)) : 0.f;
            s[k] = mm::smooth_cell_typed<T, T>(cls, vi[k], mm::round_to_stored<T>(f, a.fillO), a.ops.unI, a.ops.unO, a.ops.pack, useOuter);
        }
#pragma unroll
        for (int k = 0; k < N; ++k) st_raw<T, false>(c.slice(a.s, z + k), cb, 0, s[k]);
    });
}

template <typename T>
struct MergeOverlayTypedArgs {
    TypedPlan<T> st;     // smoothed inner -> target
    TypedPlan<T> ot;     // outer -> target
    const T* s;          // [nz] source slices of st
    const T* outer;      // [nz] source slices of ot
    T* out;              // [nz][ny][nx]
    Tile tile;
    T fillI, fillO;
    CellOps<T, T> ops;
};

// steps 3 and 4: an invalid inner -> target entry issues no load from S, and the outer -> target entry is evaluated only where the
// first regrid leaves the inner's fill value
template <int ST, int OT, typename T>
__global__ void __launch_bounds__(kBlock) merge_overlay_typed_kernel(const MergeOverlayTypedArgs<T> a)
{
    const Cell c(a.tile);
    if (!c.inside) return;
    const GatherEntry<ST, T> es = a.st.template entry<ST>(c.cell);
    const GatherEntry<OT, T> eo = a.ot.template entry<OT>(c.cell);
    const uint32_t cb = c.offset<T>();
    for_z_groups<kAhead>(c.z0, c.z1, [&](uint32_t z, auto n) {
        constexpr int N = decltype(n)::value;
        float top[N], base[N];
#pragma unroll
        for (int k = 0; k < N; ++k) top[k] = es.value(a.st.slice(a.s, z + k));
#pragma unroll
        for (int k = 0; k < N; ++k)
            base[k] = mm::overlay_needs_base<T>(mm::round_to_stored<T>(top[k], a.fillI), a.ops.unI) ? eo.value(a.ot.slice(a.outer, z + k)) : 0.f;
#pragma unroll
        for (int k = 0; k < N; ++k)
            st_raw<T, true>(c.slice(a.out, z + k), cb, 0,
                            mm::regrid_overlay_cell_typed<T, T>(top[k], a.fillI, base[k], a.fillO, a.ops.unI, a.ops.unO, a.ops.pack));
    });
}

template <typename T>
void merge_fused_t(const fimex_amd_merge_plan& m, const void* d_inner, const fimex_amd_packing& pi, const void* d_outer, const fimex_amd_packing& po,
                   size_t nz, void* d_out, hipStream_t stream)
{
    const fimex_amd_regrid_plan &oi = *m.outerToInner, &st = *m.innerToTarget, &ot = *m.outerToTarget;
    Scratch s(nz * oi.outX * oi.outY * sizeof(T), stream);
    const T *inner = static_cast<const T*>(d_inner), *outer = static_cast<const T*>(d_outer);
    const T fillI = static_cast<T>(pi.fill), fillO = static_cast<T>(po.fill);
    const CellOps<T, T> ops = cell_ops<T, T>(pi, po);
    {
        MergeSmoothTypedArgs<T> a{plan_ref<T>(oi, po.fill), inner, outer, s.get<T>(), {}, smoothing(m.transitionWidth, m.borderWidth, m.useOuter), fillO, ops};
        const dim3 grid = tile_grid(oi.outX, oi.outY, nz, a.tile);
        with_stencil(oi, [&](auto stencil) { merge_smooth_typed_kernel<decltype(stencil)::value, T><<<grid, tile_block(), 0, stream>>>(a); });
        FA_HIP(hipGetLastError());
    }
    MergeOverlayTypedArgs<T> a{plan_ref<T>(st, pi.fill), plan_ref<T>(ot, po.fill), s.get<T>(), outer, static_cast<T*>(d_out), {}, fillI, fillO, ops};
    const dim3 grid = tile_grid(st.outX, st.outY, nz, a.tile);
    with_stencil(st, [&](auto sts) {
        with_stencil(ot, [&](auto ots) {
            merge_overlay_typed_kernel<decltype(sts)::value, decltype(ots)::value, T><<<grid, tile_block(), 0, stream>>>(a);
        });
    });
    FA_HIP(hipGetLastError());
}

// regridT: fimex_amd_regrid_apply_typed_device's work with stream-ordered temporaries
void regrid_typed(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double fill, void* d_out, hipStream_t stream)
{
    if (launch_typed_apply(plan, d_in, cdmType, nz, fill, d_out, stream)) return;
    const size_t inCells = nz * plan.inX * plan.inY, outCells = nz * plan.outX * plan.outY;
    Scratch fIn(inCells * sizeof(float), stream), fOut(outCells * sizeof(float), stream);
    launch_data2interpolation(d_in, cdmType, inCells, fill, fIn.get<float>(), stream);
    apply_plan_device(plan, fIn.get<float>(), nz, fOut.get<float>(), stream);
    launch_interpolation2data(fOut.get<float>(), outCells, cdmType, fill, d_out, stream);
}

}  // namespace

// every argument has been checked (capi_merge_typed.hip)
void launch_border_smooth_typed(const void* d_inner, const fimex_amd_packing& pi, const void* d_outerOnInner, const fimex_amd_packing& po, void* d_out,
                                size_t nx, size_t ny, size_t nz, size_t transitionWidth, size_t borderWidth, bool useOuter, hipStream_t stream)
{
    if (nz == 0) return;
    Tile tile;
    const dim3 grid = tile_grid(nx, ny, nz, tile);
    for_cdm_type(pi.type, [&](auto ti) {
        for_cdm_type(po.type, [&](auto to) {
            using TI = decltype(ti);
            using TO = decltype(to);
            const SmoothTypedArgs<TI, TO> a{static_cast<const TI*>(d_inner), static_cast<const TO*>(d_outerOnInner), static_cast<TI*>(d_out), tile,
                                            smoothing(transitionWidth, borderWidth, useOuter), cell_ops<TI, TO>(pi, po)};
            border_smooth_typed_kernel<TI, TO><<<grid, tile_block(), 0, stream>>>(a);
        });
    });
    FA_HIP(hipGetLastError());
}

void launch_overlay_typed(const void* d_top, const fimex_amd_packing& pt, const void* d_base, const fimex_amd_packing& pb, void* d_out, size_t n,
                          hipStream_t stream)
{
    if (n == 0) return;
    const size_t blocks = ceil_div(n, (size_t)kAhead * kBlock);
    FA_REQUIRE(blocks <= 0x7fffffffu, "too many values for one launch");
    for_cdm_type(pt.type, [&](auto ti) {
        for_cdm_type(pb.type, [&](auto to) {
            using TI = decltype(ti);
            using TO = decltype(to);
            overlay_typed_kernel<TI, TO><<<(uint32_t)blocks, kBlock, 0, stream>>>(static_cast<const TI*>(d_top), static_cast<const TO*>(d_base),
                                                                                  static_cast<TI*>(d_out), n, cell_ops<TI, TO>(pt, pb));
        });
    });
    FA_HIP(hipGetLastError());
}

// The dispatch rule of the fused pair: both variables short, or both unsigned short; the three buffers aligned to
// their element; both fill values representable in the type, so that the kernels' casts of them are those of the chain; not
// switched off in the tuning build.  false: not served, nothing launched.
bool launch_merge_typed_fused(const fimex_amd_merge_plan& m, const void* d_inner, const fimex_amd_packing& pi, const void* d_outer,
                              const fimex_amd_packing& po, size_t nz, void* d_out, hipStream_t stream)
{
    if (pi.type != po.type || (pi.type != FIMEX_AMD_CDM_SHORT && pi.type != FIMEX_AMD_CDM_USHORT)) return false;
    if (!aligned_to(d_inner, 2) || !aligned_to(d_outer, 2) || !aligned_to(d_out, 2)) return false;
    if (!scaled_fill_representable(pi.type, pi.fill) || !scaled_fill_representable(po.type, po.fill)) return false;
    if (tuning("MERGE_TYPED_FUSED", 1) == 0) return false;
    if (nz == 0) return true;
    if (pi.type == FIMEX_AMD_CDM_SHORT) merge_fused_t<short>(m, d_inner, pi, d_outer, po, nz, d_out, stream);
    else merge_fused_t<unsigned short>(m, d_inner, pi, d_outer, po, nz, d_out, stream);
    return true;
}

// The same four steps as the reference runs them, five launches on temporaries of the stored types: regridT three times and the
// two elementwise kernels
void launch_merge_typed_chain(const fimex_amd_merge_plan& m, const void* d_inner, const fimex_amd_packing& pi, const void* d_outer,
                              const fimex_amd_packing& po, size_t nz, void* d_out, hipStream_t stream)
{
    if (nz == 0) return;
    const fimex_amd_regrid_plan &oi = *m.outerToInner, &st = *m.innerToTarget, &ot = *m.outerToTarget;
    const size_t innerCells = nz * oi.outX * oi.outY, targetCells = nz * st.outX * st.outY;
    const size_t sizeI = cdm_type_size(pi.type), sizeO = cdm_type_size(po.type);
    Scratch onInner(innerCells * sizeO, stream), s(innerCells * sizeI, stream), top(targetCells * sizeI, stream), base(targetCells * sizeO, stream);
    regrid_typed(oi, d_outer, po.type, nz, po.fill, onInner.get(), stream);                                                        // step 1
    launch_border_smooth_typed(d_inner, pi, onInner.get(), po, s.get(), oi.outX, oi.outY, nz, m.transitionWidth, m.borderWidth, m.useOuter,
                               stream);                                                                                            // step 2
    regrid_typed(st, s.get(), pi.type, nz, pi.fill, top.get(), stream);                                                            // step 3
    regrid_typed(ot, d_outer, po.type, nz, po.fill, base.get(), stream);
    launch_overlay_typed(top.get(), pi, base.get(), po, d_out, targetCells, stream);                                               // step 4
}

}  // namespace fimex_amd
