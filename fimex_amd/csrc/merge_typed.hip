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

using merge_launch::kAhead;
using merge_launch::kTileX;
using merge_launch::kTileY;
using merge_launch::stencil_of;
using merge_launch::tile_grid;

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
    uint32_t nx, ny, nz, zPerBlock;
    uint64_t tw, bw;
    int useOuter;
    CellOps<TI, TO> ops;
};

// every lane reads its cell of both inputs before it writes it: out may be inner, or outer where the element sizes agree
template <typename TI, typename TO>
__global__ void __launch_bounds__(kBlock) border_smooth_typed_kernel(const SmoothTypedArgs<TI, TO> a)
{
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= a.nx || y >= a.ny) return;
    const mm::SmoothClass c = mm::smooth_class(x, y, a.nx, a.ny, a.tw, a.bw);
    const bool useOuter = a.useOuter != 0;
    const size_t plane = (size_t)a.nx * a.ny, cell = (size_t)y * a.nx + x;
    uint32_t z = blockIdx.z * a.zPerBlock;
    const uint32_t z1 = min(a.nz, z + a.zPerBlock);
    for (; z + kAhead <= z1; z += kAhead) {
        TI vi[kAhead];
        TO vo[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            vi[k] = a.inner[(size_t)(z + k) * plane + cell];
            vo[k] = a.outer[(size_t)(z + k) * plane + cell];
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k)
            a.out[(size_t)(z + k) * plane + cell] = mm::smooth_cell_typed<TI, TO>(c, vi[k], vo[k], a.ops.unI, a.ops.unO, a.ops.pack, useOuter);
    }
    for (; z < z1; ++z) {
        const TI vi = a.inner[(size_t)z * plane + cell];
        const TO vo = a.outer[(size_t)z * plane + cell];
        a.out[(size_t)z * plane + cell] = mm::smooth_cell_typed<TI, TO>(c, vi, vo, a.ops.unI, a.ops.unO, a.ops.pack, useOuter);
    }
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

// ---- a backward plan's arrays on slices of T; an entry is decoded once per cell and evaluated slice by slice (gather_entry.hpp:
// an undefined entry issues loads that are dropped and gives NaN, so the lane stays on the common path)
template <typename T>
struct TypedPlanRef {
    const uint32_t* pos;
    const float *xf, *yf;
    const double *xfd, *yfd;
    uint32_t ix;       // source row length
    uint32_t inBytes;  // bytes of a source slice
    size_t inLayer;    // cells of a source slice
    typename Element<T>::Params el;  // the source's fill value, as data2InterpolationArray takes it

    template <int STENCIL>
    __device__ __forceinline__ GatherEntry<STENCIL, T> entry(uint32_t cell) const
    {
        const Element<T> e(el);
        if constexpr (STENCIL == 4) return {pos[cell], xfd[cell], yfd[cell], ix, e};
        else if constexpr (STENCIL == 2) return {pos[cell], xf[cell], yf[cell], ix, e};
        else return {pos[cell], 0.f, 0.f, ix, e};
    }
};

template <typename T>
struct MergeSmoothTypedArgs {
    TypedPlanRef<T> oi;  // outer -> inner grid
    const T* inner;      // [nz][ny][nx]
    const T* outer;      // [nz] source slices of oi
    T* s;                // [nz][ny][nx]
    uint32_t nx, ny, nz, zPerBlock;
    uint64_t tw, bw;
    int useOuter;
    T fillO;             // what interpolationArray2Data writes for an undefined outer value
    CellOps<T, T> ops;
};

// steps 1 and 2 on one cell of one slice: the regrid's float result is rounded to the stored type, as regridT leaves it
template <int STENCIL, typename T>
__device__ __forceinline__ T merge_smooth_cell(const MergeSmoothTypedArgs<T>& a, const mm::SmoothClass& c, const GatherEntry<STENCIL, T>& e, T vi,
                                               uint32_t z, bool useOuter)
{
    const bool need = mm::needs_outer<double>(c, a.ops.unI(vi), useOuter);
    const float f = need ? e.value(make_rsrc(a.outer + (size_t)z * a.oi.inLayer, a.oi.inBytes)) : 0.f;
    return mm::smooth_cell_typed<T, T>(c, vi, mm::round_to_stored<T>(f, a.fillO), a.ops.unI, a.ops.unO, a.ops.pack, useOuter);
}

template <int STENCIL, typename T>
__global__ void __launch_bounds__(kBlock) merge_smooth_typed_kernel(const MergeSmoothTypedArgs<T> a)
{
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= a.nx || y >= a.ny) return;
    const uint32_t cell = y * a.nx + x, cb = cell * (uint32_t)sizeof(T);
    const mm::SmoothClass c = mm::smooth_class(x, y, a.nx, a.ny, a.tw, a.bw);
    const GatherEntry<STENCIL, T> e = a.oi.template entry<STENCIL>(cell);
    const bool useOuter = a.useOuter != 0;
    const size_t plane = (size_t)a.nx * a.ny;
    const uint32_t planeBytes = (uint32_t)plane * (uint32_t)sizeof(T);
    uint32_t z = blockIdx.z * a.zPerBlock;
    const uint32_t z1 = min(a.nz, z + a.zPerBlock);
    for (; z + kAhead <= z1; z += kAhead) {
        T vi[kAhead], s[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) vi[k] = ld_raw<T>(make_rsrc(a.inner + (size_t)(z + k) * plane, planeBytes), cb);
#pragma unroll
        for (int k = 0; k < kAhead; ++k) s[k] = merge_smooth_cell<STENCIL, T>(a, c, e, vi[k], z + k, useOuter);
#pragma unroll
        for (int k = 0; k < kAhead; ++k) st_raw<T, false>(make_rsrc(a.s + (size_t)(z + k) * plane, planeBytes), cb, 0, s[k]);
    }
    for (; z < z1; ++z) {
        const T vi = ld_raw<T>(make_rsrc(a.inner + (size_t)z * plane, planeBytes), cb);
        st_raw<T, false>(make_rsrc(a.s + (size_t)z * plane, planeBytes), cb, 0, merge_smooth_cell<STENCIL, T>(a, c, e, vi, z, useOuter));
    }
}

template <typename T>
struct MergeOverlayTypedArgs {
    TypedPlanRef<T> st;  // smoothed inner -> target
    TypedPlanRef<T> ot;  // outer -> target
    const T* s;          // [nz] source slices of st
    const T* outer;      // [nz] source slices of ot
    T* out;              // [nz][ny][nx]
    uint32_t nx, ny, nz, zPerBlock;
    T fillI, fillO;
    CellOps<T, T> ops;
};

// steps 3 and 4: an invalid inner -> target entry issues no load from S, and the outer -> target entry is evaluated only where the
// first regrid leaves the inner's fill value
template <int ST, int OT, typename T>
__global__ void __launch_bounds__(kBlock) merge_overlay_typed_kernel(const MergeOverlayTypedArgs<T> a)
{
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= a.nx || y >= a.ny) return;
    const uint32_t cell = y * a.nx + x, cb = cell * (uint32_t)sizeof(T);
    const GatherEntry<ST, T> es = a.st.template entry<ST>(cell);
    const GatherEntry<OT, T> eo = a.ot.template entry<OT>(cell);
    const size_t plane = (size_t)a.nx * a.ny;
    const uint32_t planeBytes = (uint32_t)plane * (uint32_t)sizeof(T);
    uint32_t z = blockIdx.z * a.zPerBlock;
    const uint32_t z1 = min(a.nz, z + a.zPerBlock);
    for (; z + kAhead <= z1; z += kAhead) {
        float top[kAhead], base[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) top[k] = es.value(make_rsrc(a.s + (size_t)(z + k) * a.st.inLayer, a.st.inBytes));
#pragma unroll
        for (int k = 0; k < kAhead; ++k)
            base[k] = mm::overlay_needs_base<T>(mm::round_to_stored<T>(top[k], a.fillI), a.ops.unI)
                          ? eo.value(make_rsrc(a.outer + (size_t)(z + k) * a.ot.inLayer, a.ot.inBytes))
                          : 0.f;
#pragma unroll
        for (int k = 0; k < kAhead; ++k)
            st_raw<T, true>(make_rsrc(a.out + (size_t)(z + k) * plane, planeBytes), cb, 0,
                            mm::regrid_overlay_cell_typed<T, T>(top[k], a.fillI, base[k], a.fillO, a.ops.unI, a.ops.unO, a.ops.pack));
    }
    for (; z < z1; ++z) {
        const float top = es.value(make_rsrc(a.s + (size_t)z * a.st.inLayer, a.st.inBytes));
        const float base = mm::overlay_needs_base<T>(mm::round_to_stored<T>(top, a.fillI), a.ops.unI)
                               ? eo.value(make_rsrc(a.outer + (size_t)z * a.ot.inLayer, a.ot.inBytes))
                               : 0.f;
        st_raw<T, true>(make_rsrc(a.out + (size_t)z * plane, planeBytes), cb, 0,
                        mm::regrid_overlay_cell_typed<T, T>(top, a.fillI, base, a.fillO, a.ops.unI, a.ops.unO, a.ops.pack));
    }
}

// the element parameters are those of launch_typed_gather: the fill value narrowed to float, none where that is NaN
template <typename T>
TypedPlanRef<T> plan_ref(const fimex_amd_regrid_plan& p, double fill)
{
    TypedPlanRef<T> r{};
    r.pos = p.pos.get();
    r.xf = p.xf.get();
    r.yf = p.yf.get();
    r.xfd = p.xfd.get();
    r.yfd = p.yfd.get();
    r.ix = (uint32_t)p.inX;
    r.inLayer = p.inX * p.inY;
    r.inBytes = (uint32_t)(r.inLayer * sizeof(T));
    const float bad = (float)fill;
    r.el = typename Element<T>::Params{bad, !(bad != bad), fill};
    return r;
}

template <int ST, typename T>
void launch_overlay_st(int ot, dim3 grid, const MergeOverlayTypedArgs<T>& a, hipStream_t stream)
{
    const dim3 block(kTileX, kTileY, 1);
    if (ot == 1) merge_overlay_typed_kernel<ST, 1, T><<<grid, block, 0, stream>>>(a);
    else if (ot == 2) merge_overlay_typed_kernel<ST, 2, T><<<grid, block, 0, stream>>>(a);
    else merge_overlay_typed_kernel<ST, 4, T><<<grid, block, 0, stream>>>(a);
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
void merge_fused_t(const fimex_amd_merge_plan& m, const void* d_inner, const fimex_amd_packing& pi, const void* d_outer, const fimex_amd_packing& po,
                   size_t nz, void* d_out, hipStream_t stream)
{
    const fimex_amd_regrid_plan &oi = *m.outerToInner, &st = *m.innerToTarget, &ot = *m.outerToTarget;
    const size_t innerCells = oi.outX * oi.outY;
    Scratch s(nz * innerCells * sizeof(T), stream);
    const dim3 block(kTileX, kTileY, 1);
    const CellOps<T, T> ops = cell_ops<T, T>(pi, po);
    {
        MergeSmoothTypedArgs<T> a{};
        const dim3 grid = tile_grid(oi.outX, oi.outY, nz, a.zPerBlock);
        a.oi = plan_ref<T>(oi, po.fill);
        a.inner = static_cast<const T*>(d_inner);
        a.outer = static_cast<const T*>(d_outer);
        a.s = static_cast<T*>(s.get());
        a.nx = (uint32_t)oi.outX;
        a.ny = (uint32_t)oi.outY;
        a.nz = (uint32_t)nz;
        a.tw = m.transitionWidth;
        a.bw = m.borderWidth;
        a.useOuter = m.useOuter ? 1 : 0;
        a.fillO = static_cast<T>(po.fill);
        a.ops = ops;
        switch (stencil_of(oi)) {
        case 1: merge_smooth_typed_kernel<1, T><<<grid, block, 0, stream>>>(a); break;
        case 2: merge_smooth_typed_kernel<2, T><<<grid, block, 0, stream>>>(a); break;
        default: merge_smooth_typed_kernel<4, T><<<grid, block, 0, stream>>>(a); break;
        }
        FA_HIP(hipGetLastError());
    }
    MergeOverlayTypedArgs<T> a{};
    const dim3 grid = tile_grid(st.outX, st.outY, nz, a.zPerBlock);
    a.st = plan_ref<T>(st, pi.fill);
    a.ot = plan_ref<T>(ot, po.fill);
    a.s = static_cast<const T*>(s.get());
    a.outer = static_cast<const T*>(d_outer);
    a.out = static_cast<T*>(d_out);
    a.nx = (uint32_t)st.outX;
    a.ny = (uint32_t)st.outY;
    a.nz = (uint32_t)nz;
    a.fillI = static_cast<T>(pi.fill);
    a.fillO = static_cast<T>(po.fill);
    a.ops = ops;
    const int otStencil = stencil_of(ot);
    switch (stencil_of(st)) {
    case 1: launch_overlay_st<1, T>(otStencil, grid, a, stream); break;
    case 2: launch_overlay_st<2, T>(otStencil, grid, a, stream); break;
    default: launch_overlay_st<4, T>(otStencil, grid, a, stream); break;
    }
    FA_HIP(hipGetLastError());
}

// regridT: fimex_amd_regrid_apply_typed_device's work with stream-ordered temporaries
void regrid_typed(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double fill, void* d_out, hipStream_t stream)
{
    if (launch_typed_apply(plan, d_in, cdmType, nz, fill, d_out, stream)) return;
    const size_t inCells = nz * plan.inX * plan.inY, outCells = nz * plan.outX * plan.outY;
    Scratch fIn(inCells * sizeof(float), stream), fOut(outCells * sizeof(float), stream);
    launch_data2interpolation(d_in, cdmType, inCells, fill, static_cast<float*>(fIn.get()), stream);
    apply_plan_device(plan, static_cast<const float*>(fIn.get()), nz, static_cast<float*>(fOut.get()), stream);
    launch_interpolation2data(static_cast<const float*>(fOut.get()), outCells, cdmType, fill, d_out, stream);
}

bool aligned_to(const void* p, size_t elem) { return reinterpret_cast<uintptr_t>(p) % elem == 0; }

}  // namespace

// every argument has been checked (capi_merge_typed.hip)
void launch_border_smooth_typed(const void* d_inner, const fimex_amd_packing& pi, const void* d_outerOnInner, const fimex_amd_packing& po, void* d_out,
                                size_t nx, size_t ny, size_t nz, size_t transitionWidth, size_t borderWidth, bool useOuter, hipStream_t stream)
{
    if (nz == 0) return;
    uint32_t zPerBlock = 0;
    const dim3 grid = tile_grid(nx, ny, nz, zPerBlock);
    for_cdm_type(pi.type, [&](auto ti) {
        for_cdm_type(po.type, [&](auto to) {
            using TI = decltype(ti);
            using TO = decltype(to);
            SmoothTypedArgs<TI, TO> a{};
            a.inner = static_cast<const TI*>(d_inner);
            a.outer = static_cast<const TO*>(d_outerOnInner);
            a.out = static_cast<TI*>(d_out);
            a.nx = (uint32_t)nx;
            a.ny = (uint32_t)ny;
            a.nz = (uint32_t)nz;
            a.zPerBlock = zPerBlock;
            a.tw = transitionWidth;
            a.bw = borderWidth;
            a.useOuter = useOuter ? 1 : 0;
            a.ops = cell_ops<TI, TO>(pi, po);
            border_smooth_typed_kernel<TI, TO><<<grid, dim3(kTileX, kTileY, 1), 0, stream>>>(a);
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
