// One plan entry of a backward plan in byte offsets, for the kernels that gather per lane (gather.hip, merge.hip): the decoder of
// stencil_math.hpp plus the loads and stores through buffer descriptors and the element conversions of a slice's stored type.
// Device only.
//
// Addressing: buffer instructions.  A 128-bit descriptor (4 SGPRs) is built from wave-uniform values; the per-lane part of an
// address is one 32-bit byte offset VGPR (plus an immediate), a slice index goes into the scalar offset.  No 64-bit per-lane
// address arithmetic, which keeps the register budget for loads in flight.  rsrc_t / make_rsrc: common.hpp.
#pragma once

#include "stencil_math.hpp"
#include "typed_convert.hpp"

namespace fimex_amd {

template <typename T>
__device__ __forceinline__ T ld_raw(rsrc_t r, uint32_t voff, uint32_t soff = 0)
{
    if (sizeof(T) == 1) return (T)__builtin_amdgcn_raw_buffer_load_b8(r, voff, soff, 0);
    if (sizeof(T) == 2) return (T)__builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, 0);
    return (T)__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
}
// outputs are written once and never re-read by the kernel that writes them: non-temporal (aux = 2) unless NT is false
template <typename T, bool NT = true>
__device__ __forceinline__ void st_raw(rsrc_t r, uint32_t voff, uint32_t soff, T v)
{
    if (sizeof(T) == 1) __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, r, voff, soff, NT ? 2 : 0);
    else if (sizeof(T) == 2) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)v, r, voff, soff, NT ? 2 : 0);
    else __builtin_amdgcn_raw_buffer_store_b32((unsigned int)v, r, voff, soff, NT ? 2 : 0);
}
__device__ __forceinline__ float ld(rsrc_t r, uint32_t voff, uint32_t soff = 0) { return __uint_as_float(ld_raw<uint32_t>(r, voff, soff)); }
__device__ __forceinline__ void st_stream(rsrc_t r, uint32_t voff, uint32_t soff, float v) { st_raw<uint32_t, true>(r, voff, soff, __float_as_uint(v)); }
__device__ __forceinline__ void st_plain(rsrc_t r, uint32_t voff, uint32_t soff, float v) { st_raw<uint32_t, false>(r, voff, soff, __float_as_uint(v)); }

// ---- the elements of a slice.  Stored types: an element of T is read as it lies in the file, becomes float with the
// fill value as NaN in the register (data2InterpolationArray), and a result goes back to T with NaN as the fill value
// (interpolationArray2Data) -- typed_convert.hpp.  Params is what the host passes; the conversions of it run on the device.
template <typename T>
struct Element {
    struct Params {
        float bad;       // the fill value narrowed to float (mifi_bad2nanf's parameter)
        int hasBad;
        double fillOut;  // the fill value as interpolationArray2Data receives it
    };
    float bad;
    bool hasBad;
    T fill;  // ScaleValue's newFill_ (Utils.h:456)
    __device__ __forceinline__ explicit Element(const Params& p) : bad(p.bad), hasBad(p.hasBad != 0), fill(static_cast<T>(p.fillOut)) {}
    __device__ __forceinline__ float load(rsrc_t r, uint32_t voff, uint32_t soff) const { return as_float_nan(ld_raw<T>(r, voff, soff), bad, hasBad); }
    template <bool NT = true>
    __device__ __forceinline__ void store(rsrc_t r, uint32_t voff, uint32_t soff, float v) const
    {
        st_raw<T>(r, voff, soff, from_float_fill<T>(v, fill));
    }
};
template <>
struct Element<float> {
    struct Params {};
    __device__ __forceinline__ explicit Element(const Params& = Params()) {}
    __device__ __forceinline__ float load(rsrc_t r, uint32_t voff, uint32_t soff) const { return ld(r, voff, soff); }
    template <bool NT = true>
    __device__ __forceinline__ void store(rsrc_t r, uint32_t voff, uint32_t soff, float v) const
    {
        if (NT) st_stream(r, voff, soff, v);
        else st_plain(r, voff, soff, v);
    }
};

// An undefined entry (kInvalidPos) is parked at a lane offset beyond every slice, with zero steps: the buffer range check drops
// its loads, so it reads nothing and the lane stays on the common path; combine then gives the undefined value.
constexpr uint32_t kDropped = 0xFFFFFFFCu;  // a slice has fewer than 2^30 cells of at most 4 bytes: its bytes end below this offset

template <int STENCIL, typename T>
struct GatherEntry {
    StencilEntry<STENCIL> e;
    Element<T> el;
    uint32_t pb, colb, rowb;  // byte offset of the first cell, byte steps to the next column and row

    GatherEntry() = default;
    __device__ __forceinline__ GatherEntry(uint32_t pos, frac_t<STENCIL> xf, frac_t<STENCIL> yf, uint32_t ix, const Element<T>& el_ = Element<T>())
        : e(decode_entry<STENCIL>(pos, xf, yf, ix)), el(el_)
    {
        pb = e.valid ? e.first * (uint32_t)sizeof(T) : kDropped;
        colb = e.dx * (uint32_t)sizeof(T);
        rowb = e.dy * (uint32_t)sizeof(T);
    }
    __device__ __forceinline__ bool valid() const { return e.valid; }
    // the loads of one slice: rsrc spans it, or several slices with this one at byte sliceOffset
    __device__ __forceinline__ void fetch(rsrc_t rsrc, uint32_t sliceOffset, float (&taps)[STENCIL][STENCIL]) const
    {
#pragma unroll
        for (int i = 0; i < STENCIL; ++i)
#pragma unroll
            for (int j = 0; j < STENCIL; ++j) taps[i][j] = el.load(rsrc, pb + i * rowb + j * colb, sliceOffset);
    }
    __device__ __forceinline__ float combine(const float (&taps)[STENCIL][STENCIL]) const { return e.valid ? e.combine(taps) : undefined_f(); }
    __device__ __forceinline__ float value(rsrc_t rsrc) const
    {
        float taps[STENCIL][STENCIL];
        fetch(rsrc, 0, taps);
        return combine(taps);
    }
};

}  // namespace fimex_amd
