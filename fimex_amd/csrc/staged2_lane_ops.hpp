// What a lane does to single elements in the kernels of the second staged form that convert or rotate: reading stored 1- and
// 2-byte elements out of the staged image and rounding results back to the stored type (staged2_typed.hip,
// staged2_vector_typed.hip), and the rotation of one cell of a vector pair (staged2_vector.hip, staged2_vector_typed.hip).
#pragma once

#include "staged_common.hpp"
#include "typed_convert.hpp"

namespace fimex_amd {
namespace {

template <typename T>
__device__ __forceinline__ float lds_one(const char* buf, uint32_t byteOff, float bad, bool hasBad)
{
    return as_float_nan(*reinterpret_cast<const T*>(buf + byteOff), bad, hasBad);
}
// two neighbouring 1- or 2-byte elements at element offset `byteOff / sizeof(T)` of the staged image
// (alignedOff = byteOff & ~3; shift = byteOff * 8: v_alignbit_b32 takes the low five bits, (byteOff & 3) * 8 -- both are
// computed once per lane, outside the slice loop),
// as they are stored, converted but not yet compared with the fill value (the interior form tests all four
// stencil values at once: any fill value among them makes the result undefined, whatever its weight -- 0 * NaN is NaN)
template <typename T>
__device__ __forceinline__ void lds_pair2_raw(const char* buf, uint32_t alignedOff, uint32_t shift, float& first, float& second)
{
    const uint32_t* w = reinterpret_cast<const uint32_t*>(buf + alignedOff);
    const uint32_t both = __builtin_amdgcn_alignbit(w[1], w[0], shift);
    if constexpr (sizeof(T) == 2) {
        first = (float)(T)(unsigned short)(both & 0xffffu);
        second = (float)(T)(unsigned short)(both >> 16);
    } else {
        first = (float)(T)(unsigned char)(both & 0xffu);
        second = (float)(T)(unsigned char)((both >> 8) & 0xffu);
    }
}
template <typename T>
__device__ __forceinline__ void lds_pair2(const char* buf, uint32_t alignedOff, uint32_t shift, float bad, bool hasBad, float& first, float& second)
{
    const uint32_t* w = reinterpret_cast<const uint32_t*>(buf + alignedOff);
    const uint32_t both = __builtin_amdgcn_alignbit(w[1], w[0], shift);
    if constexpr (sizeof(T) == 2) {
        first = as_float_nan((T)(unsigned short)(both & 0xffffu), bad, hasBad);
        second = as_float_nan((T)(unsigned short)(both >> 16), bad, hasBad);
    } else {
        first = as_float_nan((T)(unsigned char)(both & 0xffu), bad, hasBad);
        second = as_float_nan((T)(unsigned char)((both >> 8) & 0xffu), bad, hasBad);
    }
}
// interpolationArray2Data for results of THESE kernels: NaN -> fill, else MetNoFimex::round (lround) and the reference's casts
// long -> int -> T (typed_convert.hpp: from_float_fill).  The results are stored elements or convex combinations of four
// of them, |v| < 2^17 (the extreme is unsigned short without a fill value: up to 65535), or such values of a vector pair after
// its rotation, |u cos - v sin| <= sqrt(u^2 + v^2) (1 + a few ulp) < 2^18: still far inside the int range, so the branch of
// from_float_fill for values beyond it cannot be taken and is left out, the rest is the same arithmetic without branches (the
// fraction v - trunc(v) is exact in float).  A rotated value may leave T's range; the reference's int -> T cast then wraps, and
// so do the callers, which keep the low bits of what this returns.
template <typename T>
__device__ __forceinline__ uint32_t round_bits(float v, T fill)
{
    const float t = truncf(v);
    const float r = t + ((fabsf(v - t) >= 0.5f) ? copysignf(1.f, v) : 0.f);
    const int i = (v != v) ? (int)fill : (int)r;
    return (uint32_t)i;
}
// results r0 (cell c) and r1 (cell c + 1) of one pair; offsets in BYTES of the typed slice, ~0u = not mine
constexpr int kTypedStoreAux = 2;  // non-temporal (written through as well -- sc1 nt, the float kernel's policy -- these 4-byte-per-lane stores of half as many bytes lose 9 %: 1.48 against 1.35 ms)
template <typename T, bool PAIR>
__device__ __forceinline__ void store_pair(rsrc_t ro, uint32_t off0, uint32_t off1, float r0, float r1, T fill)
{
    constexpr uint32_t kMask = sizeof(T) == 2 ? 0xffffu : 0xffu;
    const uint32_t b0 = round_bits<T>(r0, fill) & kMask, b1 = round_bits<T>(r1, fill) & kMask;
    if constexpr (PAIR) {  // both cells exist or neither (even row length, even tile widths)
        if constexpr (sizeof(T) == 2) __builtin_amdgcn_raw_buffer_store_b32(b0 | (b1 << 16), ro, off0, 0, kTypedStoreAux);
        else __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(b0 | (b1 << 8)), ro, off0, 0, 2);
        (void)off1;
    } else if constexpr (sizeof(T) == 2) {
        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)b0, ro, off0, 0, 2);
        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)b1, ro, off1, 0, 2);
    } else {
        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)b0, ro, off0, 0, 2);
        __builtin_amdgcn_raw_buffer_store_b8((unsigned char)b1, ro, off1, 0, 2);
    }
}

// src/interpolation.c:796-810 on one cell, as rotate() of vector.hip: float -> double products, one double add / sub, -> float
__device__ __forceinline__ void rotate_pair(float u, float v, double c, double s, float& uOut, float& vOut)
{
    const double un = (double)u * c - (double)v * s;  // :804
    const double vn = (double)u * s + (double)v * c;  // :805
    uOut = (float)un;
    vOut = (float)vn;
}

}  // namespace
}  // namespace fimex_amd
