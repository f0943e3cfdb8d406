// The per-cell arithmetic of grid merging, stated once for host and device: CDMBorderSmoothing_Linear::operator()
// (src/CDMBorderSmoothing_Linear.cc:41-85) with the value type as a parameter, ScaleValue<IN, OUT> (include/fimex/Utils.h:443-464)
// as getScaledDataSlice and convertDataType use it, and the cells of CDMBorderSmoothing::getDataSlice (src/CDMBorderSmoothing.cc:
// 129-139) and CDMOverlay::getDataSlice (src/CDMOverlay.cc:80-92) on two variables in their stored types, each with its own
// packing.  merge_typed.hip compiles it for the device; tests/merge_math_host.cc compiles it with a plain C++ compiler, so it
// includes nothing of HIP and uses no device builtin.  Compile with -ffp-contract=off: a * x + b and I + alpha * diff are a
// multiply and an add each, as in the reference.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>
#include <type_traits>

#if defined(__HIPCC__)
#define FA_MM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FA_MM_HD inline
#endif

namespace fimex_amd {
namespace merge_math {

// ---- CDMBorderSmoothing_Linear::operator() (:41-85), split into what depends on the cell and what depends on the values.
// size_t arithmetic that wraps, as the reference's: xmax2 = nx - bw and xmin2 = xmax2 - tw may wrap, and the comparisons decide
// the branch on the wrapped values.
enum : int { kOuter = 0, kInner = 1, kBlend = 2 };
struct SmoothClass {
    int kind;
    double alpha;  // kBlend: divided by the transition width and clamped (:79-83)
};

FA_MM_HD double dist(double dx, double dy) { return sqrt(dx * dx + dy * dy); }  // :33-35

FA_MM_HD SmoothClass smooth_class(uint64_t x, uint64_t y, uint64_t nx, uint64_t ny, uint64_t tw, uint64_t bw)
{
    const uint64_t xmin1 = bw, xmax1 = xmin1 + tw;      // :46
    const uint64_t ymin1 = bw, ymax1 = ymin1 + tw;      // :47
    const uint64_t xmax2 = nx - bw, xmin2 = xmax2 - tw;  // :48
    const uint64_t ymax2 = ny - bw, ymin2 = ymax2 - tw;  // :49
    SmoothClass c{kOuter, 0.};
    if (x < xmin1 || x >= xmax2 || y < ymin1 || y >= ymax2) return c;  // :52
    c.kind = kInner;
    if (x >= xmax1 && x < xmin2 && y >= ymax1 && y < ymin2) return c;  // :54
    c.kind = kBlend;
    double alpha = 0;
    if (x < xmax1) {  // :60-78
        if (y < ymax1) alpha = dist((double)(xmax1 - x), (double)(ymax1 - y));
        else if (y >= ymin2) alpha = dist((double)(xmax1 - x), (double)(y - ymin2));
        else alpha = (double)(xmax1 - x);
    } else if (x >= xmin2) {
        if (y < ymax1) alpha = dist((double)(x - xmin2), (double)(ymax1 - y));
        else if (y >= ymin2) alpha = dist((double)(x - xmin2), (double)(y - ymin2));
        else alpha = (double)(x - xmin2);
    } else if (y < ymax1) {
        alpha = (double)(ymax1 - y);
    } else if (y >= ymin2) {
        alpha = (double)(y - ymin2);
    }
    alpha /= (double)tw;
    if (alpha > 1) alpha = 1;
    else if (alpha < 0) alpha = 0;
    c.alpha = alpha;
    return c;
}

// MIFI_UNDEFINED_F / MIFI_UNDEFINED_D: the quiet NaN
template <typename V>
FA_MM_HD V undefined_value()
{
    return std::numeric_limits<V>::quiet_NaN();
}

// true: smooth_value reads the outer value for this inner value
template <typename V>
FA_MM_HD bool needs_outer(const SmoothClass& c, V inner, bool useOuter)
{
    return inner != inner ? useOuter : c.kind != kInner;
}

// CDMBorderSmoothing.cc:129-139 on one cell; outer is read only where needs_outer says so.  V = float: the values of a float
// interpolation array, blended in double and narrowed once; V = double: the scaled values of getScaledDataSlice, never narrowed.
template <typename V>
FA_MM_HD V smooth_value(const SmoothClass& c, V inner, V outer, bool useOuter)
{
    if (inner != inner) return useOuter ? outer : undefined_value<V>();  // :132-133
    if (c.kind == kInner || outer != outer) return inner;                 // :134-135, Linear :54-55
    if (c.kind == kOuter) return outer;                                   // Linear :52-53
    const double valueI = (double)inner, valueO = (double)outer;
    const double diff = valueO - valueI;  // :56
    if (diff == 0) return outer;          // :57-58
    return (V)(valueI + c.alpha * diff);
}

// ---- mifi_round_d and round_to_stored below are the host-and-device twins of mifi_round and from_float_fill in
// typed_convert.hpp (device only, used by the regrids on stored types): a change to either belongs in both.
// MetNoFimex::round(double) (include/fimex/Utils.h:72-75): lround, then long -> int.  Outside the range of long the
// reference is unspecified; LONG_MIN (what glibc/x86-64 yields) is kept (DESIGN.md divergence D6).
FA_MM_HD int mifi_round_d(double num)
{
    const long long r = (fabs(num) < 9223372036854775808.0) ? llround(num) : (-9223372036854775807LL - 1);
    return (int)r;
}

// ---- ScaleValue<IN, OUT> (Utils.h:443-464)
template <typename IN, typename OUT>
struct ScaleValue {
    IN oldFill;
    bool hasFill;  // false: (IN)oldFill does not exist, nothing compares equal to it
    double a, b;   // oldScale / newScale, (oldOffset - newOffset) / newScale
    OUT newFill;
    // :456-460: in double, then data_caster<OUT, double>: mifi_round for an integer OUT, a plain cast otherwise
    FA_MM_HD OUT operator()(IN in) const
    {
        if ((hasFill && in == oldFill) || (std::is_floating_point<IN>::value && in != in)) return newFill;
        const double d = a * (double)in + b;
        if (std::is_integral<OUT>::value) return (OUT)mifi_round_d(d);
        return (OUT)d;
    }
};

// static_cast<T>(v) of a double is defined: trunc(v) lies in the range of an integer T, a finite v within that of float
template <typename T>
inline bool representable(double v)
{
    if (std::is_same<T, float>::value) return !std::isfinite(v) || std::fabs(v) <= (double)std::numeric_limits<float>::max();
    if (std::is_floating_point<T>::value) return true;
    if (v != v) return false;
    const double t = std::trunc(v);
    return t >= (double)std::numeric_limits<T>::min() && t < std::ldexp(1.0, std::numeric_limits<T>::digits);
}

// a and b are formed on the host (Utils.h:453-454)
template <typename IN, typename OUT>
inline ScaleValue<IN, OUT> make_scale_value(double oldFill, double oldScale, double oldOffset, double newFill, double newScale, double newOffset)
{
    ScaleValue<IN, OUT> sv{};
    sv.hasFill = representable<IN>(oldFill);
    sv.oldFill = sv.hasFill ? static_cast<IN>(oldFill) : IN(0);
    sv.a = oldScale / newScale;
    sv.b = (oldOffset - newOffset) / newScale;
    sv.newFill = static_cast<OUT>(newFill);
    return sv;
}

// getScaledDataSlice: ScaleValue<T, double>(fill, scale, offset, MIFI_UNDEFINED_D, 1, 0)
template <typename T>
using Unpack = ScaleValue<T, double>;
template <typename T>
inline Unpack<T> make_unpack(double fill, double scale, double offset)
{
    return make_scale_value<T, double>(fill, scale, offset, undefined_value<double>(), 1., 0.);
}

// convertDataType(MIFI_UNDEFINED_D, 1, 0, type, fill, scale, offset): ScaleValue<double, T>; fill must be representable in T
template <typename T>
using Pack = ScaleValue<double, T>;
template <typename T>
inline Pack<T> make_pack(double fill, double scale, double offset)
{
    return make_scale_value<double, T>(undefined_value<double>(), 1., 0., fill, scale, offset);
}

// interpolationArray2Data (src/CDMInterpolator.cc:120-124): ScaleValue<float, T>(NaN, 1, 0, fill, 1, 0) on one value
template <typename T>
FA_MM_HD T round_to_stored(float v, T fill)
{
    if (v != v) return fill;
    if (std::is_integral<T>::value && fabsf(v) < 2147483648.f) {
        // lround of a float inside the int range, without the detour through double: the fraction v - trunc(v) is exact in
        // float, and from 2^23 on v is an integer already; then int -> T as the reference's static_cast
        const float t = truncf(v);
        return (T)(int)(t + ((fabsf(v - t) >= 0.5f) ? copysignf(1.f, v) : 0.f));
    }
    const double d = 1.0 * (double)v + 0.0;  // turns -0.0 into +0.0, as the reference does
    if (std::is_integral<T>::value) return (T)mifi_round_d(d);
    return (T)d;
}

// ---- the cells on stored types: the inner (top) variable is TI in its packing, the outer (base) variable TO in its own, the
// result TI in the inner's packing

// CDMBorderSmoothing::getDataSlice on one cell: both values scaled to double, blended in double, packed
template <typename TI, typename TO>
FA_MM_HD TI smooth_cell_typed(const SmoothClass& c, TI inner, TO outerOnInner, const Unpack<TI>& unI, const Unpack<TO>& unO, const Pack<TI>& pack,
                              bool useOuter)
{
    return pack(smooth_value<double>(c, unI(inner), unO(outerOnInner), useOuter));
}

// CDMOverlay::getDataSlice on one cell: a defined top value is unpacked and packed again, as the reference does
template <typename TI, typename TO>
FA_MM_HD TI overlay_cell_typed(TI top, TO base, const Unpack<TI>& unI, const Unpack<TO>& unO, const Pack<TI>& pack)
{
    const double vT = unI(top);
    return pack(vT != vT ? unO(base) : vT);
}

// true: overlay_cell_typed reads the base value for this top value
template <typename TI>
FA_MM_HD bool overlay_needs_base(TI top, const Unpack<TI>& unI)
{
    const double vT = unI(top);
    return vT != vT;
}

// Steps 3 and 4 of the merge on one target cell, from the two regrids' float results: each is rounded to its stored type
// (interpolationArray2Data), then the overlay unpacks, chooses and packs: two roundings on the way of every value.  `base` is read
// only where overlay_needs_base(round_to_stored(top)) holds.
template <typename TI, typename TO>
FA_MM_HD TI regrid_overlay_cell_typed(float top, TI fillI, float base, TO fillO, const Unpack<TI>& unI, const Unpack<TO>& unO, const Pack<TI>& pack)
{
    return overlay_cell_typed<TI, TO>(round_to_stored<TI>(top, fillI), round_to_stored<TO>(base, fillO), unI, unO, pack);
}

}  // namespace merge_math
}  // namespace fimex_amd
