// The per-cell arithmetic of grid merging on an x/y vector pair, stated once for host and device: the rotation of
// mifi_vector_reproject_values_by_matrix_f (src/interpolation.c:796-810) that every CDMInterpolator of the merger applies behind
// its regrid (src/CDMInterpolator.cc:259-283), and the two per-cell steps of CDMMerger on a pair -- CDMBorderSmoothing::getDataSlice
// and CDMOverlay::getDataSlice component by component, on pairs that were rotated together.  merge_vector.hip compiles it for the
// device; tests/merge_vector_math_host.cc compiles it with a plain C++ compiler, so it includes nothing of HIP and uses no device
// builtin.  Compile with -ffp-contract=off: the products of the rotation and the add or subtract are separate operations.
#pragma once

#include "merge_math.hpp"

namespace fimex_amd {
namespace merge_math {

struct Pair {
    float u, v;
};

// interpolation.c:804-805 on one cell: float -> double products, one double subtract / add, each narrowed to float once.  A NaN
// in u, v, m0 or m1 makes both components NaN.
FA_MM_HD Pair rotate_pair_values(float u, float v, double m0, double m1)
{
    const double un = (double)u * m0 - (double)v * m1;  // :804
    const double vn = (double)u * m1 + (double)v * m0;  // :805
    return Pair{(float)un, (float)vn};
}

// true: smooth_pair calls rotatedOuter for these inner values
FA_MM_HD bool pair_needs_outer(const SmoothClass& c, float innerU, float innerV, bool useOuter)
{
    return needs_outer<float>(c, innerU, useOuter) || needs_outer<float>(c, innerV, useOuter);
}

// Steps 1 and 2 on one inner cell: rotatedOuter() yields the outer pair regridded to this cell and rotated by R_oi; it is called
// once, and only where one of the components reads the outer.  Each component is then smoothed on its own.
template <class RotatedOuter>
FA_MM_HD Pair smooth_pair(const SmoothClass& c, float innerU, float innerV, RotatedOuter&& rotatedOuter, bool useOuter)
{
    Pair o{0.f, 0.f};
    if (pair_needs_outer(c, innerU, innerV, useOuter)) o = rotatedOuter();
    return Pair{smooth_value<float>(c, innerU, o.u, useOuter), smooth_value<float>(c, innerV, o.v, useOuter)};
}

// true: overlay_pair calls rotatedBase for this top pair
FA_MM_HD bool pair_needs_base(const Pair& top) { return top.u != top.u || top.v != top.v; }

// Step 4 on one target cell: top is the smoothed pair regridded and rotated by R_st; rotatedBase() yields the outer pair
// regridded and rotated by R_ot, and is called once, only where a component of top is undefined.  The choice is per component.
template <class RotatedBase>
FA_MM_HD Pair overlay_pair(const Pair& top, RotatedBase&& rotatedBase)
{
    if (!pair_needs_base(top)) return top;
    const Pair b = rotatedBase();
    return Pair{top.u != top.u ? b.u : top.u, top.v != top.v ? b.v : top.v};
}

}  // namespace merge_math
}  // namespace fimex_amd
