// The per-cell arithmetic of grid merging on an x/y vector pair in its stored types, stated once for host and
// device: the two per-cell steps of CDMMerger on a pair whose four fields -- inner u, inner v, outer u, outer v -- are packed, each
// with its own packing.  The regridded pairs arrive as floats, rotated on the raw counts (merge_vector_math.hpp's
// rotate_pair_values behind data2InterpolationArray and the regrid); each component is rounded to its stored type as
// interpolationArray2Data leaves it (merge_math.hpp's round_to_stored), then smoothed or overlaid as a scalar of 6.15 is
// (smooth_cell_typed, overlay_cell_typed).  merge_vector_typed.hip compiles it for the device;
// tests/merge_vector_typed_math_host.cc compiles it with a plain C++ compiler, so it includes nothing of HIP and uses no device
// builtin.  Compile with -ffp-contract=off.
#pragma once

#include "merge_vector_math.hpp"

namespace fimex_amd {
namespace merge_math {

template <typename T>
struct StoredPair {
    T u, v;
};

// one component of the pair: the inner field's and the outer field's unpacking, and the inner field's packing for the result
template <typename T>
struct ComponentOps {
    Unpack<T> unI;
    Unpack<T> unO;
    Pack<T> pack;
};

template <typename T>
inline ComponentOps<T> make_component_ops(double fillI, double scaleI, double offsetI, double fillO, double scaleO, double offsetO)
{
    return {make_unpack<T>(fillI, scaleI, offsetI), make_unpack<T>(fillO, scaleO, offsetO), make_pack<T>(fillI, scaleI, offsetI)};
}

// true: smooth_pair_typed calls rotatedOuter for these inner counts
template <typename T>
FA_MM_HD bool pair_needs_outer_typed(const SmoothClass& c, T innerU, T innerV, const ComponentOps<T>& opsU, const ComponentOps<T>& opsV, bool useOuter)
{
    return needs_outer<double>(c, opsU.unI(innerU), useOuter) || needs_outer<double>(c, opsV.unI(innerV), useOuter);
}

// Steps 1 and 2 on one inner cell: rotatedOuter() yields the outer pair's counts regridded to this cell and rotated by R_oi, as
// floats; it is called once, and only where one of the components reads the outer.  Each rotated component becomes a count of the
// outer component's type with that component's fill value (fillOu, fillOv), and each component is then smoothed on its own.
template <typename T, class RotatedOuter>
FA_MM_HD StoredPair<T> smooth_pair_typed(const SmoothClass& c, T innerU, T innerV, RotatedOuter&& rotatedOuter, T fillOu, T fillOv,
                                         const ComponentOps<T>& opsU, const ComponentOps<T>& opsV, bool useOuter)
{
    Pair o{0.f, 0.f};
    if (pair_needs_outer_typed<T>(c, innerU, innerV, opsU, opsV, useOuter)) o = rotatedOuter();
    return StoredPair<T>{smooth_cell_typed<T, T>(c, innerU, round_to_stored<T>(o.u, fillOu), opsU.unI, opsU.unO, opsU.pack, useOuter),
                         smooth_cell_typed<T, T>(c, innerV, round_to_stored<T>(o.v, fillOv), opsV.unI, opsV.unO, opsV.pack, useOuter)};
}

// Steps 3 and 4 on one target cell: top is the smoothed pair's counts regridded and rotated by R_st, as floats; each component
// is rounded to the inner component's type with its fill value (fillIu, fillIv).  rotatedBase() yields the outer pair regridded
// and rotated by R_ot, and is called once, only where a rounded component of top is its fill value.  The choice is per component;
// a defined top value is unpacked and packed again.
template <typename T, class RotatedBase>
FA_MM_HD StoredPair<T> regrid_overlay_pair_typed(const Pair& top, T fillIu, T fillIv, RotatedBase&& rotatedBase, T fillOu, T fillOv,
                                                 const ComponentOps<T>& opsU, const ComponentOps<T>& opsV)
{
    const T tu = round_to_stored<T>(top.u, fillIu), tv = round_to_stored<T>(top.v, fillIv);
    Pair b{0.f, 0.f};
    if (overlay_needs_base<T>(tu, opsU.unI) || overlay_needs_base<T>(tv, opsV.unI)) b = rotatedBase();
    return StoredPair<T>{overlay_cell_typed<T, T>(tu, round_to_stored<T>(b.u, fillOu), opsU.unI, opsU.unO, opsU.pack),
                         overlay_cell_typed<T, T>(tv, round_to_stored<T>(b.v, fillOv), opsV.unI, opsV.unO, opsV.pack)};
}

}  // namespace merge_math
}  // namespace fimex_amd
