// What the stored-type kernels of the second LDS-staged regrid form share beside their text (staged2_apply_typed_kernel.hpp):
// staged2_typed.hip (slices of one array) and staged2_list_typed.hip (slices of a list of variables).  A lane owns two PAIRS of neighbouring outputs (cells
// 2 * t, 2 * t + 1 of the tile, and the same NT * 2 cells further on), so that two results leave in one 4-byte (2-byte elements)
// or 2-byte store and a wave still writes 256 (128) contiguous bytes; the two source elements of a stencil row arrive in one
// ds_read2_b32 and are shifted apart; elements become float / NaN as Data::asFloat + mifi_bad2nanf do, results go back through
// ScaleValue's rounding (typed_convert.hpp); the element reads and the stores are staged2_lane_ops.hpp's.
#pragma once

#include "staged2_lane_ops.hpp"
#include "staged2_ring.hpp"

namespace fimex_amd {
namespace {

struct TypedEdge {
    float bad;          // the variable's fill value narrowed to float (mifi_bad2nanf's argument)
    uint32_t hasBad;
    double fillOut;     // NaN -> this (interpolationArray2Data)
    uint32_t pairStore; // outX even: the two results of a pair share one store
};

// list form: TypedEdge's bad and fillOut of every variable of the launch (hasBad follows from bad, pairStore holds for the launch)
struct TypedListEdge {
    float bad[kSliceListMaxVars];
    double fillOut[kSliceListMaxVars];
};

}  // namespace
}  // namespace fimex_amd
