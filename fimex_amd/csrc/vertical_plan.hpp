// A vertical interpolation plan as it lives in HBM (vertical_plan.hip builds and applies it, capi_vertical_plan.hip is its C boundary).
//
// CDMVerticalInterpolator::getLevelDataSlice searches the pair of input levels around every target level again for every variable,
// although the search depends on the levels, the validity range and the method only.  Here it runs once; per output cell
// (t, k, column) the plan keeps two planes [nt][nzo][ny][nx], 8 bytes per cell:
//   pair    u32  first | second << 16: pos.first / pos.second of src/CDMVerticalInterpolator.cc:476; first == second: the cell is
//                undefined (outside the validity range, no second distinct level, a failed guard of a log method, a factor outside
//                the range of the two bounded linear methods)
//   factor  f32  the f of the blend with the method folded in (vertical_plan.hip, entry_factor), so that the apply has one rule for
//                all seven methods: f == 0 ? A : f == 1 ? B : A + f * (B - A)
#pragma once

#include "plan.hpp"

struct fimex_amd_vertical_plan {
    int device = 0;
    fimex_amd_vertical_info info{};
    fimex_amd::DeviceArray<uint32_t> pair;
    fimex_amd::DeviceArray<float> factor;
    fimex_amd::ScopedEvent built;  // recorded behind the build: what reads the entries from the host waits for it
};

namespace fimex_amd {

// one variable of an apply: device pointers in the stored type, [nt][nzi][plane] in and [nt][nzo][plane] out
struct VerticalPlanVar {
    const void* in;
    void* out;
    double badValue;
    float clampMin, clampMax;
};

// every argument has been checked; plan.info is filled in and the two planes are allocated
void build_vertical_plan(fimex_amd_vertical_plan& plan, const fimex_amd_vertical_levels& inLevels, const fimex_amd_vertical_levels* outLevels,
                         const double* h_level1, const double* d_validMin, const double* d_validMax, hipStream_t stream);
void launch_vertical_plan_apply(const fimex_amd_vertical_plan& plan, const VerticalPlanVar* vars, size_t nvar, int cdmType, hipStream_t stream);

}  // namespace fimex_amd
