// fimex_amd/csrc/backward_dispatch.hpp for the CPU tests (tests/test_backward_dispatch.py, through tests/backward_dispatch_host.py):
// every function of the rule over the cross product of a table of switch settings, a table of plans and a table of calls, one
// call per table.  Rows are int64 columns; answers are written as out[switch][plan][call][...] bytes.
#include "backward_dispatch.hpp"

using namespace fimex_amd;
using namespace fimex_amd::dispatch;

namespace {

constexpr int kSwitchCols = 8, kPlanCols = 9, kCallCols = 6;

// STAGED, STAGED_NEAREST, STAGED2, TYPED_FUSED, TYPED_STAGED, TYPED_STAGED2, VECTOR_FUSED, STAGED_MIN_NZ
Switches switches_of(const int64_t* r)
{
    return {(int)r[0], (int)r[1], (int)r[2], (int)r[3], (int)r[4], (int)r[5], (int)r[6], (uint64_t)r[7]};
}

// kind (0 nearest, 1 bilinear, 2 bicubic), funcType, bicubicFast, first form valid, second form valid, inX, inY, outX, outY
PlanFacts plan_of(const int64_t* r)
{
    return {(PlanKind)r[0], (int)r[1], r[2] != 0, r[3] != 0, r[4] != 0, (uint64_t)r[5], (uint64_t)r[6], (uint64_t)r[7], (uint64_t)r[8]};
}

// nz, cdmType, cdmType2, aligned; then for bd_tune: the plan has a second workgroup shape, the batch has the chunks of the second order
CallFacts call_of(const int64_t* r) { return {(uint64_t)r[0], (int)r[1], (int)r[2], r[3] != 0}; }

template <class F>
void cross(const int64_t* sw, uint64_t nSw, const int64_t* plans, uint64_t nPlans, const int64_t* calls, uint64_t nCalls, int width, int8_t* out, F&& f)
{
    for (uint64_t s = 0; s < nSw; ++s) {
        const Switches S = switches_of(sw + s * kSwitchCols);
        for (uint64_t p = 0; p < nPlans; ++p) {
            const PlanFacts P = plan_of(plans + p * kPlanCols);
            for (uint64_t c = 0; c < nCalls; ++c, out += width) f(S, P, calls + c * kCallCols, out);
        }
    }
}

}  // namespace

extern "C" {

int bd_columns(int table) { return table == 0 ? kSwitchCols : (table == 1 ? kPlanCols : kCallCols); }

// out[switch][plan][2]: builds_first, builds_second (the plans' "first form valid" is the outcome of the first build)
void bd_plan_build(const int64_t* sw, uint64_t nSw, const int64_t* plans, uint64_t nPlans, int8_t* out)
{
    const int64_t none[kCallCols] = {};
    cross(sw, nSw, plans, nPlans, none, 1, 2, out, [](const Switches& S, const PlanFacts& P, const int64_t*, int8_t* o) {
        o[0] = builds_first(S, P);
        o[1] = builds_second(S, P);
    });
}

// out[switch][plan][call][4]: float_apply, tune_has_choice (second order as fimex_amd_regrid_plan_tune_device states it),
// float_list, vector_fused
void bd_float(const int64_t* sw, uint64_t nSw, const int64_t* plans, uint64_t nPlans, const int64_t* calls, uint64_t nCalls, int8_t* out)
{
    cross(sw, nSw, plans, nPlans, calls, nCalls, 4, out, [](const Switches& S, const PlanFacts& P, const int64_t* c, int8_t* o) {
        const uint64_t nz = (uint64_t)c[0];
        o[0] = (int8_t)float_apply(S, P, nz);
        o[1] = tune_has_choice(S, P, nz, c[4] != 0, float_apply(S, P, nz) == FloatApply::Second && c[5] != 0);
        o[2] = float_list(S, P, nz);
        o[3] = vector_fused(S, P, nz);
    });
}

// out[switch][plan][call][6]: the four slots of typed_apply's candidates (-1: beyond the list), typed_list, vector_typed_fused
void bd_typed(const int64_t* sw, uint64_t nSw, const int64_t* plans, uint64_t nPlans, const int64_t* calls, uint64_t nCalls, int8_t* out)
{
    cross(sw, nSw, plans, nPlans, calls, nCalls, 6, out, [](const Switches& S, const PlanFacts& P, const int64_t* c, int8_t* o) {
        const CallFacts C = call_of(c);
        CallFacts one = C;  // a variable or a list has one type
        one.cdmType2 = one.cdmType;
        const TypedCandidates t = typed_apply(S, P, one);
        for (int i = 0; i < 4; ++i) o[i] = i < t.n ? (int8_t)t.c[i] : (int8_t)-1;
        o[4] = typed_list(S, P, one);
        o[5] = vector_typed_fused(S, P, C);
    });
}

}  // extern "C"
