// extern "C" boundary, regridding a LIST of variables on one plan in one call (fimex_amd_regrid_apply_multi_*): the reference
// calls CDMInterpolator::getDataSlice once per variable and time step (src/CDMInterpolator.cc:251-259), and most variables of a
// weather file are surface fields of one slice, each an allocation of its own.  Where the slices together make a batch of the
// second staged form, they run in one launch of its list kernels (staged2_list.hip, staged2_list_typed.hip); everything else runs
// the per-variable calls in here.  The bytes are the same either way.
#include "host_call.hpp"

#include "slice_list.hpp"

#include <algorithm>
#include <string>
#include <vector>

static_assert(FIMEX_AMD_REGRID_MULTI_MAX_VARS == fimex_amd::kSliceListMaxVars, "the header states what one launch takes");

namespace fimex_amd {
namespace {

// Outputs must not overlap each other or any input (an input may be given more than once): checked on the caller's own
// pointers before anything is copied or launched.  Sorted by start, an array overlaps an earlier one iff it starts before the
// furthest end seen so far.
void require_disjoint_outputs(size_t nvar, const void* const* in, void* const* out, const size_t* nz, size_t inSliceBytes, size_t outSliceBytes)
{
    struct Span {
        uintptr_t begin, end;
        bool output;
    };
    std::vector<Span> spans;
    for (size_t i = 0; i < nvar; ++i) {
        if (nz[i] == 0) continue;
        const uintptr_t a = reinterpret_cast<uintptr_t>(in[i]), b = reinterpret_cast<uintptr_t>(out[i]);
        if (inSliceBytes) spans.push_back(Span{a, a + nz[i] * inSliceBytes, false});
        if (outSliceBytes) spans.push_back(Span{b, b + nz[i] * outSliceBytes, true});
    }
    std::sort(spans.begin(), spans.end(), [](const Span& x, const Span& y) { return x.begin < y.begin; });
    uintptr_t endAny = 0, endOut = 0;
    for (const Span& s : spans) {
        FA_REQUIRE(!(s.output && s.begin < endAny), "an output overlaps another array of the list");
        FA_REQUIRE(!(!s.output && s.begin < endOut), "an input overlaps an output of the list");
        endAny = std::max(endAny, s.end);
        if (s.output) endOut = std::max(endOut, s.end);
    }
}

// both entries on both kinds of buffers; typed == false: float slices, cdmType and badValue are not looked at
template <class Call>
void regrid_multi(Call&& c, bool switchDevice, const fimex_amd_regrid_plan* plan, size_t nvar, const void* const* in, bool typed, int cdmType,
                  const size_t* nz, const double* badValue, void* const* out, int* path)
{
    if (path) *path = 0;
    FA_REQUIRE(plan != nullptr, "NULL plan");
    const size_t elem = typed ? cdm_type_size(cdmType) : sizeof(float);
    if (nvar == 0) return;
    FA_REQUIRE(in != nullptr && nz != nullptr && out != nullptr && (!typed || badValue != nullptr), "NULL argument");
    bool any = false;
    for (size_t i = 0; i < nvar; ++i) {
        if (nz[i] == 0) continue;
        any = true;
        FA_REQUIRE(in[i] != nullptr && out[i] != nullptr, "NULL buffer of variable " + std::to_string(i));
    }
    if (!any) return;  // (nothing of the plan has been looked at: no device is needed up to here)
    const size_t inLayer = plan->inX * plan->inY, outLayer = plan->outX * plan->outY;
    require_disjoint_outputs(nvar, in, out, nz, inLayer * elem, outLayer * elem);
    PlanDevice dev{switchDevice, {}};
    dev.enter(plan->device);
    std::vector<const void*> dIn(nvar, nullptr);
    std::vector<void*> dOut(nvar, nullptr);
    for (size_t i = 0; i < nvar; ++i) {
        if (nz[i] == 0) continue;
        dIn[i] = c.in_bytes(in[i], nz[i] * inLayer * elem);
        dOut[i] = c.out_bytes(out[i], nz[i] * outLayer * elem);
    }
    // (the launchers copy what they need of the caller's tables into the kernels' arguments: nothing reads them after the return)
    hipStream_t st = c.stream();
    bool list;
    if (typed) {
        list = launch_typed_apply_list(*plan, nvar, dIn.data(), cdmType, nz, badValue, dOut.data(), st);
    } else {
        list = launch_backward_apply_list(*plan, nvar, reinterpret_cast<const float* const*>(dIn.data()), nz, reinterpret_cast<float* const*>(dOut.data()), st);
    }
    if (!list) {
        for (size_t i = 0; i < nvar; ++i) {
            if (nz[i] == 0) continue;
            if (typed) apply_plan_typed_device(*plan, dIn[i], cdmType, nz[i], badValue[i], dOut[i], st);
            else apply_plan_device(*plan, static_cast<const float*>(dIn[i]), nz[i], static_cast<float*>(dOut[i]), st);
        }
    }
    if (path) *path = list ? 1 : 0;
    c.finish();
}

}  // namespace
}  // namespace fimex_amd

using namespace fimex_amd;

extern "C" {

int fimex_amd_regrid_apply_multi_device(const fimex_amd_regrid_plan* plan, size_t nvar, const float* const* d_in, const size_t* nz,
                                        float* const* d_out, void* stream, int* path)
{
    return c_guard([&] {
        regrid_multi(DeviceCall{as_stream(stream)}, false, plan, nvar, reinterpret_cast<const void* const*>(d_in), false, FIMEX_AMD_CDM_FLOAT, nz,
                     nullptr, reinterpret_cast<void* const*>(d_out), path);
    });
}

int fimex_amd_regrid_apply_multi_typed_device(const fimex_amd_regrid_plan* plan, size_t nvar, const void* const* d_in, int cdmType,
                                              const size_t* nz, const double* badValue, void* const* d_out, void* stream, int* path)
{
    return c_guard([&] { regrid_multi(DeviceCall{as_stream(stream)}, true, plan, nvar, d_in, true, cdmType, nz, badValue, d_out, path); });
}

int fimex_amd_regrid_apply_multi_host(const fimex_amd_regrid_plan* plan, size_t nvar, const float* const* in, const size_t* nz,
                                      float* const* out, int* path)
{
    return c_guard([&] {
        regrid_multi(HostCall(), true, plan, nvar, reinterpret_cast<const void* const*>(in), false, FIMEX_AMD_CDM_FLOAT, nz, nullptr,
                     reinterpret_cast<void* const*>(out), path);
    });
}

int fimex_amd_regrid_apply_multi_typed_host(const fimex_amd_regrid_plan* plan, size_t nvar, const void* const* in, int cdmType,
                                            const size_t* nz, const double* badValue, void* const* out, int* path)
{
    return c_guard([&] { regrid_multi(HostCall(), true, plan, nvar, in, true, cdmType, nz, badValue, out, path); });
}

}  // extern "C"
