// extern "C" boundary, vertical interpolation plans (8f n5b): create, destroy, info, the apply on stored types and the entries read
// back for diagnostics (vertical_plan.hip).  The create pair and the apply pair are one template each over the call type
// (host_call.hpp).  Everything that can be refused without a device is refused before one is touched.
#include "capi_checks.hpp"
#include "host_call.hpp"
#include "vertical_plan.hpp"

#include "../../include/fimex_amd_vertical_plan_host.h"

#include <memory>
#include <vector>

using namespace fimex_amd;

namespace {

constexpr size_t kMaxInputLevels = 65535;  // an entry holds a level index in 16 bits

template <class Call>
void plan_create(Call&& c, int method, size_t nx, size_t ny, size_t nt, const fimex_amd_vertical_levels* inLevels,
                 const fimex_amd_vertical_levels* outLevels, const double* level1, size_t nzo, const double* validMin, const double* validMax,
                 fimex_amd_vertical_plan** plan)
{
    FA_REQUIRE(plan != nullptr, "NULL argument");
    *plan = nullptr;
    (void)check_vertical_search(method, nx, ny, nt, inLevels, outLevels, level1, nzo, false);  // differs: asks on an empty grid too
    FA_REQUIRE(inLevels->nz <= kMaxInputLevels, "a plan holds level indices in 16 bits: at most 65535 input levels (nzi > 65535)");
    FA_REQUIRE(nt <= 65535, "at most 65535 unlimited-dimension positions per plan");
    size_t plane = 0, cells = 0, entries = 0, bytes = 0;
    FA_REQUIRE(!__builtin_mul_overflow(nx, ny, &plane) && !__builtin_mul_overflow(plane, nt, &cells) && !__builtin_mul_overflow(cells, nzo, &entries) &&
                   !__builtin_mul_overflow(entries, sizeof(uint32_t) + sizeof(float), &bytes),
               "the plan holds more entries than size_t counts");
    const int device = current_device_checked();  // before the plan and its event exist
    auto p = std::make_unique<fimex_amd_vertical_plan>();
    p->device = device;
    p->info.nx = nx;
    p->info.ny = ny;
    p->info.nt = nt;
    p->info.nzi = inLevels->nz;
    p->info.nzo = nzo;
    p->info.method = method;
    p->info.entryBytes = bytes;
    p->pair.allocate(entries);
    p->factor.allocate(entries);
    const fimex_amd_vertical_levels li = levels_on(c, *inLevels, plane, nt);
    fimex_amd_vertical_levels lo{};
    if (outLevels) lo = levels_on(c, *outLevels, plane, nt);
    build_vertical_plan(*p, li, outLevels ? &lo : nullptr, level1, c.in(validMin, plane), c.in(validMax, plane), c.stream());
    c.finish();
    *plan = p.release();
}

template <class Call>
void plan_apply(Call&& c, PlanDevice& dev, const fimex_amd_vertical_plan* plan, size_t nvar, const void* const* in, int cdmType,
                const double* badValue, const float* clampMin, const float* clampMax, void* const* out)
{
    FA_REQUIRE(plan != nullptr, "NULL vertical plan");
    const size_t elem = cdm_type_size(cdmType);  // throws for NAT and STRING
    FA_REQUIRE(nvar >= 1, "no variables (nvar == 0)");
    FA_REQUIRE(in != nullptr && out != nullptr && badValue != nullptr && clampMin != nullptr && clampMax != nullptr, "NULL argument");
    const size_t cells = plan->info.nx * plan->info.ny * plan->info.nt;
    if (cells == 0) return;
    size_t inBytes = 0;
    FA_REQUIRE(!__builtin_mul_overflow(cells * plan->info.nzi, elem, &inBytes), "a variable holds more bytes than size_t counts");
    const size_t outBytes = cells * plan->info.nzo * elem;
    for (size_t i = 0; i < nvar; ++i) {
        const std::string which = "variable " + std::to_string(i);
        FA_REQUIRE(in[i] != nullptr && out[i] != nullptr, "NULL data buffer of " + which);
        FA_REQUIRE(reinterpret_cast<uintptr_t>(in[i]) % elem == 0 && reinterpret_cast<uintptr_t>(out[i]) % elem == 0,
                   "a data buffer of " + which + " is not aligned to its element size of " + std::to_string(elem) + " bytes");
        for (size_t j = 0; j < nvar; ++j) {
            const std::string other = "the input of variable " + std::to_string(j);
            require_no_overlap(out[i], outBytes, {{in[j], inBytes, other.c_str()}});
            if (j < i) require_no_overlap(out[i], outBytes, {{out[j], outBytes, "another output"}});
        }
        require_no_overlap(out[i], outBytes, {{plan->pair.get(), plan->pair.bytes(), "the plan"}, {plan->factor.get(), plan->factor.bytes(), "the plan"}});
    }
    dev.enter(plan->device);
    std::vector<VerticalPlanVar> vars(nvar);
    for (size_t i = 0; i < nvar; ++i)
        vars[i] = VerticalPlanVar{c.in_bytes(in[i], inBytes), c.out_bytes(out[i], outBytes), badValue[i], clampMin[i], clampMax[i]};
    launch_vertical_plan_apply(*plan, vars.data(), nvar, cdmType, c.stream());
    c.finish();
}

}  // namespace

extern "C" {

int fimex_amd_vertical_plan_create_device(int method, size_t nx, size_t ny, size_t nt, const fimex_amd_vertical_levels* inLevels,
                                          const fimex_amd_vertical_levels* outLevels, const double* level1, size_t nzo, const double* d_validMin,
                                          const double* d_validMax, void* stream, fimex_amd_vertical_plan** plan)
{
    return c_guard([&] {
        plan_create(DeviceCall{as_stream(stream)}, method, nx, ny, nt, inLevels, outLevels, level1, nzo, d_validMin, d_validMax, plan);
    });
}

int fimex_amd_vertical_plan_create_host(int method, size_t nx, size_t ny, size_t nt, const fimex_amd_vertical_levels* inLevels,
                                        const fimex_amd_vertical_levels* outLevels, const double* level1, size_t nzo, const double* validMin,
                                        const double* validMax, fimex_amd_vertical_plan** plan)
{
    return c_guard([&] { plan_create(HostCall(), method, nx, ny, nt, inLevels, outLevels, level1, nzo, validMin, validMax, plan); });
}

int fimex_amd_vertical_plan_destroy(fimex_amd_vertical_plan* plan)
{
    return c_guard([&] { delete plan; });
}

int fimex_amd_vertical_plan_info(const fimex_amd_vertical_plan* plan, fimex_amd_vertical_info* info)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr && info != nullptr, "NULL argument");
        *info = plan->info;
    });
}

int fimex_amd_vertical_plan_apply_device(const fimex_amd_vertical_plan* plan, size_t nvar, const void* const* d_in, int cdmType,
                                         const double* badValue, const float* clampMin, const float* clampMax, void* const* d_out, void* stream)
{
    return c_guard([&] {
        PlanDevice dev{false, {}};
        plan_apply(DeviceCall{as_stream(stream)}, dev, plan, nvar, d_in, cdmType, badValue, clampMin, clampMax, d_out);
    });
}

int fimex_amd_vertical_plan_apply_host(const fimex_amd_vertical_plan* plan, size_t nvar, const void* const* in, int cdmType,
                                       const double* badValue, const float* clampMin, const float* clampMax, void* const* out)
{
    return c_guard([&] {
        PlanDevice dev{true, {}};  // outlives the HostCall: its buffers go while the plan's device is current
        plan_apply(HostCall(), dev, plan, nvar, in, cdmType, badValue, clampMin, clampMax, out);
    });
}

int fimex_amd_vertical_plan_read_host(const fimex_amd_vertical_plan* plan, unsigned* first, unsigned* second, float* factor)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL vertical plan");
        const size_t n = plan->pair.size();
        if (n == 0) return;
        FA_REQUIRE(first != nullptr && second != nullptr && factor != nullptr, "NULL argument");
        ScopedDevice scoped(plan->device);
        FA_HIP(hipEventSynchronize(plan->built.e));
        std::vector<uint32_t> pair(n);
        FA_HIP(hipMemcpy(pair.data(), plan->pair.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        FA_HIP(hipMemcpy(factor, plan->factor.get(), n * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            first[i] = pair[i] & 0xffffu;
            second[i] = pair[i] >> 16;
        }
    });
}

}  // extern "C"
