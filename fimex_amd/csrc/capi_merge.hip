// extern "C" boundary, grid merging: border smoothing, overlay, the merge plan and its applies (merge.hip).
#include "capi_checks.hpp"
#include "host_call.hpp"

#include <memory>

using namespace fimex_amd;

namespace {

// false: nothing to do
bool check_smooth_call(const float* inner, const float* outer, const float* out, size_t nx, size_t ny, size_t nz, size_t transitionWidth)
{
    // CDMBorderSmoothing_LinearFactory throws "invalid parameter values for linear smoothing"
    FA_REQUIRE(transitionWidth > 0, "invalid parameter values for linear smoothing (transitionWidth == 0)");
    FA_REQUIRE(nx > 0 && ny > 0, "empty grid (nx == 0 or ny == 0)");
    if (nz == 0) return false;
    FA_REQUIRE(inner != nullptr && outer != nullptr && out != nullptr, "NULL data buffer");
    const size_t n = nx * ny * nz;
    require_same_or_apart(out, inner, n, "the inner field (other than in place)");
    require_same_or_apart(out, outer, n, "the outer field (other than in place)");
    return true;
}

bool check_overlay_call(const float* top, const float* base, const float* out, size_t n)
{
    if (n == 0) return false;
    FA_REQUIRE(top != nullptr && base != nullptr && out != nullptr, "NULL data buffer");
    require_same_or_apart(out, top, n, "the top field (other than in place)");
    require_same_or_apart(out, base, n, "the base field (other than in place)");
    return true;
}

struct MergeSizes {
    size_t inner, outer, target;  // cells of a slice
};

MergeSizes merge_sizes(const fimex_amd_merge_plan& m)
{
    return {m.outerToInner->outX * m.outerToInner->outY, m.outerToInner->inX * m.outerToInner->inY,
            m.innerToTarget->outX * m.innerToTarget->outY};
}

// false: nothing to do
bool check_merge_call(const fimex_amd_merge_plan* plan, const float* inner, const float* outer, size_t nz, const float* out)
{
    FA_REQUIRE(plan != nullptr, "NULL plan");
    if (nz == 0) return false;
    FA_REQUIRE(inner != nullptr && outer != nullptr && out != nullptr, "NULL data buffer");
    const MergeSizes s = merge_sizes(*plan);
    require_no_overlap(out, nz * s.target * sizeof(float), {{inner, nz * s.inner * sizeof(float), "the inner field"},
                                                            {outer, nz * s.outer * sizeof(float), "the outer field"}});
    return true;
}

// host form: the copy of the outer field is smoothed in place, as the reference does, and lands in out
template <class Call>
void border_smooth(Call&& c, const float* inner, const float* outerOnInner, float* out, size_t nx, size_t ny, size_t nz,
                   size_t transitionWidth, size_t borderWidth, int useOuterIfInnerUndefined)
{
    if (!check_smooth_call(inner, outerOnInner, out, nx, ny, nz, transitionWidth)) return;
    (void)current_device_checked();
    const size_t n = nx * ny * nz;
    const Through<float> outer = c.through(outerOnInner, out, n);
    launch_border_smooth(c.in(inner, n), outer.in, outer.out, nx, ny, nz, transitionWidth, borderWidth, useOuterIfInnerUndefined != 0, c.stream());
    c.finish();
}

template <class Call>
void overlay(Call&& c, const float* top, const float* base, float* out, size_t n)
{
    if (!check_overlay_call(top, base, out, n)) return;
    (void)current_device_checked();
    const Through<float> b = c.through(base, out, n);
    launch_overlay(c.in(top, n), b.in, b.out, n, c.stream());
    c.finish();
}

}  // namespace

extern "C" {

int fimex_amd_border_smooth_device(const float* d_inner, const float* d_outerOnInner, float* d_out, size_t nx, size_t ny, size_t nz,
                                   size_t transitionWidth, size_t borderWidth, int useOuterIfInnerUndefined, void* stream)
{
    return c_guard([&] {
        border_smooth(DeviceCall{as_stream(stream)}, d_inner, d_outerOnInner, d_out, nx, ny, nz, transitionWidth, borderWidth,
                      useOuterIfInnerUndefined);
    });
}

int fimex_amd_border_smooth_host(const float* inner, const float* outerOnInner, float* out, size_t nx, size_t ny, size_t nz,
                                 size_t transitionWidth, size_t borderWidth, int useOuterIfInnerUndefined)
{
    return c_guard([&] { border_smooth(HostCall(), inner, outerOnInner, out, nx, ny, nz, transitionWidth, borderWidth, useOuterIfInnerUndefined); });
}

int fimex_amd_overlay_device(const float* d_top, const float* d_base, float* d_out, size_t n, void* stream)
{
    return c_guard([&] { overlay(DeviceCall{as_stream(stream)}, d_top, d_base, d_out, n); });
}

int fimex_amd_overlay_host(const float* top, const float* base, float* out, size_t n)
{
    return c_guard([&] { overlay(HostCall(), top, base, out, n); });
}

int fimex_amd_merge_plan_create(const fimex_amd_regrid_plan* outerToInner, const fimex_amd_regrid_plan* innerToTarget,
                                const fimex_amd_regrid_plan* outerToTarget, size_t transitionWidth, size_t borderWidth,
                                int useOuterIfInnerUndefined, fimex_amd_merge_plan** plan)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL argument");
        *plan = nullptr;
        FA_REQUIRE(outerToInner != nullptr && innerToTarget != nullptr && outerToTarget != nullptr, "NULL regrid plan");
        FA_REQUIRE(transitionWidth > 0, "invalid parameter values for linear smoothing (transitionWidth == 0)");
        for (const fimex_amd_regrid_plan* p : {outerToInner, innerToTarget, outerToTarget})
            FA_REQUIRE(p->kind != PlanKind::Forward, "a merge needs backward plans (nearest, bilinear or bicubic)");
        FA_REQUIRE(outerToInner->device == innerToTarget->device && outerToInner->device == outerToTarget->device,
                   "the three regrid plans live on different devices");
        FA_REQUIRE(outerToInner->inX == outerToTarget->inX && outerToInner->inY == outerToTarget->inY,
                   "the plans do not chain: outerToInner and outerToTarget read different outer grids");
        FA_REQUIRE(outerToInner->outX == innerToTarget->inX && outerToInner->outY == innerToTarget->inY,
                   "the plans do not chain: outerToInner writes another grid than innerToTarget reads");
        FA_REQUIRE(innerToTarget->outX == outerToTarget->outX && innerToTarget->outY == outerToTarget->outY,
                   "the plans do not chain: innerToTarget and outerToTarget write different target grids");
        auto m = std::make_unique<fimex_amd_merge_plan>();
        m->device = outerToInner->device;
        m->outerToInner = outerToInner;
        m->innerToTarget = innerToTarget;
        m->outerToTarget = outerToTarget;
        m->transitionWidth = transitionWidth;
        m->borderWidth = borderWidth;
        m->useOuter = useOuterIfInnerUndefined != 0;
        *plan = m.release();
    });
}

int fimex_amd_merge_plan_destroy(fimex_amd_merge_plan* plan)
{
    return c_guard([&] { delete plan; });
}

int fimex_amd_merge_apply_device(const fimex_amd_merge_plan* plan, const float* d_inner, const float* d_outer, size_t nz, float* d_out, void* stream)
{
    return c_guard([&] {
        if (!check_merge_call(plan, d_inner, d_outer, nz, d_out)) return;
        require_current_device(plan->device);
        launch_merge_fused(*plan, d_inner, d_outer, nz, d_out, as_stream(stream));
    });
}

int fimex_amd_merge_apply_chain_device(const fimex_amd_merge_plan* plan, const float* d_inner, const float* d_outer, size_t nz, float* d_out,
                                       void* stream)
{
    return c_guard([&] {
        if (!check_merge_call(plan, d_inner, d_outer, nz, d_out)) return;
        require_current_device(plan->device);
        launch_merge_chain(*plan, d_inner, d_outer, nz, d_out, as_stream(stream));
    });
}

// not one template with merge_apply_device: the host form switches to the plan's device, the device form demands it
int fimex_amd_merge_apply_host(const fimex_amd_merge_plan* plan, const float* inner, const float* outer, size_t nz, float* out)
{
    return c_guard([&] {
        if (!check_merge_call(plan, inner, outer, nz, out)) return;
        ScopedDevice dev(plan->device);
        HostCall hc;
        const MergeSizes s = merge_sizes(*plan);
        launch_merge_fused(*plan, hc.in(inner, nz * s.inner), hc.in(outer, nz * s.outer), nz, hc.out(out, nz * s.target), hc.stream());
        hc.finish();
    });
}

}  // extern "C"
