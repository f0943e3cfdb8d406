// extern "C" boundary, grid merging of an x/y vector pair: the fused apply, its chain and the host form (merge_vector.hip).
#include "capi_checks.hpp"
#include "host_call.hpp"

#include "../../include/fimex_amd_merge_vector_host.h"

using namespace fimex_amd;

namespace {

struct VectorMergeCall {
    const fimex_amd_merge_plan* plan;
    const fimex_amd_vector_plan *rotOI, *rotST, *rotOT;
    const float *innerU, *innerV, *outerU, *outerV;
    size_t nz;
    float *outU, *outV;
};

struct MergeCells {
    size_t inner, outer, target;  // cells of nz slices
};

// false: nothing to do.  The plans are looked into only after everything that can be refused without them; the buffers are the
// caller's own pointers, host or device
bool check_merge_vector_call(const VectorMergeCall& c, MergeCells& n)
{
    FA_REQUIRE(c.plan != nullptr, "NULL plan");
    FA_REQUIRE(c.rotOI != nullptr && c.rotST != nullptr && c.rotOT != nullptr,
               "NULL vector plan (a pair that no interpolator rotates is merged as two scalar fields)");
    if (c.nz == 0) return false;
    FA_REQUIRE(c.innerU != nullptr && c.innerV != nullptr && c.outerU != nullptr && c.outerV != nullptr && c.outU != nullptr && c.outV != nullptr,
               "NULL data buffer");
    const fimex_amd_regrid_plan &oi = *c.plan->outerToInner, &st = *c.plan->innerToTarget;
    FA_REQUIRE(c.rotOI->ox == oi.outX && c.rotOI->oy == oi.outY, "outerToInnerVec's grid (ox, oy) differs from the inner grid, outerToInner's output grid");
    FA_REQUIRE(c.rotST->ox == st.outX && c.rotST->oy == st.outY, "innerToTargetVec's grid (ox, oy) differs from the target grid, innerToTarget's output grid");
    FA_REQUIRE(c.rotOT->ox == st.outX && c.rotOT->oy == st.outY, "outerToTargetVec's grid (ox, oy) differs from the target grid, outerToTarget's output grid");
    for (const fimex_amd_vector_plan* r : {c.rotOI, c.rotST, c.rotOT})
        FA_REQUIRE(r->device == c.plan->device, "the merge plan and a vector plan live on different devices");
    n = {c.nz * oi.outX * oi.outY, c.nz * oi.inX * oi.inY, c.nz * st.outX * st.outY};
    const size_t f = sizeof(float);
    for (const float* out : {c.outU, c.outV})
        require_no_overlap(out, n.target * f, {{c.innerU, n.inner * f, "the inner field's x component"}, {c.innerV, n.inner * f, "the inner field's y component"},
                                               {c.outerU, n.outer * f, "the outer field's x component"}, {c.outerV, n.outer * f, "the outer field's y component"}});
    require_no_overlap(c.outU, n.target * f, {{c.outV, n.target * f, "the other output buffer"}});
    return true;
}

using Launch = void (*)(const fimex_amd_merge_plan&, const fimex_amd_vector_plan&, const fimex_amd_vector_plan&, const fimex_amd_vector_plan&, const float*,
                        const float*, const float*, const float*, size_t, float*, float*, hipStream_t);

int merge_vector_device(const VectorMergeCall& c, void* stream, Launch launch)
{
    return c_guard([&] {
        MergeCells n{};
        if (!check_merge_vector_call(c, n)) return;
        require_current_device(c.plan->device);
        launch(*c.plan, *c.rotOI, *c.rotST, *c.rotOT, c.innerU, c.innerV, c.outerU, c.outerV, c.nz, c.outU, c.outV, as_stream(stream));
    });
}

}  // namespace

extern "C" {

// the fused kernels' median was below the chain's on the workload of scripts/bench_merge_vector.py, so this
// entry always takes them
int fimex_amd_merge_apply_vector_device(const fimex_amd_merge_plan* plan, const fimex_amd_vector_plan* outerToInnerVec,
                                        const fimex_amd_vector_plan* innerToTargetVec, const fimex_amd_vector_plan* outerToTargetVec,
                                        const float* d_innerU, const float* d_innerV, const float* d_outerU, const float* d_outerV, size_t nz,
                                        float* d_outU, float* d_outV, void* stream)
{
    return merge_vector_device({plan, outerToInnerVec, innerToTargetVec, outerToTargetVec, d_innerU, d_innerV, d_outerU, d_outerV, nz, d_outU, d_outV},
                               stream, launch_merge_vector_fused);
}

int fimex_amd_merge_apply_vector_chain_device(const fimex_amd_merge_plan* plan, const fimex_amd_vector_plan* outerToInnerVec,
                                              const fimex_amd_vector_plan* innerToTargetVec, const fimex_amd_vector_plan* outerToTargetVec,
                                              const float* d_innerU, const float* d_innerV, const float* d_outerU, const float* d_outerV,
                                              size_t nz, float* d_outU, float* d_outV, void* stream)
{
    return merge_vector_device({plan, outerToInnerVec, innerToTargetVec, outerToTargetVec, d_innerU, d_innerV, d_outerU, d_outerV, nz, d_outU, d_outV},
                               stream, launch_merge_vector_chain);
}

// the host form switches to the plan's device, the device forms demand it
int fimex_amd_merge_apply_vector_host(const fimex_amd_merge_plan* plan, const fimex_amd_vector_plan* outerToInnerVec,
                                      const fimex_amd_vector_plan* innerToTargetVec, const fimex_amd_vector_plan* outerToTargetVec,
                                      const float* innerU, const float* innerV, const float* outerU, const float* outerV, size_t nz, float* outU,
                                      float* outV)
{
    return c_guard([&] {
        MergeCells n{};
        if (!check_merge_vector_call({plan, outerToInnerVec, innerToTargetVec, outerToTargetVec, innerU, innerV, outerU, outerV, nz, outU, outV}, n)) return;
        ScopedDevice dev(plan->device);
        HostCall hc;
        const float *dIu = hc.in(innerU, n.inner), *dIv = hc.in(innerV, n.inner), *dOu = hc.in(outerU, n.outer), *dOv = hc.in(outerV, n.outer);
        launch_merge_vector_fused(*plan, *outerToInnerVec, *innerToTargetVec, *outerToTargetVec, dIu, dIv, dOu, dOv, nz, hc.out(outU, n.target),
                                  hc.out(outV, n.target), hc.stream());
        hc.finish();
    });
}

}  // extern "C"
