// extern "C" boundary, grid merging of an x/y vector pair in its stored types: the apply with its dispatch, its chain and the host
// form (merge_vector_typed.hip).
#include "capi_checks.hpp"
#include "host_call.hpp"

#include "../../include/fimex_amd_merge_vector_typed_host.h"

using namespace fimex_amd;

namespace {

struct VectorTypedMergeCall {
    const fimex_amd_merge_plan* plan;
    const fimex_amd_vector_plan *rotOI, *rotST, *rotOT;
    const void* innerU;
    const fimex_amd_packing* pIu;
    const void* innerV;
    const fimex_amd_packing* pIv;
    const void* outerU;
    const fimex_amd_packing* pOu;
    const void* outerV;
    const fimex_amd_packing* pOv;
    size_t nz;
    void *outU, *outV;
};

struct MergeBytes {
    size_t innerU, innerV, outerU, outerV, targetU, targetV;  // bytes of nz slices, each in its own element size
};

// false: nothing to do.  The plans are looked into only after everything that can be refused without them; the buffers are the
// caller's own pointers, host or device
bool check_merge_vector_typed_call(const VectorTypedMergeCall& c, MergeBytes& b)
{
    FA_REQUIRE(c.plan != nullptr, "NULL plan");
    FA_REQUIRE(c.rotOI != nullptr && c.rotST != nullptr && c.rotOT != nullptr,
               "NULL vector plan (a pair that no interpolator rotates is merged as two scalar fields)");
    FA_REQUIRE(c.pIu != nullptr && c.pIv != nullptr && c.pOu != nullptr && c.pOv != nullptr, "NULL packing");
    const size_t sIu = cdm_type_size(c.pIu->type), sIv = cdm_type_size(c.pIv->type);  // throws for NAT and STRING
    const size_t sOu = cdm_type_size(c.pOu->type), sOv = cdm_type_size(c.pOv->type);
    for (const fimex_amd_packing* p : {c.pIu, c.pIv})
        FA_REQUIRE(scaled_fill_representable(p->type, p->fill),
                   "the inner fill value " + std::to_string(p->fill) + " is not representable in the output type");
    if (c.nz == 0) return false;
    FA_REQUIRE(c.innerU != nullptr && c.innerV != nullptr && c.outerU != nullptr && c.outerV != nullptr && c.outU != nullptr && c.outV != nullptr,
               "NULL data buffer");
    const fimex_amd_regrid_plan &oi = *c.plan->outerToInner, &st = *c.plan->innerToTarget;
    FA_REQUIRE(c.rotOI->ox == oi.outX && c.rotOI->oy == oi.outY, "outerToInnerVec's grid (ox, oy) differs from the inner grid, outerToInner's output grid");
    FA_REQUIRE(c.rotST->ox == st.outX && c.rotST->oy == st.outY, "innerToTargetVec's grid (ox, oy) differs from the target grid, innerToTarget's output grid");
    FA_REQUIRE(c.rotOT->ox == st.outX && c.rotOT->oy == st.outY, "outerToTargetVec's grid (ox, oy) differs from the target grid, outerToTarget's output grid");
    for (const fimex_amd_vector_plan* r : {c.rotOI, c.rotST, c.rotOT})
        FA_REQUIRE(r->device == c.plan->device, "the merge plan and a vector plan live on different devices");
    const size_t inner = c.nz * oi.outX * oi.outY, outer = c.nz * oi.inX * oi.inY, target = c.nz * st.outX * st.outY;
    b = {inner * sIu, inner * sIv, outer * sOu, outer * sOv, target * sIu, target * sIv};
    auto apart_from_inputs = [&](const void* out, size_t outBytes) {
        require_no_overlap(out, outBytes, {{c.innerU, b.innerU, "the inner field's x component"}, {c.innerV, b.innerV, "the inner field's y component"},
                                           {c.outerU, b.outerU, "the outer field's x component"}, {c.outerV, b.outerV, "the outer field's y component"}});
    };
    apart_from_inputs(c.outU, b.targetU);
    apart_from_inputs(c.outV, b.targetV);
    require_no_overlap(c.outU, b.targetU, {{c.outV, b.targetV, "the other output buffer"}});
    return true;
}

PackedVectorFields fields_of(const VectorTypedMergeCall& c, const void* dIu, const void* dIv, const void* dOu, const void* dOv)
{
    return {dIu, dIv, dOu, dOv, *c.pIu, *c.pIv, *c.pOu, *c.pOv};
}

// the fused kernels where they serve the call, else the chain; returns the path
int launch_merge_vector_typed(const VectorTypedMergeCall& c, const PackedVectorFields& in, void* dOutU, void* dOutV, hipStream_t stream)
{
    if (launch_merge_vector_typed_fused(*c.plan, *c.rotOI, *c.rotST, *c.rotOT, in, c.nz, dOutU, dOutV, stream)) return 1;
    launch_merge_vector_typed_chain(*c.plan, *c.rotOI, *c.rotST, *c.rotOT, in, c.nz, dOutU, dOutV, stream);
    return 0;
}

}  // namespace

extern "C" {

int fimex_amd_merge_apply_vector_typed_device(const fimex_amd_merge_plan* plan, const fimex_amd_vector_plan* outerToInnerVec,
                                              const fimex_amd_vector_plan* innerToTargetVec, const fimex_amd_vector_plan* outerToTargetVec,
                                              const void* d_innerU, const fimex_amd_packing* innerUPacking, const void* d_innerV,
                                              const fimex_amd_packing* innerVPacking, const void* d_outerU, const fimex_amd_packing* outerUPacking,
                                              const void* d_outerV, const fimex_amd_packing* outerVPacking, size_t nz, void* d_outU, void* d_outV,
                                              void* stream, int* path)
{
    return c_guard([&] {
        if (path) *path = 0;
        const VectorTypedMergeCall c{plan, outerToInnerVec, innerToTargetVec, outerToTargetVec, d_innerU, innerUPacking, d_innerV, innerVPacking,
                                     d_outerU, outerUPacking, d_outerV, outerVPacking, nz, d_outU, d_outV};
        MergeBytes b{};
        if (!check_merge_vector_typed_call(c, b)) return;
        require_current_device(plan->device);
        const int taken = launch_merge_vector_typed(c, fields_of(c, d_innerU, d_innerV, d_outerU, d_outerV), d_outU, d_outV, as_stream(stream));
        if (path) *path = taken;
    });
}

int fimex_amd_merge_apply_vector_typed_chain_device(const fimex_amd_merge_plan* plan, const fimex_amd_vector_plan* outerToInnerVec,
                                                    const fimex_amd_vector_plan* innerToTargetVec, const fimex_amd_vector_plan* outerToTargetVec,
                                                    const void* d_innerU, const fimex_amd_packing* innerUPacking, const void* d_innerV,
                                                    const fimex_amd_packing* innerVPacking, const void* d_outerU,
                                                    const fimex_amd_packing* outerUPacking, const void* d_outerV,
                                                    const fimex_amd_packing* outerVPacking, size_t nz, void* d_outU, void* d_outV, void* stream)
{
    return c_guard([&] {
        const VectorTypedMergeCall c{plan, outerToInnerVec, innerToTargetVec, outerToTargetVec, d_innerU, innerUPacking, d_innerV, innerVPacking,
                                     d_outerU, outerUPacking, d_outerV, outerVPacking, nz, d_outU, d_outV};
        MergeBytes b{};
        if (!check_merge_vector_typed_call(c, b)) return;
        require_current_device(plan->device);
        launch_merge_vector_typed_chain(*plan, *outerToInnerVec, *innerToTargetVec, *outerToTargetVec,
                                        fields_of(c, d_innerU, d_innerV, d_outerU, d_outerV), nz, d_outU, d_outV, as_stream(stream));
    });
}

// the host form switches to the plan's device, the device forms demand it; only stored-type bytes cross to the device and back
int fimex_amd_merge_apply_vector_typed_host(const fimex_amd_merge_plan* plan, const fimex_amd_vector_plan* outerToInnerVec,
                                            const fimex_amd_vector_plan* innerToTargetVec, const fimex_amd_vector_plan* outerToTargetVec,
                                            const void* innerU, const fimex_amd_packing* innerUPacking, const void* innerV,
                                            const fimex_amd_packing* innerVPacking, const void* outerU, const fimex_amd_packing* outerUPacking,
                                            const void* outerV, const fimex_amd_packing* outerVPacking, size_t nz, void* outU, void* outV)
{
    return c_guard([&] {
        const VectorTypedMergeCall c{plan, outerToInnerVec, innerToTargetVec, outerToTargetVec, innerU, innerUPacking, innerV, innerVPacking,
                                     outerU, outerUPacking, outerV, outerVPacking, nz, outU, outV};
        MergeBytes b{};
        if (!check_merge_vector_typed_call(c, b)) return;
        ScopedDevice dev(plan->device);
        HostCall hc;
        const void *dIu = hc.in_bytes(innerU, b.innerU), *dIv = hc.in_bytes(innerV, b.innerV);
        const void *dOu = hc.in_bytes(outerU, b.outerU), *dOv = hc.in_bytes(outerV, b.outerV);
        void *dOutU = hc.out_bytes(outU, b.targetU), *dOutV = hc.out_bytes(outV, b.targetV);
        launch_merge_vector_typed(c, fields_of(c, dIu, dIv, dOu, dOv), dOutU, dOutV, hc.stream());
        hc.finish();
    });
}

}  // extern "C"
