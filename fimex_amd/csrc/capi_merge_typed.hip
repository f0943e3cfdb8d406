// extern "C" boundary, grid merging on variables in their stored types: typed border smoothing, typed overlay and the typed
// merge applies (merge_typed.hip).  Each device / host pair of the elementwise entries is one template over the call type
// (host_call.hpp).
#include "capi_checks.hpp"
#include "host_call.hpp"

#include "../../include/fimex_amd_merge_typed_host.h"

using namespace fimex_amd;

namespace {

struct PackedPair {
    size_t sizeI, sizeO;  // element sizes of the inner (top) and the outer (base) variable
};

// NULL packings, types without element size, an output fill value that the inner's type cannot hold: before anything else is
// looked at
PackedPair check_packings(const fimex_amd_packing* inner, const fimex_amd_packing* outer)
{
    FA_REQUIRE(inner != nullptr && outer != nullptr, "NULL packing");
    const PackedPair p{cdm_type_size(inner->type), cdm_type_size(outer->type)};  // throws for NAT and STRING
    FA_REQUIRE(scaled_fill_representable(inner->type, inner->fill),
               "the inner fill value " + std::to_string(inner->fill) + " is not representable in the output type");
    return p;
}

// out against one input of n elements: the input itself where every cell is read before it is written over, apart otherwise
void require_same_or_apart(const void* out, size_t outBytes, const void* in, size_t inBytes, bool sameAllowed, const char* name)
{
    if (out == in && sameAllowed) return;
    require_no_overlap(out, outBytes, {{in, inBytes, name}});
}

template <class Call>
void border_smooth_typed(Call&& c, const void* inner, const fimex_amd_packing* pi, const void* outerOnInner, const fimex_amd_packing* po, void* out,
                         size_t nx, size_t ny, size_t nz, size_t transitionWidth, size_t borderWidth, int useOuterIfInnerUndefined)
{
    const PackedPair p = check_packings(pi, po);
    FA_REQUIRE(transitionWidth > 0, "invalid parameter values for linear smoothing (transitionWidth == 0)");
    FA_REQUIRE(nx > 0 && ny > 0, "empty grid (nx == 0 or ny == 0)");
    if (nz == 0) return;
    FA_REQUIRE(inner != nullptr && outerOnInner != nullptr && out != nullptr, "NULL data buffer");
    const size_t n = nx * ny * nz;
    require_same_or_apart(out, n * p.sizeI, inner, n * p.sizeI, true, "the inner field (other than in place)");
    require_same_or_apart(out, n * p.sizeI, outerOnInner, n * p.sizeO, p.sizeI == p.sizeO,
                          "the outer field (in place needs types of one size)");
    (void)current_device_checked();
    const void* dI = c.in_bytes(inner, n * p.sizeI);
    const void* dO = c.in_bytes(outerOnInner, n * p.sizeO);
    // a device call hands its pointers through: where out is one of the inputs the kernel works in place; a host call has three buffers
    launch_border_smooth_typed(dI, *pi, dO, *po, c.out_bytes(out, n * p.sizeI), nx, ny, nz, transitionWidth, borderWidth,
                               useOuterIfInnerUndefined != 0, c.stream());
    c.finish();
}

template <class Call>
void overlay_typed(Call&& c, const void* top, const fimex_amd_packing* pt, const void* base, const fimex_amd_packing* pb, void* out, size_t n)
{
    const PackedPair p = check_packings(pt, pb);
    if (n == 0) return;
    FA_REQUIRE(top != nullptr && base != nullptr && out != nullptr, "NULL data buffer");
    require_same_or_apart(out, n * p.sizeI, top, n * p.sizeI, true, "the top field (other than in place)");
    require_same_or_apart(out, n * p.sizeI, base, n * p.sizeO, p.sizeI == p.sizeO, "the base field (in place needs types of one size)");
    (void)current_device_checked();
    const void* dT = c.in_bytes(top, n * p.sizeI);
    const void* dB = c.in_bytes(base, n * p.sizeO);
    launch_overlay_typed(dT, *pt, dB, *pb, c.out_bytes(out, n * p.sizeI), n, c.stream());
    c.finish();
}

struct MergeBytes {
    size_t inner, outer, target;  // bytes of nz slices
};

// false: nothing to do.  The plan is looked into only after everything that can be refused without it
bool check_merge_typed_call(const fimex_amd_merge_plan* plan, const void* inner, const fimex_amd_packing* pi, const void* outer,
                            const fimex_amd_packing* po, size_t nz, const void* out, MergeBytes& bytes)
{
    FA_REQUIRE(plan != nullptr, "NULL plan");
    const PackedPair p = check_packings(pi, po);
    if (nz == 0) return false;
    FA_REQUIRE(inner != nullptr && outer != nullptr && out != nullptr, "NULL data buffer");
    const fimex_amd_regrid_plan &oi = *plan->outerToInner, &st = *plan->innerToTarget;
    bytes = {nz * oi.outX * oi.outY * p.sizeI, nz * oi.inX * oi.inY * p.sizeO, nz * st.outX * st.outY * p.sizeI};
    require_no_overlap(out, bytes.target, {{inner, bytes.inner, "the inner field"}, {outer, bytes.outer, "the outer field"}});
    return true;
}

}  // namespace

extern "C" {

int fimex_amd_border_smooth_typed_device(const void* d_inner, const fimex_amd_packing* innerPacking, const void* d_outerOnInner,
                                         const fimex_amd_packing* outerPacking, void* d_out, size_t nx, size_t ny, size_t nz,
                                         size_t transitionWidth, size_t borderWidth, int useOuterIfInnerUndefined, void* stream)
{
    return c_guard([&] {
        border_smooth_typed(DeviceCall{as_stream(stream)}, d_inner, innerPacking, d_outerOnInner, outerPacking, d_out, nx, ny, nz, transitionWidth,
                            borderWidth, useOuterIfInnerUndefined);
    });
}

int fimex_amd_border_smooth_typed_host(const void* inner, const fimex_amd_packing* innerPacking, const void* outerOnInner,
                                       const fimex_amd_packing* outerPacking, void* out, size_t nx, size_t ny, size_t nz,
                                       size_t transitionWidth, size_t borderWidth, int useOuterIfInnerUndefined)
{
    return c_guard([&] {
        border_smooth_typed(HostCall(), inner, innerPacking, outerOnInner, outerPacking, out, nx, ny, nz, transitionWidth, borderWidth,
                            useOuterIfInnerUndefined);
    });
}

int fimex_amd_overlay_typed_device(const void* d_top, const fimex_amd_packing* topPacking, const void* d_base,
                                   const fimex_amd_packing* basePacking, void* d_out, size_t n, void* stream)
{
    return c_guard([&] { overlay_typed(DeviceCall{as_stream(stream)}, d_top, topPacking, d_base, basePacking, d_out, n); });
}

int fimex_amd_overlay_typed_host(const void* top, const fimex_amd_packing* topPacking, const void* base,
                                 const fimex_amd_packing* basePacking, void* out, size_t n)
{
    return c_guard([&] { overlay_typed(HostCall(), top, topPacking, base, basePacking, out, n); });
}

int fimex_amd_merge_apply_typed_device(const fimex_amd_merge_plan* plan, const void* d_inner, const fimex_amd_packing* innerPacking,
                                       const void* d_outer, const fimex_amd_packing* outerPacking, size_t nz, void* d_out, void* stream,
                                       int* path)
{
    return c_guard([&] {
        if (path) *path = 0;
        MergeBytes bytes{};
        if (!check_merge_typed_call(plan, d_inner, innerPacking, d_outer, outerPacking, nz, d_out, bytes)) return;
        require_current_device(plan->device);
        if (launch_merge_typed_fused(*plan, d_inner, *innerPacking, d_outer, *outerPacking, nz, d_out, as_stream(stream))) {
            if (path) *path = 1;
            return;
        }
        launch_merge_typed_chain(*plan, d_inner, *innerPacking, d_outer, *outerPacking, nz, d_out, as_stream(stream));
    });
}

int fimex_amd_merge_apply_typed_chain_device(const fimex_amd_merge_plan* plan, const void* d_inner, const fimex_amd_packing* innerPacking,
                                             const void* d_outer, const fimex_amd_packing* outerPacking, size_t nz, void* d_out,
                                             void* stream)
{
    return c_guard([&] {
        MergeBytes bytes{};
        if (!check_merge_typed_call(plan, d_inner, innerPacking, d_outer, outerPacking, nz, d_out, bytes)) return;
        require_current_device(plan->device);
        launch_merge_typed_chain(*plan, d_inner, *innerPacking, d_outer, *outerPacking, nz, d_out, as_stream(stream));
    });
}

// not one template with the device form: the host form switches to the plan's device, the device form demands it
int fimex_amd_merge_apply_typed_host(const fimex_amd_merge_plan* plan, const void* inner, const fimex_amd_packing* innerPacking,
                                     const void* outer, const fimex_amd_packing* outerPacking, size_t nz, void* out)
{
    return c_guard([&] {
        MergeBytes bytes{};
        if (!check_merge_typed_call(plan, inner, innerPacking, outer, outerPacking, nz, out, bytes)) return;
        ScopedDevice dev(plan->device);
        HostCall hc;
        const void* dI = hc.in_bytes(inner, bytes.inner);
        const void* dO = hc.in_bytes(outer, bytes.outer);
        void* dOut = hc.out_bytes(out, bytes.target);
        if (!launch_merge_typed_fused(*plan, dI, *innerPacking, dO, *outerPacking, nz, dOut, hc.stream()))
            launch_merge_typed_chain(*plan, dI, *innerPacking, dO, *outerPacking, nz, dOut, hc.stream());
        hc.finish();
    });
}

}  // extern "C"
