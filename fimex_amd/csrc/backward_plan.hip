// Backward-mapping regrid for gfx950: plan classification, and the launch of the form of the apply that the rule names for a
// call -- the two LDS-staged ones (staged.hip, staged2.hip) or the per-lane gather (gather.hip).  The rule: backward_dispatch.hpp.
//
// The reference keeps two doubles per output cell and re-derives floor / fraction / border class for every cell of every call
// (src/interpolation.c:862-1028); here that runs once per plan (plan.hpp).
#include "plan.hpp"
#include "stencil_math.hpp"

#include "slice_list.hpp"

namespace fimex_amd {

namespace {

struct PlanCounters {
    unsigned long long undefined;
    unsigned long long border;
};

// ---------------------------------------------------------------- plan classification
// One output cell per lane: classify<STENCIL> (stencil_math.hpp) says which source cells it reads, the entry is encoded from that.
// src/interpolation.c:864-868
__global__ void __launch_bounds__(kBlock) classify_nearest(const double* __restrict__ px, const double* __restrict__ py,
                                                           uint32_t n, int64_t ix, int64_t iy,
                                                           uint32_t* __restrict__ pos, PlanCounters* counters)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const CellNeed c = classify<1>(px[i], py[i], ix, iy);
    pos[i] = encode_pos(c, ix);
    if (!c.valid) atomicAdd(&counters->undefined, 1ull);
}

// src/interpolation.c:883-954 without the z loops
__global__ void __launch_bounds__(kBlock) classify_bilinear(const double* __restrict__ px, const double* __restrict__ py,
                                                            uint32_t n, int64_t ix, int64_t iy,
                                                            uint32_t* __restrict__ pos, float* __restrict__ xf,
                                                            float* __restrict__ yf, PlanCounters* counters)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double x = px[i], y = py[i];
    const CellNeed c = classify<2>(x, y, ix, iy);
    const bool oneColumn = c.xa == c.xb, oneRow = c.ya == c.yb;
    pos[i] = encode_pos(c, ix);
    xf[i] = encode_frac_bilinear(c, oneColumn, x);
    yf[i] = encode_frac_bilinear(c, oneRow, y);
    if (!c.valid) atomicAdd(&counters->undefined, 1ull);
    else if (oneColumn || oneRow) atomicAdd(&counters->border, 1ull);
}

// src/interpolation.c:970-976
__global__ void __launch_bounds__(kBlock) classify_bicubic(const double* __restrict__ px, const double* __restrict__ py,
                                                           uint32_t n, int64_t ix, int64_t iy,
                                                           uint32_t* __restrict__ pos, double* __restrict__ xfd,
                                                           double* __restrict__ yfd, PlanCounters* counters)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double x = px[i], y = py[i];
    const CellNeed c = classify<4>(x, y, ix, iy);
    pos[i] = encode_pos(c, ix);
    xfd[i] = encode_frac_bicubic(c, x);
    yfd[i] = encode_frac_bicubic(c, y);
    if (!c.valid) atomicAdd(&counters->undefined, 1ull);
}

}  // namespace

void build_backward_plan(fimex_amd_regrid_plan& plan, const double* d_px, const double* d_py, hipStream_t stream)
{
    const size_t n = plan.outX * plan.outY;
    FA_REQUIRE(n > 0 && n <= kMaxSliceCells, "output grid must have between 1 and 2^30-1 cells per slice");
    FA_REQUIRE(plan.inX > 0 && plan.inY > 0 && plan.inX * plan.inY <= kMaxSliceCells,
               "input grid must have between 1 and 2^30-1 cells per slice");
    DeviceArray<PlanCounters> counters(1);
    FA_HIP(hipMemsetAsync(counters.get(), 0, sizeof(PlanCounters), stream));
    const dim3 grid((uint32_t)ceil_div(n, kBlock));
    plan.pos.allocate(n);
    switch (plan.kind) {
    case PlanKind::Nearest:
        classify_nearest<<<grid, kBlock, 0, stream>>>(d_px, d_py, (uint32_t)n, (int64_t)plan.inX, (int64_t)plan.inY,
                                                      plan.pos.get(), counters.get());
        plan.info.planBytes = plan.pos.bytes();
        break;
    case PlanKind::Bilinear:
        plan.xf.allocate(n);
        plan.yf.allocate(n);
        classify_bilinear<<<grid, kBlock, 0, stream>>>(d_px, d_py, (uint32_t)n, (int64_t)plan.inX, (int64_t)plan.inY,
                                                       plan.pos.get(), plan.xf.get(), plan.yf.get(), counters.get());
        plan.info.planBytes = plan.pos.bytes() + plan.xf.bytes() + plan.yf.bytes();
        break;
    case PlanKind::Bicubic:
        plan.xfd.allocate(n);
        plan.yfd.allocate(n);
        classify_bicubic<<<grid, kBlock, 0, stream>>>(d_px, d_py, (uint32_t)n, (int64_t)plan.inX, (int64_t)plan.inY,
                                                      plan.pos.get(), plan.xfd.get(), plan.yfd.get(), counters.get());
        plan.info.planBytes = plan.pos.bytes() + plan.xfd.bytes() + plan.yfd.bytes();
        break;
    default:
        throw Error("build_backward_plan: not a backward plan");
    }
    FA_HIP(hipGetLastError());
    PlanCounters h{};
    FA_HIP(hipMemcpyAsync(&h, counters.get(), sizeof(h), hipMemcpyDeviceToHost, stream));
    FA_HIP(hipStreamSynchronize(stream));
    plan.info.undefinedCells = (size_t)h.undefined;
    plan.info.borderCells = (size_t)h.border;
    // also the LDS-staged form (staged.hip); plans whose tiles do not fit keep the gather kernel only
    const dispatch::Switches sw = dispatch_switches();
    if (dispatch::builds_first(sw, plan_facts(plan)) && build_staged_plan(plan, d_px, d_py, stream)) {
        const auto& s = plan.staged;  // the staged kernel reads LDS offsets instead of pos, plus the tile tables
        plan.info.planBytes = plan.info.planBytes - plan.pos.bytes() + s.ldsA.bytes() + s.ldsB.bytes() + s.tileHdr.bytes() +
                              (size_t)s.nTiles * 2 * 4 * 48;
        plan.info.stagedCells = s.stagedCells;
        plan.info.tileW = s.tileW;
        plan.info.tileH = s.tileH;
    }
    // the second staged form (staged2.hip), where the plan will prefer it for float slices
    if (dispatch::builds_second(sw, plan_facts(plan)) && build_staged2_plan(plan, d_px, d_py, stream)) {
        const auto& s = plan.staged2;
        const size_t perCell = plan.kind == PlanKind::Nearest ? 0 : (plan.kind == PlanKind::Bilinear ? plan.xf.bytes() + plan.yf.bytes()
                                                                                                       : plan.xfd.bytes() + plan.yfd.bytes());
        auto bytes_of = [&](const Staged2Plan& q) {
            return perCell + q.ldsA.bytes() + q.ldsB.bytes() + q.totalChunks * 4 + (size_t)q.nTiles * sizeof(StagedTile) + q.order.bytes();
        };
        plan.planBytesShape[0] = bytes_of(s);
        plan.planBytesShape[1] = plan.staged2Alt.valid ? bytes_of(plan.staged2Alt) : 0;
        plan.info.planBytes = plan.planBytesShape[0];
        plan.info.stagedCells = s.stagedCells;
        plan.info.tileW = s.tileWMax;
        plan.info.tileH = s.tileH;
    }
}

// the one reader of the switches of backward_dispatch.hpp (tests/test_backward_dispatch.py holds every other file to that)
dispatch::Switches dispatch_switches()
{
    dispatch::Switches sw{};
    sw.staged = tuning("STAGED", 1);
    sw.stagedNearest = tuning("STAGED_NEAREST", 1);
    sw.staged2 = tuning("STAGED2", 1);
    sw.typedFused = tuning("TYPED_FUSED", 1);
    sw.typedStaged = tuning("TYPED_STAGED", 1);
    sw.typedStaged2 = tuning("TYPED_STAGED2", 1);
    sw.vectorFused = tuning("VECTOR_FUSED", 1);
    sw.stagedMinNz = (uint64_t)tuning("STAGED_MIN_NZ", 4);
    return sw;
}

int backward_launch_order(const fimex_amd_regrid_plan& plan, size_t nz)
{
    const bool second = dispatch::float_apply(dispatch_switches(), plan_facts(plan), nz) == dispatch::FloatApply::Second;
    return second ? staged2_float_launch_order(plan, nz) : -1;
}

void launch_backward_apply(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, float* d_out, hipStream_t stream)
{
    if (nz == 0) return;
    FA_REQUIRE(nz <= 0xFFFFFFFFu, "too many slices");
    switch (dispatch::float_apply(dispatch_switches(), plan_facts(plan), nz)) {
    case dispatch::FloatApply::Second: launch_staged2_apply(plan, d_in, nz, d_out, stream); break;
    case dispatch::FloatApply::First: launch_staged_apply(plan, d_in, nz, d_out, stream); break;
    case dispatch::FloatApply::Gather: launch_backward_gather(plan, d_in, nz, d_out, stream); break;
    }
}

// One kernel on the stored type where the rule has one; false: the caller runs the three passes (to float, regrid, from float)
bool launch_typed_apply(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double badValue, void* d_out,
                        hipStream_t stream)
{
    // forward plans with long buckets: the LDS-staged forward kernel on the stored type (forward_tiled.hip)
    if (plan.kind == PlanKind::Forward) return launch_forward_tiled_typed(plan, d_in, cdmType, nz, badValue, d_out, stream);
    const dispatch::TypedCandidates t = dispatch::typed_apply(dispatch_switches(), plan_facts(plan), {nz, cdmType, cdmType, aligned4(d_in)});
    for (int i = 0; i < t.n; ++i) {
        switch (t.c[i]) {
        case dispatch::TypedApply::Second:  // (the plan may turn out to have no form for this element size)
            if (launch_staged2_apply_typed(plan, d_in, cdmType, nz, badValue, d_out, stream)) return true;
            break;
        case dispatch::TypedApply::First: launch_staged_apply_typed(plan, d_in, cdmType, nz, badValue, d_out, stream); return true;
        case dispatch::TypedApply::Gather: launch_typed_gather(plan, d_in, cdmType, nz, badValue, d_out, stream); return true;
        case dispatch::TypedApply::ThreePasses: return false;
        }
    }
    return false;
}

bool launch_backward_apply_list(const fimex_amd_regrid_plan& plan, size_t nvar, const float* const* d_in, const size_t* nz, float* const* d_out,
                                hipStream_t stream)
{
    const dispatch::Switches sw = dispatch_switches();
    if (!dispatch::float_list(sw, plan_facts(plan), list_slices(nz, nvar)) || !staged2_list_serves(plan)) return false;
    for_list_launches(nz, nvar, [&](size_t first, size_t count) {
        launch_staged2_apply_list(plan, sw, count, d_in + first, nz + first, d_out + first, stream);
    });
    return true;
}

bool launch_typed_apply_list(const fimex_amd_regrid_plan& plan, size_t nvar, const void* const* d_in, int cdmType, const size_t* nz,
                             const double* badValue, void* const* d_out, hipStream_t stream)
{
    bool aligned = true;
    for (size_t i = 0; i < nvar; ++i) aligned = aligned && (nz[i] == 0 || aligned4(d_in[i]));
    if (!dispatch::typed_list(dispatch_switches(), plan_facts(plan), {list_slices(nz, nvar), cdmType, cdmType, aligned}) ||
        !staged2_list_typed_serves(plan, cdmType, stream))
        return false;
    for_list_launches(nz, nvar, [&](size_t first, size_t count) {
        launch_staged2_apply_list_typed(plan, count, d_in + first, cdmType, nz + first, badValue + first, d_out + first, stream);
    });
    return true;
}

}  // namespace fimex_amd
