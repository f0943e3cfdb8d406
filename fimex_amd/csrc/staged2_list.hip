// The float kernel of the second staged form on a LIST of variables (fimex_amd_regrid_apply_multi_device): one launch regrids the
// slices of up to kSliceListMaxVars arrays [nz[i]][inY][inX].  Text and ring are the array kernel's (staged2_apply_kernel.hpp); the
// slices are addressed through ListSlices (staged2_ring.hpp, slice_list.hpp), the launch layout is the one an array of the same
// number of slices gets.
#include "staged2_apply.hpp"

// the kernel on the slices of a list
#define STAGED2_KERNEL staged_apply2_list
#define STAGED2_SLICES ListSlices
#define STAGED2_LIST_PARAM , SliceListArgs l
#define STAGED2_LIST &l
#include "staged2_apply_kernel.hpp"
#undef STAGED2_KERNEL
#undef STAGED2_SLICES
#undef STAGED2_LIST_PARAM
#undef STAGED2_LIST

namespace fimex_amd {

namespace {

template <int STENCIL, int NT, int PER, int KMAX, bool FAST>
void launch_list_one(const Staged2Args& a, const SliceListArgs& l, dim3 grid, size_t ldsBytes, uint32_t depth, hipStream_t stream)
{
    auto go = [&](auto kernel) {
        allow_dynamic_lds(reinterpret_cast<const void*>(kernel), ldsBytes);
        kernel<<<grid, NT, ldsBytes, stream>>>(a, l);
    };
    if constexpr (kTuningBuild) {  // (STAGE2_DEPTH: the product build's plans have rings of two slots)
        if (depth == 3) return go(&staged_apply2_list<STENCIL, NT, PER, KMAX, FAST, 3>);
    }
    go(&staged_apply2_list<STENCIL, NT, PER, KMAX, FAST, 2>);
}

// The list kernels exist for the workgroup shapes a plan of the product build can hold (build_staged2_plan, staged2_plan.hip):
// 1024 threads for the 1 x 1 and 2 x 2 stencils, 512 for the 2 x 2 stencil's second shape and the 4 x 4 stencil in float
// arithmetic, 256 for that stencil's second shape; rings of two slots, of three in the tuning build too.  Any other shape
// (STAGE2_NT and its like in the tuning build): false, the caller runs the variables one by one.
bool list_shape(const fimex_amd_regrid_plan& plan, const Staged2Plan& s)
{
    const uint32_t key = s.nt * 10000 + s.per * 100 + s.kmax;
    if (s.depth != 2 && !(kTuningBuild && s.depth == 3)) return false;
    switch (plan.kind) {
    case PlanKind::Nearest: return key == 10240405;
    case PlanKind::Bilinear: return key == 10240405 || key == 5120406;
    case PlanKind::Bicubic: return plan.bicubicFast && (key == 5120406 || key == 2560406);
    default: return false;
    }
}

}  // namespace

bool staged2_list_serves(const fimex_amd_regrid_plan& plan)
{
    return list_shape(plan, staged2_shape_of(plan));
}

void launch_staged2_apply_list(const fimex_amd_regrid_plan& plan, const dispatch::Switches& sw, size_t nvar, const float* const* d_in,
                               const size_t* nz, float* const* d_out, hipStream_t stream)
{
    SliceListArgs l{};
    uint32_t index[kSliceListMaxVars];
    size_t total = 0;
    FA_REQUIRE(build_slice_ends(nz, nvar, l.e, index, total), "staged2 list: too many variables or slices for one launch");
    if (total == 0) return;
    for (uint32_t k = 0; k < l.e.nvar; ++k) {
        l.in[k] = reinterpret_cast<const char*>(d_in[index[k]]);
        l.out[k] = reinterpret_cast<char*>(d_out[index[k]]);
    }
    // float arithmetic only for the variables whose own call would run this form (launch_backward_apply)
    if (plan.kind == PlanKind::Bicubic)
        for (uint32_t k = 0; k < l.e.nvar; ++k)
            if (dispatch::float_apply(sw, plan_facts(plan), nz[index[k]]) != dispatch::FloatApply::Second) l.exactMask |= 1ull << k;
    const Staged2Plan& s = staged2_shape_of(plan);
    FA_REQUIRE(list_shape(plan, s), "staged2 list: no kernel for this workgroup shape");
    Staged2Args a = staged2_args(plan, s, nullptr, nullptr, 4, total);
    const dim3 grid = staged2_z_chunks(a, s, total, plan.chunkXcd ? kChunkPerXcd : kTileMajor, true);
    set_store_policy(a);
    const uint32_t nt = s.nt;
    switch (plan.kind) {
    case PlanKind::Nearest: launch_list_one<1, 1024, 4, 5, false>(a, l, grid, s.ldsBytes, s.depth, stream); break;
    case PlanKind::Bilinear:
        if (nt == 1024) launch_list_one<2, 1024, 4, 5, false>(a, l, grid, s.ldsBytes, s.depth, stream);
        else launch_list_one<2, 512, 4, 6, false>(a, l, grid, s.ldsBytes, s.depth, stream);
        break;
    default:
        if (nt == 512) launch_list_one<4, 512, 4, 6, true>(a, l, grid, s.ldsBytes, s.depth, stream);
        else launch_list_one<4, 256, 4, 6, true>(a, l, grid, s.ldsBytes, s.depth, stream);
        break;
    }
    FA_HIP(hipGetLastError());
}

}  // namespace fimex_amd
