// The float kernel of the second LDS-staged regrid form and its launch (the form itself: staged2_plan.hip).
#include "staged2_apply.hpp"

// the kernel on the slices of one array
#define STAGED2_KERNEL staged_apply2
#define STAGED2_SLICES ArraySlices
#define STAGED2_LIST_PARAM
#define STAGED2_LIST nullptr
#include "staged2_apply_kernel.hpp"
#undef STAGED2_KERNEL
#undef STAGED2_SLICES
#undef STAGED2_LIST_PARAM
#undef STAGED2_LIST

namespace fimex_amd {

namespace {

template <int STENCIL, int NT, int PER, int KMAX, bool FAST = false>
void launch_one(const Staged2Args& a, dim3 grid, size_t ldsBytes, uint32_t depth, hipStream_t stream)
{
    auto go = [&](auto kernel) {
        allow_dynamic_lds(reinterpret_cast<const void*>(kernel), ldsBytes);
        kernel<<<grid, NT, ldsBytes, stream>>>(a);
    };
    depth == 3 ? go(&staged_apply2<STENCIL, NT, PER, KMAX, FAST, 3>) : go(&staged_apply2<STENCIL, NT, PER, KMAX, FAST, 2>);
}

template <int STENCIL, bool FAST = false>
void launch_shape(const Staged2Plan& s, const Staged2Args& a, dim3 grid, hipStream_t stream)
{
    const uint32_t key = s.nt * 10000 + s.per * 100 + s.kmax;
    switch (key) {
    case 2560406: launch_one<STENCIL, 256, 4, 6, FAST>(a, grid, s.ldsBytes, s.depth, stream); break;
    case 5120406: launch_one<STENCIL, 512, 4, 6, FAST>(a, grid, s.ldsBytes, s.depth, stream); break;
    case 10240405: launch_one<STENCIL, 1024, 4, 5, FAST>(a, grid, s.ldsBytes, s.depth, stream); break;
    case 5120203: launch_one<STENCIL, 512, 2, 3, FAST>(a, grid, s.ldsBytes, s.depth, stream); break;
    case 10240203: launch_one<STENCIL, 1024, 2, 3, FAST>(a, grid, s.ldsBytes, s.depth, stream); break;
    case 2560204: launch_one<STENCIL, 256, 2, 4, FAST>(a, grid, s.ldsBytes, s.depth, stream); break;
    default: throw Error("staged2: unexpected workgroup shape");
    }
}

}  // namespace

int staged2_float_launch_order(const fimex_amd_regrid_plan& plan, size_t nz)
{
    return launch_order_of(tuning("STAGE2_ORDER", plan.chunkXcd ? kChunkPerXcd : kTileMajor), true, nz, staged2_zpb());
}

void launch_staged2_apply(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, float* d_out, hipStream_t stream)
{
    const Staged2Plan& s = staged2_shape_of(plan);
    Staged2Args a = staged2_args(plan, s, d_in, d_out, 4, nz);
    const dim3 grid = staged2_z_chunks(a, s, nz, plan.chunkXcd ? kChunkPerXcd : kTileMajor, true);
    set_store_policy(a);
    switch (plan.kind) {
    case PlanKind::Nearest: launch_shape<1>(s, a, grid, stream); break;
    case PlanKind::Bilinear: launch_shape<2>(s, a, grid, stream); break;
    default:
        if (plan.bicubicFast) launch_shape<4, true>(s, a, grid, stream);
        else launch_shape<4>(s, a, grid, stream);
        break;
    }
    FA_HIP(hipGetLastError());
}

}  // namespace fimex_amd
