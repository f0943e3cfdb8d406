// The second LDS-staged regrid form (staged2.hip) on a variable's STORED type: kernel, form cache and launch (data2InterpolationArray + interpolateValues +
// interpolationArray2Data of src/CDMInterpolator.cc:115-124, 251-285 in one kernel): slices of 1- or 2-byte integers.
// The plan form is its own (built on first use, staged2_typed_form): a 16-byte chunk holds 8 or 16 source cells, LDS offsets
// count elements.  The kernel's text: staged2_apply_typed_kernel.hpp; how it differs from the float kernel: staged2_apply_typed.hpp.
#include "staged2_apply_typed.hpp"

// the kernel on the slices of one array
#define STAGED2_KERNEL staged_apply2_typed
#define STAGED2_SLICES ArraySlices
#define STAGED2_LIST_PARAM
#define STAGED2_LIST nullptr
#define STAGED2_EDGES static_cast<const TypedListEdge*>(nullptr)
#include "staged2_apply_typed_kernel.hpp"
#undef STAGED2_KERNEL
#undef STAGED2_SLICES
#undef STAGED2_LIST_PARAM
#undef STAGED2_LIST
#undef STAGED2_EDGES

namespace fimex_amd {

// the plan's staged form for slices of elemBytes-byte elements (2 or 1), built on first use; nullptr: none (the caller takes
// the first staged form or the gather kernels)
const Staged2Plan* staged2_typed_form(const fimex_amd_regrid_plan& plan, uint32_t elemBytes, hipStream_t stream)
{
    FA_REQUIRE((elemBytes == 1 || elemBytes == 2) && (plan.kind == PlanKind::Nearest || plan.kind == PlanKind::Bilinear) &&
                   (plan.inX * plan.inY * elemBytes) % 4 == 0,
               "staged2 typed: no form for this plan and element size (typed_second, backward_dispatch.hpp)");
    const int idx = elemBytes == 2 ? 0 : 1;
    std::lock_guard<std::mutex> lock(plan.typed2.mtx);
    Staged2Plan& form = plan.typed2.form[idx];
    if (!plan.typed2.tried[idx]) {
        plan.typed2.tried[idx] = true;
        // 512 threads on 256 x 8 tiles, two workgroups per CU: the kernel converts every element it touches and is bound by its
        // instructions as much as by memory, so occupancy counts for more than tile size here
        Shape2 sh{};
        sh.nt = tuning("STAGE2T_NT", 512);
        sh.per = 4;
        sh.kmax = sh.nt == 1024 ? 5 : 6;
        sh.tileW = (uint32_t)tuning("STAGE2T_TW", sh.nt / 2);
        sh.ldsBytes = (uint32_t)tuning("STAGE2T_LDS_KB", sh.nt == 256 ? 39 : (sh.nt == 512 ? 79 : 159)) * 1024u;
        sh.depth = sh.nt == 512 ? (uint32_t)tuning("STAGE2T_DEPTH", 2) : 2u;
        if (!finish_shape(sh, 64)) return nullptr;
        try {
            build_staged2_form(plan, form, nullptr, nullptr, sh, 1, 16u / elemBytes, stream);
        } catch (...) {
            form.valid = false;
            throw;
        }
    }
    return form.valid ? &form : nullptr;
}

namespace {

template <int STENCIL, typename T>
void launch_typed_shape(const Staged2Plan& s, const Staged2Args& a, const TypedEdge& te, dim3 grid, hipStream_t stream)
{
    auto go = [&](auto kernel, int nt) {
        allow_dynamic_lds(reinterpret_cast<const void*>(kernel), s.ldsBytes);
        kernel<<<grid, nt, s.ldsBytes, stream>>>(a, te);
    };
    const bool pair = te.pairStore != 0;
    if (s.nt == 512 && s.depth == 3) {
        pair ? go(&staged_apply2_typed<STENCIL, 512, 6, T, true, 3>, 512) : go(&staged_apply2_typed<STENCIL, 512, 6, T, false, 3>, 512);
        return;
    }
    switch (s.nt) {
    case 256: pair ? go(&staged_apply2_typed<STENCIL, 256, 6, T, true>, 256) : go(&staged_apply2_typed<STENCIL, 256, 6, T, false>, 256); break;
    case 512: pair ? go(&staged_apply2_typed<STENCIL, 512, 6, T, true>, 512) : go(&staged_apply2_typed<STENCIL, 512, 6, T, false>, 512); break;
    case 1024: pair ? go(&staged_apply2_typed<STENCIL, 1024, 5, T, true>, 1024) : go(&staged_apply2_typed<STENCIL, 1024, 5, T, false>, 1024); break;
    default: throw Error("staged2 typed: unexpected workgroup shape");
    }
}

template <typename T>
void launch_typed(bool nearest, const Staged2Plan& s, const Staged2Args& a, const TypedEdge& te, dim3 grid, hipStream_t stream)
{
    nearest ? launch_typed_shape<1, T>(s, a, te, grid, stream) : launch_typed_shape<2, T>(s, a, te, grid, stream);
}

}  // namespace

// data2InterpolationArray + interpolateValues + interpolationArray2Data (src/CDMInterpolator.cc:115-124, 251-285) on slices of
// 1- and 2-byte integers, nearest and bilinear, through the second staged form.  false: the plan has no such form, the caller goes on.
bool launch_staged2_apply_typed(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double badValue, void* d_out,
                                hipStream_t stream)
{
    const uint32_t eb = dispatch::staged_elem_bytes(cdmType);
    FA_REQUIRE(eb != 0 && aligned4(d_in), "staged2 typed: not a call of this kernel (typed_second, backward_dispatch.hpp)");
    if (nz == 0) return true;
    const Staged2Plan* form = staged2_typed_form(plan, eb, stream);
    if (!form) return false;
    const Staged2Plan& s = *form;
    Staged2Args a = staged2_args(plan, s, d_in, d_out, eb, nz);
    // z chunks of about 50 slices (200 slices: 1.354 against 1.364 ms with 25, profiles/r03_sweep_typed*.log), at least four
    // where the batch allows, so that short batches still fill the chip
    const uint32_t n = typed_z_chunk_count(nz, (uint32_t)tuning("STAGE2T_ZPB", 50));
    set_z_chunks(a, even_z_split(nz, n), true);
    TypedEdge te{};
    te.bad = (float)badValue;
    te.hasBad = !(te.bad != te.bad);
    te.fillOut = badValue;
    // two results per store where both the row length and the slice start allow aligned 4-byte (2-byte) stores
    te.pairStore = (plan.outX % 2 == 0 && reinterpret_cast<uintptr_t>(d_out) % 4 == 0 && tuning("STAGE2T_PAIR", 1) != 0) ? 1u : 0u;
    const dim3 grid(s.gridX * n, 1, 1);
    const bool nearest = plan.kind == PlanKind::Nearest;
    switch (cdmType) {
    case FIMEX_AMD_CDM_CHAR: launch_typed<signed char>(nearest, s, a, te, grid, stream); break;
    case FIMEX_AMD_CDM_UCHAR: launch_typed<unsigned char>(nearest, s, a, te, grid, stream); break;
    case FIMEX_AMD_CDM_SHORT: launch_typed<short>(nearest, s, a, te, grid, stream); break;
    default: launch_typed<unsigned short>(nearest, s, a, te, grid, stream); break;
    }
    FA_HIP(hipGetLastError());
    return true;
}

}  // namespace fimex_amd
