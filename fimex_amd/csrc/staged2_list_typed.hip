// The stored-type kernel of the second staged form on a LIST of variables (fimex_amd_regrid_apply_multi_typed_device): one launch
// regrids the slices of up to kSliceListMaxVars arrays of one 1- or 2-byte type, each with a fill value of its own.  Text and ring
// are the array kernel's (staged2_apply_typed_kernel.hpp), the plan form is staged2_typed_form's, the launch layout is the one an array
// of the same number of slices gets (launch_staged2_apply_typed).
#include "staged2_apply_typed.hpp"

// the kernel on the slices of a list
#define STAGED2_KERNEL staged_apply2_list_typed
#define STAGED2_SLICES ListSlices
#define STAGED2_LIST_PARAM , SliceListArgs l, TypedListEdge edges
#define STAGED2_LIST &l
#define STAGED2_EDGES (&edges)
#include "staged2_apply_typed_kernel.hpp"
#undef STAGED2_KERNEL
#undef STAGED2_SLICES
#undef STAGED2_LIST_PARAM
#undef STAGED2_LIST
#undef STAGED2_EDGES

namespace fimex_amd {

namespace {

// the form's workgroup shape in the product build, 512 threads; rings of two slots, of three in the tuning build too
// (STAGE2T_DEPTH).  Any other shape (STAGE2T_NT): the caller runs the variables one by one.
bool list_shape(const Staged2Plan& s)
{
    return s.nt == 512 && s.kmax == 6 && (s.depth == 2 || (kTuningBuild && s.depth == 3));
}

template <int STENCIL, typename T>
void launch_list_shape(const Staged2Plan& s, const Staged2Args& a, const TypedEdge& te, const SliceListArgs& l, const TypedListEdge& edges, dim3 grid,
                       hipStream_t stream)
{
    auto go = [&](auto kernel) {
        allow_dynamic_lds(reinterpret_cast<const void*>(kernel), s.ldsBytes);
        kernel<<<grid, 512, s.ldsBytes, stream>>>(a, te, l, edges);
    };
    const bool pair = te.pairStore != 0;
    if constexpr (kTuningBuild) {
        if (s.depth == 3) return pair ? go(&staged_apply2_list_typed<STENCIL, 512, 6, T, true, 3>) : go(&staged_apply2_list_typed<STENCIL, 512, 6, T, false, 3>);
    }
    pair ? go(&staged_apply2_list_typed<STENCIL, 512, 6, T, true, 2>) : go(&staged_apply2_list_typed<STENCIL, 512, 6, T, false, 2>);
}

}  // namespace

// the two facts the rule (typed_list) leaves to the launcher: the plan has a form for the type, of a shape above
bool staged2_list_typed_serves(const fimex_amd_regrid_plan& plan, int cdmType, hipStream_t stream)
{
    const Staged2Plan* form = staged2_typed_form(plan, dispatch::staged_elem_bytes(cdmType), stream);
    return form && list_shape(*form);
}

void launch_staged2_apply_list_typed(const fimex_amd_regrid_plan& plan, size_t nvar, const void* const* d_in, int cdmType, const size_t* nz,
                                     const double* badValue, void* const* d_out, hipStream_t stream)
{
    const uint32_t eb = dispatch::staged_elem_bytes(cdmType);
    const Staged2Plan* form = eb ? staged2_typed_form(plan, eb, stream) : nullptr;
    FA_REQUIRE(form && list_shape(*form), "staged2 typed list: no kernel for this plan and type");
    SliceListArgs l{};
    TypedListEdge edges{};
    uint32_t index[kSliceListMaxVars];
    size_t total = 0;
    FA_REQUIRE(build_slice_ends(nz, nvar, l.e, index, total), "staged2 typed list: too many variables or slices for one launch");
    if (total == 0) return;
    // two results per store where the row length and every variable's start allow aligned 4-byte (2-byte) stores
    bool pair = plan.outX % 2 == 0 && tuning("STAGE2T_PAIR", 1) != 0;
    for (uint32_t k = 0; k < l.e.nvar; ++k) {
        const uint32_t i = index[k];
        FA_REQUIRE(reinterpret_cast<uintptr_t>(d_in[i]) % 4 == 0, "staged2 typed list: a source is not 4-byte aligned");
        l.in[k] = static_cast<const char*>(d_in[i]);
        l.out[k] = static_cast<char*>(d_out[i]);
        edges.bad[k] = (float)badValue[i];
        edges.fillOut[k] = badValue[i];
        pair = pair && reinterpret_cast<uintptr_t>(d_out[i]) % 4 == 0;
    }
    const Staged2Plan& s = *form;
    Staged2Args a = staged2_args(plan, s, nullptr, nullptr, eb, total);
    const uint32_t n = typed_z_chunk_count(total, (uint32_t)tuning("STAGE2T_ZPB", 50));
    set_z_chunks(a, even_z_split(total, n), true);
    TypedEdge te{};  // (bad, hasBad and fillOut: per variable, in `edges`)
    te.pairStore = pair ? 1u : 0u;
    const dim3 grid(s.gridX * n, 1, 1);
    const bool nearest = plan.kind == PlanKind::Nearest;
    auto go = [&](auto t) {
        using T = decltype(t);
        nearest ? launch_list_shape<1, T>(s, a, te, l, edges, grid, stream) : launch_list_shape<2, T>(s, a, te, l, edges, grid, stream);
    };
    switch (cdmType) {
    case FIMEX_AMD_CDM_CHAR: go((signed char)0); break;
    case FIMEX_AMD_CDM_UCHAR: go((unsigned char)0); break;
    case FIMEX_AMD_CDM_SHORT: go((short)0); break;
    default: go((unsigned short)0); break;
    }
    FA_HIP(hipGetLastError());
}

}  // namespace fimex_amd
