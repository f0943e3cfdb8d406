// The second LDS-staged regrid form (staged2.hip) on a variable's STORED type: kernel, form cache and launch (data2InterpolationArray + interpolateValues +
// interpolationArray2Data of src/CDMInterpolator.cc:115-124, 251-285 in one kernel): slices of 1- or 2-byte integers.
// The plan form is its own (built on first use, staged2_typed_form): a 16-byte chunk holds 8 or 16 source cells, LDS offsets
// count elements.  Differences to the float kernel: a lane owns two PAIRS of neighbouring outputs (cells 2 * t, 2 * t + 1 of
// the tile, and the same NT * 2 cells further on), so that two results leave in one 4-byte (2-byte elements) or 2-byte store
// and a wave still writes 256 (128) contiguous bytes; the two source elements of a stencil row arrive in one ds_read2_b32 and
// are shifted apart; elements become float / NaN as Data::asFloat + mifi_bad2nanf do, results go back through ScaleValue's
// rounding (typed_convert.hpp); the element reads and the stores are staged2_lane_ops.hpp's.
#include "staged2_lane_ops.hpp"
#include "staged2_ring.hpp"

namespace fimex_amd {

namespace {

struct TypedEdge {
    float bad;          // the variable's fill value narrowed to float (mifi_bad2nanf's argument)
    uint32_t hasBad;
    double fillOut;     // NaN -> this (interpolationArray2Data)
    uint32_t pairStore; // outX even: the two results of a pair share one store
};

// STENCIL 1 (nearest) or 2 (bilinear); NT threads, 4 outputs per lane (two pairs); KMAX 16-byte chunks per lane and slice
// PAIR: the row length and the slice start allow aligned stores of two results
template <int STENCIL, int NT, int KMAX, typename T, bool PAIR, int DEPTH = 2>
__global__ void __launch_bounds__(NT) staged_apply2_typed(Staged2Args a, TypedEdge te)
{
    static_assert(STENCIL == 1 || STENCIL == 2, "stored types: nearest and bilinear");
    constexpr uint32_t EB = sizeof(T);
    constexpr int PER = 4;
    StagedTile T_;
    uint32_t z0, z1;
    if (!decode_workgroup(a, T_, z0, z1)) return;
    const SliceRing<NT, KMAX, DEPTH> ring(a, T_, z0, z1, EB);
    const bool hasBad = te.hasBad != 0;
    const T fillT = static_cast<T>(te.fillOut);  // ScaleValue's newFill_ (include/fimex/Utils.h:456)
    // per-lane plan: output q = 2 * p + h is cell 2 * threadIdx.x + h + p * 2 * NT of the tile (row-major over the tile's width)
    uint32_t cellOff[PER];       // byte offset inside a typed output slice, ~0u = not mine
    uint32_t row[PER][STENCIL];  // byte offsets of the stencil rows in the staged image
    uint32_t cellIdx[PER];
    float xf[PER], yf[PER];
    bool undef[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const uint32_t e = 2u * threadIdx.x + (uint32_t)(q & 1) + (uint32_t)(q >> 1) * 2u * NT;
        const uint32_t ly = e / T_.w, lx = e - ly * T_.w;
        const uint32_t y = T_.y0 + ly;
        cellOff[q] = 0xFFFFFFFFu;
        cellIdx[q] = 0xFFFFFFFFu;
        uint32_t pa = kInvalidPos;
        xf[q] = yf[q] = 0.f;
        if (ly < a.tileH && y < a.outY) {
            const uint32_t cell = y * a.outX + T_.x0 + lx;
            cellIdx[q] = cell;
            cellOff[q] = cell * EB;
            pa = a.ldsA[cell];
            if (STENCIL == 2) { xf[q] = a.xf[cell]; yf[q] = a.yf[cell]; }
        }
        undef[q] = pa == kInvalidPos;
        row[q][0] = undef[q] ? 0u : (pa & 0xFFFFu) * EB;
        if (STENCIL == 2) row[q][STENCIL - 1] = undef[q] ? 0u : (pa >> 16) * EB;
    }
    if (T_.rsv[0] != 0) {
        // gather tile (see staged_apply2): stencils straight from memory, element by element
        uint32_t p[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            p[q] = (cellIdx[q] != 0xFFFFFFFFu) ? a.pos[cellIdx[q]] : kInvalidPos;
            undef[q] = p[q] == kInvalidPos;
            if (undef[q]) p[q] = 0;
        }
        for (uint32_t z = z0; z < z1; ++z) {
            const rsrc_t rs = ring.in_uniform(z), ro = ring.out_uniform(z);
            auto ld = [&](uint32_t cell) {
                if constexpr (EB == 2) return as_float_nan((T)__builtin_amdgcn_raw_buffer_load_b16(rs, cell * 2u, 0, 0), te.bad, hasBad);
                else return as_float_nan((T)__builtin_amdgcn_raw_buffer_load_b8(rs, cell, 0, 0), te.bad, hasBad);
            };
            float r[PER];
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                if constexpr (STENCIL == 1) {
                    r[q] = ld(p[q]);
                } else {
                    const uint32_t dx = is_nn(xf[q]) ? 0u : 1u, dy = is_nn(yf[q]) ? 0u : a.inX;
                    r[q] = bilinear_value(ld(p[q]), ld(p[q] + dx), ld(p[q] + dy), ld(p[q] + dx + dy), xf[q], yf[q]);
                }
                if (undef[q]) r[q] = undefined_f();
            }
            store_pair<T, PAIR>(ro, cellOff[0], cellOff[1], r[0], r[1], fillT);
            store_pair<T, PAIR>(ro, cellOff[2], cellOff[3], r[2], r[3], fillT);
        }
        return;
    }
    if (T_.nChunks == 0) {  // every output of the tile is undefined
        for (uint32_t z = z0; z < z1; ++z) {
            const rsrc_t ro = ring.out(z);
            store_pair<T, PAIR>(ro, cellOff[0], cellOff[1], undefined_f(), undefined_f(), fillT);
            store_pair<T, PAIR>(ro, cellOff[2], cellOff[3], undefined_f(), undefined_f(), fillT);
        }
        return;
    }
    ring.wait_first();
    constexpr int NST = PAIR ? 2 : 4;  // store instructions a lane issues per slice
    // plain waves and the masks of the border forms: as in staged_apply2
    bool plainWave = true;
#pragma unroll
    for (int q = 0; q < PER; ++q)
        plainWave = plainWave && !undef[q] && (STENCIL != 2 || !(is_nn(xf[q]) || is_nn(yf[q])));
    plainWave = __all(plainWave) != 0;
    uint32_t mNnx[PER], mNny[PER], mUndef[PER];
    uint32_t rowA[PER][STENCIL], rowS[PER][STENCIL];  // bilinear: aligned byte offset of a stencil row's pair, and its shift operand
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        mNnx[q] = nn_mask(xf[q]);
        mNny[q] = nn_mask(yf[q]);
        mUndef[q] = undef[q] ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (int i = 0; i < STENCIL; ++i) { rowA[q][i] = row[q][i] & ~3u; rowS[q][i] = row[q][i] << 3; }
    }
    // no fill value: comparisons with NaN never hold, the loops need no separate test
    const float badCmp = hasBad ? te.bad : undefined_f();
    dispatch_un<KMAX>(ring.un, plainWave, [&](auto unTag, auto plainTag) __attribute__((always_inline)) {
        constexpr bool PLAIN = decltype(plainTag)::value;
        ring.template run<decltype(unTag)::value, NST>([&](uint32_t z, const char* curb) __attribute__((always_inline)) {
            const rsrc_t ro = ring.out(z);
            float r[PER];
            if constexpr (STENCIL == 1) {
#pragma unroll
                for (int q = 0; q < PER; ++q) {
                    const float v = lds_one<T>(curb, row[q][0], te.bad, hasBad);
                    r[q] = PLAIN ? v : pick(mUndef[q], undefined_f(), v);
                }
            } else {
                float s00[PER], s01[PER], s10[PER], s11[PER];
#pragma unroll
                for (int q = 0; q < PER; ++q) {
                    if constexpr (PLAIN) {
                        lds_pair2_raw<T>(curb, rowA[q][0], rowS[q][0], s00[q], s01[q]);
                        lds_pair2_raw<T>(curb, rowA[q][STENCIL - 1], rowS[q][STENCIL - 1], s10[q], s11[q]);
                    } else {
                        lds_pair2<T>(curb, rowA[q][0], rowS[q][0], te.bad, hasBad, s00[q], s01[q]);
                        lds_pair2<T>(curb, rowA[q][STENCIL - 1], rowS[q][STENCIL - 1], te.bad, hasBad, s10[q], s11[q]);
                    }
                }
#pragma unroll
                for (int q = 0; q < PER; ++q) {
                    const BilinearForms b = bilinear_forms(s00[q], s01[q], s10[q], s11[q], xf[q], yf[q]);
                    r[q] = b.inter;
                    if constexpr (PLAIN) {  // interior cell: undefined iff one of the four is the fill value (mifi_bad2nanf, then NaN spreads)
                        // (the stored elements are integers, exact in float, and so is a fill value that can occur among them: the
                        // product of the four differences is zero iff one element is the fill value -- one comparison and one
                        // selection per output instead of four of each; without a fill value the product is NaN and never zero)
                        const float anyBad = ((s00[q] - badCmp) * (s01[q] - badCmp)) * ((s10[q] - badCmp) * (s11[q] - badCmp));
                        r[q] = (anyBad == 0.f) ? undefined_f() : b.inter;
                    }
                    if constexpr (!PLAIN) {
                        r[q] = pick(mNnx[q], pick(mNny[q], s00[q], b.liny), pick(mNny[q], b.top, b.inter));
                        r[q] = pick(mUndef[q], undefined_f(), r[q]);
                    }
                }
            }
            store_pair<T, PAIR>(ro, cellOff[0], cellOff[1], r[0], r[1], fillT);
            store_pair<T, PAIR>(ro, cellOff[2], cellOff[3], r[2], r[3], fillT);
        });
    });
}

}  // namespace

// the plan's staged form for slices of elemBytes-byte elements (2 or 1), built on first use; nullptr: none (the caller takes
// the first staged form or the gather kernels)
const Staged2Plan* staged2_typed_form(const fimex_amd_regrid_plan& plan, uint32_t elemBytes, hipStream_t stream)
{
    if (plan.kind != PlanKind::Nearest && plan.kind != PlanKind::Bilinear) return nullptr;
    if ((plan.inX * plan.inY * elemBytes) % 4 != 0) return nullptr;  // slices start on 4-byte boundaries (LDS-DMA)
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
// 1- and 2-byte integers, nearest and bilinear, through the second staged form.  false: not applicable, the caller goes on.
bool launch_staged2_apply_typed(const fimex_amd_regrid_plan& plan, const void* d_in, int cdmType, size_t nz, double badValue, void* d_out,
                                hipStream_t stream)
{
    if (!(cdmType == FIMEX_AMD_CDM_CHAR || cdmType == FIMEX_AMD_CDM_UCHAR || cdmType == FIMEX_AMD_CDM_SHORT || cdmType == FIMEX_AMD_CDM_USHORT))
        return false;
    const uint32_t eb = (cdmType == FIMEX_AMD_CDM_SHORT || cdmType == FIMEX_AMD_CDM_USHORT) ? 2u : 1u;
    if (reinterpret_cast<uintptr_t>(d_in) % 4 != 0) return false;
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
