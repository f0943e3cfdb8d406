// The pair kernel of the second LDS-staged regrid form on the STORED type of a vector pair, and its launch: both components of an
// x/y vector whose slices are 2-byte integers (packed winds) walk through one slice ring, u(z), v(z), u(z + 1), ..., are converted,
// interpolated and rotated in the lane's registers and leave in their stored type -- CDMInterpolator::getDataSlice's vector branch
// (src/CDMInterpolator.cc:251-285 without pre- and post-processes: data2InterpolationArray and interpolateValues on both
// components, CachedVectorReprojection::reprojectValues, interpolationArray2Data on both) in one launch instead of five, with no
// float copy of a slice.  The lane layout, the element reads, the arithmetic and the stores are staged_apply2_typed's
// (staged2_typed.hip), the ring of pairs and the rotation staged_apply2_vector's (staged2_vector.hip); the plan form is the
// stored-type form of staged2_typed.hip as it is.  Nearest and bilinear plans, short and unsigned short.
#include "staged2_lane_ops.hpp"
#include "staged2_ring.hpp"

namespace fimex_amd {

namespace {

struct PairEdge {
    float badU, badV;        // the components' fill values narrowed to float (mifi_bad2nanf's argument)
    uint32_t hasBadU, hasBadV;
    double fillU, fillV;     // NaN -> this (interpolationArray2Data), per component
};

struct Staged2VectorTypedArgs {
    Staged2Args a;  // in / out: the x component; nz and the z chunks count pairs
    const void* inV;
    void* outV;
    const double2* cs;  // (m0, m1) of the rotation matrix per output cell
    PairEdge e;
};

// STENCIL 1 (nearest) or 2 (bilinear); NT threads, 4 outputs per lane (two pairs of neighbours); KMAX 16-byte chunks per lane and
// slice; PAIR: the row length and both slice starts allow aligned stores of two results.  Every shape's LDS holds it at four waves
// per SIMD (two workgroups of 512 threads, four of 256, one of 1024 per CU): the compiler is told so, 128 VGPRs are the budget
// (profiles/staged2_vector_typed_resource_usage.md)
template <int STENCIL, int NT, int KMAX, typename T, bool PAIR, int DEPTH>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4))) staged_apply2_vector_typed(Staged2VectorTypedArgs va)
{
    static_assert(STENCIL == 1 || STENCIL == 2, "pairs: nearest and bilinear");
    static_assert(sizeof(T) == 2, "pairs on stored types: 2-byte elements");
    constexpr uint32_t EB = sizeof(T);
    constexpr int PER = 4;
    const Staged2Args& a = va.a;
    const PairEdge& e = va.e;
    StagedTile T_;
    uint32_t z0, z1;
    if (!decode_workgroup(a, T_, z0, z1)) return;
    const SliceRing<NT, KMAX, DEPTH> ring(a, T_, z0, z1, va.inV, EB);
    char* const outBaseV = reinterpret_cast<char*>(va.outV);
    const bool hasBadU = e.hasBadU != 0, hasBadV = e.hasBadV != 0;
    const T fillU = static_cast<T>(e.fillU), fillV = static_cast<T>(e.fillV);  // ScaleValue's newFill_ (include/fimex/Utils.h:456)
    // per-lane plan, as staged_apply2_typed: output q = 2 * p + h is cell 2 * threadIdx.x + h + p * 2 * NT of the tile; and the
    // rotation of the lane's outputs, held over the z chunk (a load inside the loop would count in vmcnt)
    uint32_t cellOff[PER];       // byte offset inside a typed output slice, ~0u = not mine
    uint32_t row[PER][STENCIL];  // byte offsets of the stencil rows in the staged image
    uint32_t cellIdx[PER];
    float xf[PER], yf[PER];
    double mc[PER], ms[PER];
    bool undef[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const uint32_t el = 2u * threadIdx.x + (uint32_t)(q & 1) + (uint32_t)(q >> 1) * 2u * NT;
        const uint32_t ly = el / T_.w, lx = el - ly * T_.w;
        const uint32_t y = T_.y0 + ly;
        cellOff[q] = 0xFFFFFFFFu;
        cellIdx[q] = 0xFFFFFFFFu;
        uint32_t pa = kInvalidPos;
        xf[q] = yf[q] = 0.f;
        mc[q] = ms[q] = 0;
        if (ly < a.tileH && y < a.outY) {
            const uint32_t cell = y * a.outX + T_.x0 + lx;
            cellIdx[q] = cell;
            cellOff[q] = cell * EB;
            pa = a.ldsA[cell];
            if (STENCIL == 2) { xf[q] = a.xf[cell]; yf[q] = a.yf[cell]; }
            const double2 m = va.cs[cell];
            mc[q] = m.x;
            ms[q] = m.y;
        }
        undef[q] = pa == kInvalidPos;
        row[q][0] = undef[q] ? 0u : (pa & 0xFFFFu) * EB;
        if (STENCIL == 2) row[q][STENCIL - 1] = undef[q] ? 0u : (pa >> 16) * EB;
    }
    // the rotation of the lane's outputs [Q0, Q0 + QN) (whole pairs of neighbours) and the stores of both components; a cell
    // undefined in one component is NaN in both by this arithmetic alone
    auto rotate_store = [&](auto q0Tag, auto qnTag, rsrc_t roU, rsrc_t roV, const float (&u)[PER], const float (&v)[PER]) __attribute__((always_inline)) {
        constexpr int Q0 = decltype(q0Tag)::value, QN = decltype(qnTag)::value;
        float ru[PER], rv[PER];
#pragma unroll
        for (int q = Q0; q < Q0 + QN; ++q) rotate_pair(u[q], v[q], mc[q], ms[q], ru[q], rv[q]);
#pragma unroll
        for (int q = Q0; q < Q0 + QN; q += 2) store_pair<T, PAIR>(roU, cellOff[q], cellOff[q + 1], ru[q], ru[q + 1], fillU);
#pragma unroll
        for (int q = Q0; q < Q0 + QN; q += 2) store_pair<T, PAIR>(roV, cellOff[q], cellOff[q + 1], rv[q], rv[q + 1], fillV);
    };
    constexpr std::integral_constant<int, 0> kFirst{};
    constexpr std::integral_constant<int, PER> kAll{};
    if (T_.rsv[0] != 0) {  // a gather tile (see staged_apply2): both components' stencils straight from memory, element by element
        uint32_t p[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            p[q] = (cellIdx[q] != 0xFFFFFFFFu) ? a.pos[cellIdx[q]] : kInvalidPos;
            undef[q] = p[q] == kInvalidPos;
            if (undef[q]) p[q] = 0;
        }
        for (uint32_t z = z0; z < z1; ++z) {
            const rsrc_t rsU = ring.in_uniform(z), roU = ring.out_uniform(z);
            const rsrc_t rsV = make_rsrc(uniform(ring.inBaseV + (size_t)z * ring.inBytes), ring.inRecords);
            const rsrc_t roV = make_rsrc(uniform(outBaseV + (size_t)z * ring.outBytes), ring.outRecords);
            auto values = [&](rsrc_t rs, float bad, bool hasBad, float (&r)[PER]) __attribute__((always_inline)) {
                auto ld = [&](uint32_t cell) { return as_float_nan((T)__builtin_amdgcn_raw_buffer_load_b16(rs, cell * 2u, 0, 0), bad, hasBad); };
#pragma unroll
                for (int q = 0; q < PER; ++q) {
                    if constexpr (STENCIL == 1) {
                        r[q] = ld(p[q]);
                    } else {
                        const uint32_t dx = is_nn(xf[q]) ? 0u : 1u, dy = is_nn(yf[q]) ? 0u : a.inX;  // a missing neighbour repeats the cell itself
                        r[q] = bilinear_value(ld(p[q]), ld(p[q] + dx), ld(p[q] + dy), ld(p[q] + dx + dy), xf[q], yf[q]);
                    }
                    if (undef[q]) r[q] = undefined_f();
                }
            };
            float u[PER], v[PER];
            values(rsU, e.badU, hasBadU, u);
            values(rsV, e.badV, hasBadV, v);
            rotate_store(kFirst, kAll, roU, roV, u, v);
        }
        return;
    }
    if (T_.nChunks == 0) {  // nothing of the source is needed: every output of the tile is undefined, in both components
        const float nan4[PER] = {undefined_f(), undefined_f(), undefined_f(), undefined_f()};
        for (uint32_t z = z0; z < z1; ++z)
            rotate_store(kFirst, kAll, ring.out(z), make_rsrc(outBaseV + (size_t)z * ring.outBytes, ring.outRecords), nan4, nan4);
        return;
    }
    ring.wait_first();
    // the matrix is in its registers from here on: no wait for it is left to the loop, whose waits count what the loop issues
#pragma unroll
    for (int q = 0; q < PER; ++q) asm volatile("" : "+v"(mc[q]), "+v"(ms[q]));
    constexpr int NST = PAIR ? 2 : 4;  // store instructions a lane issues per slice and component
    // With single stores the bilinear loop would need more than the 128 registers that two 512-thread workgroups per CU (and one of
    // 1024 threads) leave a lane -- 148 with all four outputs in flight, as the parent kernels have them: it takes its outputs in
    // two halves of one pair each, which the scheduler may not interleave.  The stores per step stay 2 * NST.
    constexpr int HALVES = (STENCIL == 2 && !PAIR) ? 2 : 1, QN = PER / HALVES;
    constexpr std::integral_constant<int, QN> kHalf{};
    constexpr std::integral_constant<int, PER - QN> kSecond{};
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
    // (the loop in halves keeps `row` alone and splits it at every read, two instructions that must stay in the loop: eight
    // registers fewer)
    auto row_operands = [&](int q, int i, uint32_t& aligned, uint32_t& shift) __attribute__((always_inline)) {
        if constexpr (HALVES == 2) {
            asm volatile("v_and_b32 %0, -4, %2\n\tv_lshlrev_b32 %1, 3, %2" : "=&v"(aligned), "=v"(shift) : "v"(row[q][i]));
        } else {
            aligned = rowA[q][i];
            shift = rowS[q][i];
        }
    };
    // no fill value: comparisons with NaN never hold, the loops need no separate test
    const float badCmpU = hasBadU ? e.badU : undefined_f(), badCmpV = hasBadV ? e.badV : undefined_f();
    dispatch_un<KMAX>(ring.un, plainWave, [&](auto unTag, auto plainTag) __attribute__((always_inline)) {
        constexpr bool PLAIN = decltype(plainTag)::value;
        // one component's slice out of the bytes at `curb`, with that component's fill value: the lane's four values as
        // staged_apply2_typed rounds and stores them
        auto interpolate = [&](auto q0Tag, const char* curb, float bad, bool hasBad, float badCmp, float (&r)[PER]) __attribute__((always_inline)) {
            constexpr int Q0 = decltype(q0Tag)::value;
            if constexpr (STENCIL == 1) {
#pragma unroll
                for (int q = Q0; q < Q0 + QN; ++q) {
                    const float v = lds_one<T>(curb, row[q][0], bad, hasBad);
                    r[q] = PLAIN ? v : pick(mUndef[q], undefined_f(), v);
                }
            } else {
                float s00[PER], s01[PER], s10[PER], s11[PER];
#pragma unroll
                for (int q = Q0; q < Q0 + QN; ++q) {
                    uint32_t a0, sh0, a1, sh1;
                    row_operands(q, 0, a0, sh0);
                    row_operands(q, STENCIL - 1, a1, sh1);
                    if constexpr (PLAIN) {
                        lds_pair2_raw<T>(curb, a0, sh0, s00[q], s01[q]);
                        lds_pair2_raw<T>(curb, a1, sh1, s10[q], s11[q]);
                    } else {
                        lds_pair2<T>(curb, a0, sh0, bad, hasBad, s00[q], s01[q]);
                        lds_pair2<T>(curb, a1, sh1, bad, hasBad, s10[q], s11[q]);
                    }
                }
#pragma unroll
                for (int q = Q0; q < Q0 + QN; ++q) {
                    const BilinearForms b = bilinear_forms(s00[q], s01[q], s10[q], s11[q], xf[q], yf[q]);
                    r[q] = b.inter;
                    if constexpr (PLAIN) {  // interior cell: undefined iff one of the four is the fill value (see staged_apply2_typed)
                        const float anyBad = ((s00[q] - badCmp) * (s01[q] - badCmp)) * ((s10[q] - badCmp) * (s11[q] - badCmp));
                        r[q] = (anyBad == 0.f) ? undefined_f() : b.inter;
                    }
                    if constexpr (!PLAIN) {
                        r[q] = pick(mNnx[q], pick(mNny[q], s00[q], b.liny), pick(mNny[q], b.top, b.inter));
                        r[q] = pick(mUndef[q], undefined_f(), r[q]);
                    }
                }
            }
        };
        float u[PER];  // the u step's results wait here for the v step: with DEPTH 2 their slot is refilled meanwhile
        ring.template run_pairs<decltype(unTag)::value, 2 * NST>(
            [&](const char* curb) __attribute__((always_inline)) {
                interpolate(kFirst, curb, e.badU, hasBadU, badCmpU, u);
                if constexpr (HALVES == 2) {
                    __builtin_amdgcn_sched_barrier(0);
                    interpolate(kSecond, curb, e.badU, hasBadU, badCmpU, u);
                }
            },
            [&](uint32_t z, const char* curb) __attribute__((always_inline)) {
                const rsrc_t roU = ring.out(z), roV = make_rsrc(outBaseV + (size_t)z * ring.outBytes, ring.outRecords);
                float v[PER];
                interpolate(kFirst, curb, e.badV, hasBadV, badCmpV, v);
                rotate_store(kFirst, kHalf, roU, roV, u, v);
                if constexpr (HALVES == 2) {
                    __builtin_amdgcn_sched_barrier(0);
                    interpolate(kSecond, curb, e.badV, hasBadV, badCmpV, v);
                    rotate_store(kSecond, kHalf, roU, roV, u, v);
                }
            });
    });
}

template <int STENCIL, typename T>
void launch_shape(const Staged2Plan& s, const Staged2VectorTypedArgs& va, bool pair, dim3 grid, hipStream_t stream)
{
    auto go = [&](auto kernel, int nt) {
        allow_dynamic_lds(reinterpret_cast<const void*>(kernel), s.ldsBytes);
        kernel<<<grid, nt, s.ldsBytes, stream>>>(va);
    };
    // the shapes staged2_typed_form gives: 512 threads with two or three slots, 256 and 1024 threads with two
    if (s.nt == 512 && s.depth == 3) {
        pair ? go(&staged_apply2_vector_typed<STENCIL, 512, 6, T, true, 3>, 512) : go(&staged_apply2_vector_typed<STENCIL, 512, 6, T, false, 3>, 512);
        return;
    }
    switch (s.nt) {
    case 256: pair ? go(&staged_apply2_vector_typed<STENCIL, 256, 6, T, true, 2>, 256) : go(&staged_apply2_vector_typed<STENCIL, 256, 6, T, false, 2>, 256); break;
    case 512: pair ? go(&staged_apply2_vector_typed<STENCIL, 512, 6, T, true, 2>, 512) : go(&staged_apply2_vector_typed<STENCIL, 512, 6, T, false, 2>, 512); break;
    case 1024: pair ? go(&staged_apply2_vector_typed<STENCIL, 1024, 5, T, true, 2>, 1024) : go(&staged_apply2_vector_typed<STENCIL, 1024, 5, T, false, 2>, 1024); break;
    default: throw Error("staged2 typed pairs: unexpected workgroup shape");
    }
}

}  // namespace

// false: the plan has no 2-byte form (the caller takes the chain around the float pair entry), nothing launched
bool launch_staged2_apply_vector_typed(const fimex_amd_regrid_plan& plan, const fimex_amd_vector_plan& vec, const void* d_u, const void* d_v,
                                       int cdmType, double uBad, double vBad, size_t nz, void* d_uOut, void* d_vOut, hipStream_t stream)
{
    FA_REQUIRE(dispatch::staged_elem_bytes(cdmType) == 2 && aligned4(d_u) && aligned4(d_v) && nz <= 0xFFFFFFFFu,
               "staged2 typed pairs: not a call of this kernel (vector_typed_fused, backward_dispatch.hpp)");
    const Staged2Plan* form = staged2_typed_form(plan, 2, stream);
    if (!form) return false;
    const Staged2Plan& s = *form;
    Staged2VectorTypedArgs va{staged2_args(plan, s, d_u, d_uOut, 2, nz), d_v, d_vOut, vec.cossin.get(), PairEdge{}};
    // z chunks as launch_staged2_apply_typed makes them, of pairs
    const uint32_t n = typed_z_chunk_count(nz, (uint32_t)tuning("STAGE2T_ZPB", 50));
    set_z_chunks(va.a, even_z_split(nz, n), true);
    va.e.badU = (float)uBad;
    va.e.badV = (float)vBad;
    va.e.hasBadU = !(va.e.badU != va.e.badU);
    va.e.hasBadV = !(va.e.badV != va.e.badV);
    va.e.fillU = uBad;
    va.e.fillV = vBad;
    // two results per store where the row length and both slice starts allow aligned 4-byte stores
    const bool pair = plan.outX % 2 == 0 && reinterpret_cast<uintptr_t>(d_uOut) % 4 == 0 && reinterpret_cast<uintptr_t>(d_vOut) % 4 == 0 &&
                      tuning("STAGE2T_PAIR", 1) != 0;
    const dim3 grid(s.gridX * n, 1, 1);
    const bool nearest = plan.kind == PlanKind::Nearest;
    if (cdmType == FIMEX_AMD_CDM_SHORT) nearest ? launch_shape<1, short>(s, va, pair, grid, stream) : launch_shape<2, short>(s, va, pair, grid, stream);
    else nearest ? launch_shape<1, unsigned short>(s, va, pair, grid, stream) : launch_shape<2, unsigned short>(s, va, pair, grid, stream);
    FA_HIP(hipGetLastError());
    return true;
}

}  // namespace fimex_amd
