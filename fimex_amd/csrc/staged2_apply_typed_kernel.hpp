// The stored-type kernel of the second LDS-staged regrid form: its TEXT, included once per kernel (no include guard), for the
// reason staged2_apply_kernel.hpp gives.  staged2_typed.hip makes staged_apply2_typed of it, staged2_list_typed.hip
// staged_apply2_list_typed.  The including file defines, and undefines afterwards:
//   STAGED2_KERNEL      the kernel's name
//   STAGED2_SLICES      ArraySlices or ListSlices
//   STAGED2_LIST_PARAM  the parameters behind `Staged2Args a, TypedEdge te`: nothing, or `, SliceListArgs l, TypedListEdge edges`
//   STAGED2_LIST        the ring's list: nullptr, or &l
//   STAGED2_EDGES       the variables' fill values: a null pointer of TypedListEdge, or &edges

namespace fimex_amd {
namespace {

// STENCIL 1 (nearest) or 2 (bilinear); NT threads, 4 outputs per lane (two pairs); KMAX 16-byte chunks per lane and slice
// PAIR: the row length and the slice start allow aligned stores of two results
// In the list form the fill value and what follows from it belong to the variable of the slice in work and are looked up per
// slice in `edges`; in the array form `te` holds for every slice.
template <int STENCIL, int NT, int KMAX, typename T, bool PAIR, int DEPTH = 2>
__global__ void __launch_bounds__(NT) STAGED2_KERNEL(Staged2Args a, TypedEdge te STAGED2_LIST_PARAM)
{
    static_assert(STENCIL == 1 || STENCIL == 2, "stored types: nearest and bilinear");
    constexpr uint32_t EB = sizeof(T);
    constexpr int PER = 4;
    StagedTile T_;
    uint32_t z0, z1;
    if (!decode_workgroup(a, T_, z0, z1)) return;
    const SliceRing<NT, KMAX, DEPTH, STAGED2_SLICES> ring(a, T_, z0, z1, EB, STAGED2_LIST);
    bool hasBad = te.hasBad != 0;
    T fillT = static_cast<T>(te.fillOut);  // ScaleValue's newFill_ (include/fimex/Utils.h:456)
    float bad = te.bad, badCmp;
    // list form, at the head of every slice: the same four of the slice's variable (wave-uniform: the cursor is)
    auto slice_edge = [&]() __attribute__((always_inline)) {
        if constexpr (STAGED2_SLICES::kList) {
            const uint32_t v = ring.variable();
            bad = STAGED2_EDGES->bad[v];
            hasBad = !(bad != bad);
            fillT = static_cast<T>(STAGED2_EDGES->fillOut[v]);
            badCmp = hasBad ? bad : undefined_f();
        }
    };
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
        // gather tile (see staged_apply2_body): stencils straight from memory, element by element
        uint32_t p[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            p[q] = (cellIdx[q] != 0xFFFFFFFFu) ? a.pos[cellIdx[q]] : kInvalidPos;
            undef[q] = p[q] == kInvalidPos;
            if (undef[q]) p[q] = 0;
        }
        for (uint32_t z = z0; z < z1; ++z) {
            slice_edge();
            const rsrc_t rs = ring.in_uniform(z), ro = ring.out_uniform(z);
            auto ld = [&](uint32_t cell) {
                if constexpr (EB == 2) return as_float_nan((T)__builtin_amdgcn_raw_buffer_load_b16(rs, cell * 2u, 0, 0), bad, hasBad);
                else return as_float_nan((T)__builtin_amdgcn_raw_buffer_load_b8(rs, cell, 0, 0), bad, hasBad);
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
            ring.slice_done();
        }
        return;
    }
    if (T_.nChunks == 0) {  // every output of the tile is undefined
        for (uint32_t z = z0; z < z1; ++z) {
            slice_edge();
            const rsrc_t ro = ring.out(z);
            store_pair<T, PAIR>(ro, cellOff[0], cellOff[1], undefined_f(), undefined_f(), fillT);
            store_pair<T, PAIR>(ro, cellOff[2], cellOff[3], undefined_f(), undefined_f(), fillT);
            ring.slice_done();
        }
        return;
    }
    ring.wait_first();
    constexpr int NST = PAIR ? 2 : 4;  // store instructions a lane issues per slice
    // plain waves and the masks of the border forms: as in staged_apply2_body
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
    badCmp = hasBad ? bad : undefined_f();
    dispatch_un<KMAX>(ring.un, plainWave, [&](auto unTag, auto plainTag) __attribute__((always_inline)) {
        constexpr bool PLAIN = decltype(plainTag)::value;
        ring.template run<decltype(unTag)::value, NST>([&](uint32_t z, const char* curb) __attribute__((always_inline)) {
            slice_edge();
            const rsrc_t ro = ring.out(z);
            float r[PER];
            if constexpr (STENCIL == 1) {
#pragma unroll
                for (int q = 0; q < PER; ++q) {
                    const float v = lds_one<T>(curb, row[q][0], bad, hasBad);
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
                        lds_pair2<T>(curb, rowA[q][0], rowS[q][0], bad, hasBad, s00[q], s01[q]);
                        lds_pair2<T>(curb, rowA[q][STENCIL - 1], rowS[q][STENCIL - 1], bad, hasBad, s10[q], s11[q]);
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
}  // namespace fimex_amd
