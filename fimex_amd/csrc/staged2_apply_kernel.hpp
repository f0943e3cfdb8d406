// The float kernel of the second LDS-staged regrid form: its TEXT, included once per kernel (no include guard).  staged2.hip makes
// staged_apply2 of it, on the slices of one array; staged2_list.hip makes staged_apply2_list, on the slices of a list of
// variables.  The two differ in where a slice lies -- the Slices policy of SliceRing, staged2_ring.hpp -- and in nothing else.
// Text and not a function template that both kernels call: as the inlined body of a shared function the array kernels came out
// with another register allocation (bilinear: 70-74 instead of 80-82 VGPRs), and they are to stay the machine code that was
// measured (profiles/staged2_list_resource_usage.md).  The including file defines, and undefines afterwards:
//   STAGED2_KERNEL      the kernel's name
//   STAGED2_SLICES      ArraySlices or ListSlices
//   STAGED2_LIST_PARAM  the parameters behind `Staged2Args a`: nothing, or `, SliceListArgs l`
//   STAGED2_LIST        the ring's list: nullptr, or &l

namespace fimex_amd {
namespace {

// STENCIL: 1 nearest, 2 bilinear, 4 bicubic; NT: threads of the workgroup; PER: outputs per lane (tile = NT * PER outputs);
// KMAX: most 16-byte chunks a lane stages per slice.
// FAST (bicubic only): the weights rounded to float and float fused multiply-adds instead of the reference's double products
// accumulated into a float (interpolation.c:1005-1019) -- not bit-identical, within 1e-5 of the stencil's magnitude (the
// tolerance BASELINE.json states), chosen per plan (FIMEX_AMD_BICUBIC_FAST).
template <int STENCIL, int NT, int PER, int KMAX, bool FAST = false, int DEPTH = 2>
__global__ void __launch_bounds__(NT) STAGED2_KERNEL(Staged2Args a STAGED2_LIST_PARAM)
{
    // a list on a FIMEX_AMD_BICUBIC_FAST plan mixes the two arithmetics, slice by slice (SliceRing::exact_slice)
    constexpr bool kMixed = FAST && STAGED2_SLICES::kList;
    StagedTile T;
    uint32_t z0, z1;
    if (!decode_workgroup(a, T, z0, z1)) return;
    const SliceRing<NT, KMAX, DEPTH, STAGED2_SLICES> ring(a, T, z0, z1, 4u, STAGED2_LIST);
    // ---- per-lane plan: outputs e = threadIdx.x + k * NT of the tile (a wave covers 64 consecutive cells of one row)
    uint32_t cellOff[PER];
    uint32_t row[PER][STENCIL];
    float xf[PER], yf[PER];
    double XM[PER][4], MY[PER][4];
    float XMf[PER][4], MYf[PER][4];
    bool undef[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const uint32_t e = threadIdx.x + k * NT;
        const uint32_t ly = e / T.w, lx = e - ly * T.w;
        const uint32_t y = T.y0 + ly;
        cellOff[k] = 0xFFFFFFFFu;
        uint32_t pa = kInvalidPos, pb = kInvalidPos;
        xf[k] = yf[k] = 0.f;
        double fx = 0, fy = 0;
        if (ly < a.tileH && y < a.outY) {
            const uint32_t cell = y * a.outX + T.x0 + lx;
            cellOff[k] = cell * 4u;
            pa = a.ldsA[cell];
            if (STENCIL == 4) { pb = a.ldsB[cell]; fx = a.xfd[cell]; fy = a.yfd[cell]; }
            else if (STENCIL == 2) { xf[k] = a.xf[cell]; yf[k] = a.yf[cell]; }
        }
        undef[k] = pa == kInvalidPos;  // undefined cells read LDS offset 0 and discard it
        row[k][0] = undef[k] ? 0u : (pa & 0xFFFFu) * 4u;
        if (STENCIL >= 2) row[k][STENCIL >= 2 ? 1 : 0] = undef[k] ? 0u : (pa >> 16) * 4u;
        if (STENCIL == 4) {
            row[k][2] = undef[k] ? 0u : (pb & 0xFFFFu) * 4u;
            row[k][3] = undef[k] ? 0u : (pb >> 16) * 4u;
            cubic_weights(fx, XM[k]);
            cubic_weights(fy, MY[k]);
#pragma unroll
            for (int j = 0; j < 4; ++j) { XMf[k][j] = (float)XM[k][j]; MYf[k][j] = (float)MY[k][j]; }
        }
    }
    if (T.rsv[0] != 0) {
        // A tile whose footprint does not fit a slot even at the smallest width (an outlier among its positions: a grid
        // that wraps around the date line, isolated special points) reads its stencils straight from memory, like the
        // gather kernels of gather.hip; every other tile of the plan stays staged.
        uint32_t p[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            p[k] = (cellOff[k] != 0xFFFFFFFFu) ? a.pos[cellOff[k] / 4u] : kInvalidPos;
            undef[k] = p[k] == kInvalidPos;
            if (undef[k]) p[k] = 0;
        }
        for (uint32_t z = z0; z < z1; ++z) {
            const rsrc_t rs = ring.in_uniform(z), ro = ring.out_uniform(z);
            auto ld = [&](uint32_t cell) { return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, cell * 4u, 0, 0)); };
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                float r;
                if constexpr (STENCIL == 1) {
                    r = ld(p[k]);
                } else if constexpr (STENCIL == 2) {
                    const uint32_t dx = is_nn(xf[k]) ? 0u : 1u, dy = is_nn(yf[k]) ? 0u : a.inX;  // a missing neighbour repeats the cell itself
                    r = bilinear_value(ld(p[k]), ld(p[k] + dx), ld(p[k] + dy), ld(p[k] + dx + dy), xf[k], yf[k]);
                } else {
                    float f[4][4];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int j = 0; j < 4; ++j) f[q][j] = ld(p[k] + q * a.inX + j);
                    if constexpr (FAST) {
                      if (kMixed && ring.exact_slice()) {
                        r = bicubic_point(f, XM[k], MY[k]);
                      } else {
                        float acc = 0;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            float xmf = 0;
#pragma unroll
                            for (int j = 0; j < 4; ++j) xmf = __builtin_fmaf(XMf[k][j], f[q][j], xmf);
                            acc = __builtin_fmaf(xmf, MYf[k][q], acc);
                        }
                        r = acc;
                      }
                    } else {
                        r = bicubic_point(f, XM[k], MY[k]);
                    }
                }
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(undef[k] ? undefined_f() : r), ro, cellOff[k], 0, 2);
            }
            ring.slice_done();
        }
        return;
    }
    if (T.nChunks == 0) {  // nothing of the source is needed: every output of the tile is undefined
        for (uint32_t z = z0; z < z1; ++z) {
            const rsrc_t ro = ring.out(z);
#pragma unroll
            for (int k = 0; k < PER; ++k) __builtin_amdgcn_raw_buffer_store_b32(0x7fc00000u, ro, cellOff[k], 0, 2);
            ring.slice_done();
        }
        return;
    }
    ring.wait_first();
    // A wave whose outputs are all interior cells of the source (nothing undefined, no border branch: nearly every wave)
    // runs a copy of the loop without the selections between the border forms.  (Vote and masks are written out in both
    // kernels: as a shared function they cost 4-12 VGPRs and a wave per SIMD, profiles/staged2_split_resource_usage.md.)
    bool plainWave = true;
#pragma unroll
    for (int k = 0; k < PER; ++k)
        plainWave = plainWave && !undef[k] && (STENCIL != 2 || !(is_nn(xf[k]) || is_nn(yf[k])));
    plainWave = __all(plainWave) != 0;
    // selection masks of the border forms (interpolation.c:903-948) for the other copy: all ones / all zeros per output
    uint32_t mNnx[PER], mNny[PER], mUndef[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        mNnx[k] = nn_mask(xf[k]);
        mNny[k] = nn_mask(yf[k]);
        mUndef[k] = undef[k] ? 0xFFFFFFFFu : 0u;
    }
    dispatch_un<KMAX>(ring.un, plainWave, [&](auto unTag, auto plainTag) __attribute__((always_inline)) {
        constexpr bool PLAIN = decltype(plainTag)::value;
        ring.template run<decltype(unTag)::value, PER>([&](uint32_t z, const char* curb) __attribute__((always_inline)) {
            const rsrc_t ro = ring.out(z);
            if constexpr (STENCIL == 1) {
                float v[PER];
    #pragma unroll
                for (int k = 0; k < PER; ++k) v[k] = *reinterpret_cast<const float*>(curb + row[k][0]);
    #pragma unroll
                for (int k = 0; k < PER; ++k)  // src/interpolation.c:869-876
                    store_result(__float_as_uint(PLAIN ? v[k] : pick(mUndef[k], undefined_f(), v[k])), ro, cellOff[k], a.flags);
            } else if constexpr (STENCIL == 2) {
                float s00[PER], s01[PER], s10[PER], s11[PER];
    #pragma unroll
                for (int k = 0; k < PER; ++k) {  // all stencil reads first: 2 x ds_read2_b32 per output, no waits in between
                    const float* pa = reinterpret_cast<const float*>(curb + row[k][0]);
                    const float* pb = reinterpret_cast<const float*>(curb + row[k][1]);
                    s00[k] = pa[0]; s01[k] = pa[1]; s10[k] = pb[0]; s11[k] = pb[1];
                }
    #pragma unroll
                for (int k = 0; k < PER; ++k) {
                    const BilinearForms b = bilinear_forms(s00[k], s01[k], s10[k], s11[k], xf[k], yf[k]);
                    float r = b.inter;
                    if constexpr (!PLAIN) {  // bilinear_select with bit masks: no divergent branches in the loop
                        r = pick(mNnx[k], pick(mNny[k], s00[k], b.liny), pick(mNny[k], b.top, b.inter));
                        r = pick(mUndef[k], undefined_f(), r);
                    }
                    store_result(__float_as_uint(r), ro, cellOff[k], a.flags);
                }
            } else if constexpr (FAST) {
              if (kMixed && ring.exact_slice()) {  // the reference's arithmetic for this slice: the last branch's loop
    #pragma unroll
                for (int k = 0; k < PER; ++k) {
                    float f[4][4];
    #pragma unroll
                    for (int r = 0; r < 4; ++r) {
    #pragma unroll
                        for (int j = 0; j < 4; ++j) f[r][j] = *reinterpret_cast<const float*>(curb + row[k][r] + 4 * j);
                    }
                    const float acc = bicubic_point(f, XM[k], MY[k]);
                    store_result(__float_as_uint(PLAIN ? acc : pick(mUndef[k], undefined_f(), acc)), ro, cellOff[k], a.flags);
                }
              } else {
                // float arithmetic: the stencil's columns are summed first, two at a time in packed FMAs -- the two floats a
                // ds_read2_b32 delivers are one operand, the row's weight is the other (both halves) -- then the four column sums
                // meet the x weights: 11 packed / scalar instructions per output instead of 20 FMAs.  The launch is bound by its
                // instructions (LDS reads and arithmetic: 1.9 of 2.5 ms with the memory instructions switched off,
                // profiles/r03_ablate_bicubic_fast.log), so this is where its time is.
                using v2f = float __attribute__((ext_vector_type(2)));
                // (the four floats of a stencil row are read as two ds_read2_b32: 8-byte LDS reads at 4-byte addresses work on this
                // hardware but take five times as long, scripts/calib/lds_unaligned.hip, profiles/calib/r03_lds_unaligned.jsonl)
    #pragma unroll
                for (int k = 0; k < PER; ++k) {
                    v2f c01 = {0.f, 0.f}, c23 = {0.f, 0.f};
    #pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float* fr = reinterpret_cast<const float*>(curb + row[k][r]);
                        const v2f f01 = {fr[0], fr[1]};
                        const v2f f23 = {fr[2], fr[3]};
                        const v2f myPair = {MYf[k][r & 2], MYf[k][(r & 2) + 1]};  // (a register pair; the packed FMA takes one half twice)
                        const v2f my = (r & 1) ? __builtin_shufflevector(myPair, myPair, 1, 1) : __builtin_shufflevector(myPair, myPair, 0, 0);
                        c01 = __builtin_elementwise_fma(f01, my, c01);
                        c23 = __builtin_elementwise_fma(f23, my, c23);
                    }
                    const v2f x01 = {XMf[k][0], XMf[k][1]}, x23 = {XMf[k][2], XMf[k][3]};
                    const v2f p = __builtin_elementwise_fma(x23, c23, x01 * c01);
                    const float acc = p.x + p.y;
                    store_result(__float_as_uint(PLAIN ? acc : pick(mUndef[k], undefined_f(), acc)), ro, cellOff[k], a.flags);
                }
              }
            } else {
    #pragma unroll
                for (int k = 0; k < PER; ++k) {
                    float f[4][4];
    #pragma unroll
                    for (int r = 0; r < 4; ++r) {
    #pragma unroll
                        for (int j = 0; j < 4; ++j) f[r][j] = *reinterpret_cast<const float*>(curb + row[k][r] + 4 * j);
                    }
                    const float acc = bicubic_point(f, XM[k], MY[k]);
                    store_result(__float_as_uint(PLAIN ? acc : pick(mUndef[k], undefined_f(), acc)), ro, cellOff[k], a.flags);
                }
            }
        });
    });
}

}  // namespace
}  // namespace fimex_amd
