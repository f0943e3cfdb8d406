// The pair kernel of the second LDS-staged regrid form and its launch: both components of an x/y vector (a wind pair) walk through
// one slice ring, u(z), v(z), u(z + 1), ..., and are rotated in the lane's registers before they are stored --
// CDMInterpolator::getDataSlice's vector branch (src/CDMInterpolator.cc:259-277: interpolateValues on both components, then
// CachedVectorReprojection::reprojectValues) in one launch instead of three.  Nearest and bilinear plans; the plan is the one
// staged_apply2 (staged2.hip) runs, and so are tiles, chunk lists, LDS offsets, workgroup shapes and z chunks.
#include "staged2_lane_ops.hpp"
#include "staged2_ring.hpp"

namespace fimex_amd {

namespace {

struct Staged2VectorArgs {
    Staged2Args a;  // in / out: the x component; nz and the z chunks count pairs
    const float* inV;
    float* outV;
    const double2* cs;  // (m0, m1) of the rotation matrix per output cell
};

// STENCIL: 1 nearest, 2 bilinear; NT, PER, KMAX, DEPTH as staged_apply2
template <int STENCIL, int NT, int PER, int KMAX, int DEPTH>
__global__ void __launch_bounds__(NT) staged_apply2_vector(Staged2VectorArgs va)
{
    static_assert(STENCIL == 1 || STENCIL == 2, "pairs: nearest and bilinear");
    const Staged2Args& a = va.a;
    StagedTile T;
    uint32_t z0, z1;
    if (!decode_workgroup(a, T, z0, z1)) return;
    const SliceRing<NT, KMAX, DEPTH> ring(a, T, z0, z1, va.inV, 4u);
    char* const outBaseV = reinterpret_cast<char*>(va.outV);
    // ---- per-lane plan, as staged_apply2; and the rotation of the lane's outputs, held over the z chunk (a load inside the
    // loop would count in vmcnt)
    uint32_t cellOff[PER];
    uint32_t row[PER][STENCIL];
    float xf[PER], yf[PER];
    double mc[PER], ms[PER];
    bool undef[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const uint32_t e = threadIdx.x + k * NT;
        const uint32_t ly = e / T.w, lx = e - ly * T.w;
        const uint32_t y = T.y0 + ly;
        cellOff[k] = 0xFFFFFFFFu;
        uint32_t pa = kInvalidPos;
        xf[k] = yf[k] = 0.f;
        mc[k] = ms[k] = 0;
        if (ly < a.tileH && y < a.outY) {
            const uint32_t cell = y * a.outX + T.x0 + lx;
            cellOff[k] = cell * 4u;
            pa = a.ldsA[cell];
            if (STENCIL == 2) { xf[k] = a.xf[cell]; yf[k] = a.yf[cell]; }
            const double2 m = va.cs[cell];
            mc[k] = m.x;
            ms[k] = m.y;
        }
        undef[k] = pa == kInvalidPos;  // undefined cells read LDS offset 0 and discard it
        row[k][0] = undef[k] ? 0u : (pa & 0xFFFFu) * 4u;
        if (STENCIL == 2) row[k][STENCIL - 1] = undef[k] ? 0u : (pa >> 16) * 4u;
    }
    if (T.rsv[0] != 0) {  // a gather tile: both components' stencils straight from memory
        uint32_t p[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            p[k] = (cellOff[k] != 0xFFFFFFFFu) ? a.pos[cellOff[k] / 4u] : kInvalidPos;
            undef[k] = p[k] == kInvalidPos;
            if (undef[k]) p[k] = 0;
        }
        for (uint32_t z = z0; z < z1; ++z) {
            const rsrc_t rsU = ring.in_uniform(z), roU = ring.out_uniform(z);
            const rsrc_t rsV = make_rsrc(uniform(ring.inBaseV + (size_t)z * ring.inBytes), ring.inRecords);
            const rsrc_t roV = make_rsrc(uniform(outBaseV + (size_t)z * ring.outBytes), ring.outRecords);
            auto value = [&](rsrc_t rs, int k) __attribute__((always_inline)) {
                auto ld = [&](uint32_t cell) { return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, cell * 4u, 0, 0)); };
                float r;
                if constexpr (STENCIL == 1) {
                    r = ld(p[k]);
                } else {
                    const uint32_t dx = is_nn(xf[k]) ? 0u : 1u, dy = is_nn(yf[k]) ? 0u : a.inX;  // a missing neighbour repeats the cell itself
                    r = bilinear_value(ld(p[k]), ld(p[k] + dx), ld(p[k] + dy), ld(p[k] + dx + dy), xf[k], yf[k]);
                }
                return undef[k] ? undefined_f() : r;
            };
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                float ru, rv;
                rotate_pair(value(rsU, k), value(rsV, k), mc[k], ms[k], ru, rv);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ru), roU, cellOff[k], 0, 2);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(rv), roV, cellOff[k], 0, 2);
            }
        }
        return;
    }
    if (T.nChunks == 0) {  // nothing of the source is needed: every output of the tile is undefined, in both components
        for (uint32_t z = z0; z < z1; ++z) {
            const rsrc_t roU = ring.out(z), roV = make_rsrc(outBaseV + (size_t)z * ring.outBytes, ring.outRecords);
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                __builtin_amdgcn_raw_buffer_store_b32(0x7fc00000u, roU, cellOff[k], 0, 2);
                __builtin_amdgcn_raw_buffer_store_b32(0x7fc00000u, roV, cellOff[k], 0, 2);
            }
        }
        return;
    }
    ring.wait_first();
    // the matrix is in its registers from here on: no wait for it is left to the loop, whose waits count what the loop issues
#pragma unroll
    for (int k = 0; k < PER; ++k) asm volatile("" : "+v"(mc[k]), "+v"(ms[k]));
    // plain waves and the border masks: as staged_apply2
    bool plainWave = true;
#pragma unroll
    for (int k = 0; k < PER; ++k)
        plainWave = plainWave && !undef[k] && (STENCIL != 2 || !(is_nn(xf[k]) || is_nn(yf[k])));
    plainWave = __all(plainWave) != 0;
    uint32_t mNnx[PER], mNny[PER], mUndef[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        mNnx[k] = nn_mask(xf[k]);
        mNny[k] = nn_mask(yf[k]);
        mUndef[k] = undef[k] ? 0xFFFFFFFFu : 0u;
    }
    dispatch_un<KMAX>(ring.un, plainWave, [&](auto unTag, auto plainTag) __attribute__((always_inline)) {
        constexpr bool PLAIN = decltype(plainTag)::value;
        // one component's slice out of the bytes at `curb`: the lane's PER values as staged_apply2 stores them
        auto interpolate = [&](const char* curb, float (&r)[PER]) __attribute__((always_inline)) {
            if constexpr (STENCIL == 1) {
#pragma unroll
                for (int k = 0; k < PER; ++k) {  // src/interpolation.c:869-876
                    const float v = *reinterpret_cast<const float*>(curb + row[k][0]);
                    r[k] = PLAIN ? v : pick(mUndef[k], undefined_f(), v);
                }
            } else {
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
                    r[k] = b.inter;
                    if constexpr (!PLAIN) {  // bilinear_select with bit masks: no divergent branches in the loop
                        r[k] = pick(mNnx[k], pick(mNny[k], s00[k], b.liny), pick(mNny[k], b.top, b.inter));
                        r[k] = pick(mUndef[k], undefined_f(), r[k]);
                    }
                }
            }
        };
        float u[PER];  // the u step's results wait here for the v step: with DEPTH 2 their slot is refilled meanwhile
        ring.template run_pairs<decltype(unTag)::value, 2 * PER>(
            [&](const char* curb) __attribute__((always_inline)) { interpolate(curb, u); },
            [&](uint32_t z, const char* curb) __attribute__((always_inline)) {
                float v[PER];
                interpolate(curb, v);
                const rsrc_t roU = ring.out(z), roV = make_rsrc(outBaseV + (size_t)z * ring.outBytes, ring.outRecords);
#pragma unroll
                for (int k = 0; k < PER; ++k) {  // a cell undefined in one component is NaN in both by this arithmetic alone
                    float ru, rv;
                    rotate_pair(u[k], v[k], mc[k], ms[k], ru, rv);
                    // the result stores of staged_apply2: non-temporal and written through (sc1 nt)
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ru), roU, cellOff[k], 0, 18);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(rv), roV, cellOff[k], 0, 18);
                }
            });
    });
}

template <int STENCIL, int NT, int PER, int KMAX>
void launch_one(const Staged2VectorArgs& va, dim3 grid, size_t ldsBytes, uint32_t depth, hipStream_t stream)
{
    auto go = [&](auto kernel) {
        allow_dynamic_lds(reinterpret_cast<const void*>(kernel), ldsBytes);
        kernel<<<grid, NT, ldsBytes, stream>>>(va);
    };
    depth == 3 ? go(&staged_apply2_vector<STENCIL, NT, PER, KMAX, 3>) : go(&staged_apply2_vector<STENCIL, NT, PER, KMAX, 2>);
}

// the shapes build_staged2_plan gives the 1 x 1 and 2 x 2 stencils
template <int STENCIL>
void launch_shape(const Staged2Plan& s, const Staged2VectorArgs& va, dim3 grid, hipStream_t stream)
{
    const uint32_t key = s.nt * 10000 + s.per * 100 + s.kmax;
    switch (key) {
    case 2560406: launch_one<STENCIL, 256, 4, 6>(va, grid, s.ldsBytes, s.depth, stream); break;
    case 5120406: launch_one<STENCIL, 512, 4, 6>(va, grid, s.ldsBytes, s.depth, stream); break;
    case 10240405: launch_one<STENCIL, 1024, 4, 5>(va, grid, s.ldsBytes, s.depth, stream); break;
    default: throw Error("staged2 pairs: unexpected workgroup shape");
    }
}

}  // namespace

void launch_staged2_apply_vector(const fimex_amd_regrid_plan& plan, const fimex_amd_vector_plan& vec, const float* d_u, const float* d_v, size_t nz,
                                 float* d_uOut, float* d_vOut, hipStream_t stream)
{
    FA_REQUIRE(nz <= 0xFFFFFFFFu, "too many slices");
    const Staged2Plan& s = staged2_shape_of(plan);
    Staged2VectorArgs va{staged2_args(plan, s, d_u, d_uOut, 4, nz), d_v, d_vOut, vec.cossin.get()};
    // chunks of pairs; the pair kernel keeps the tile-major order whatever the plan's float launches run (the chunk-per-XCD
    // order has not been timed on pairs)
    const dim3 grid = staged2_z_chunks(va.a, s, nz, kTileMajor, false);
    if (plan.kind == PlanKind::Nearest) launch_shape<1>(s, va, grid, stream);
    else launch_shape<2>(s, va, grid, stream);
    FA_HIP(hipGetLastError());
}

}  // namespace fimex_amd
