// Host shim of fimex_amd/csrc/stencil_math.hpp for tests/test_stencil_math_host.py: the header the backward kernels compile,
// evaluated on the CPU the way the kernels use it -- classify, encode the plan entry, decode it (decode_entry, the decoder the
// gather kernels compile), gather the stencil, combine.  Built for the host only by fimex_amd/build.py (hipcc --cuda-host-only -ffp-contract=off); needs no GPU.
#include "stencil_math.hpp"

using namespace fimex_amd;

namespace {

enum { kInterior = 0, kLinearX = 1, kLinearY = 2, kNearestBoth = 3, kUndefined = 4, kEntryDisagrees = -1 };

bool same_need(const CellNeed& a, const CellNeed& b)
{
    return a.valid == b.valid && (!a.valid || (a.xa == b.xa && a.xb == b.xb && a.ya == b.ya && a.yb == b.yb));
}

// field [nz][iy][ix], points px / py [n] -> out [n][nz], cls [n]
template <int STENCIL>
void eval(const float* field, int64_t ix, int64_t iy, int64_t nz, const double* px, const double* py, int64_t n, float* out, int* cls)
{
    for (int64_t p = 0; p < n; ++p) {
        const CellNeed c = classify<STENCIL>(px[p], py[p], ix, iy);
        // the plan entry as the classify kernels write it ...
        const uint32_t pos = encode_pos(c, ix);
        const float xf = STENCIL == 2 ? encode_frac_bilinear(c, c.xa == c.xb, px[p]) : 0.f;
        const float yf = STENCIL == 2 ? encode_frac_bilinear(c, c.ya == c.yb, py[p]) : 0.f;
        // ... and as the tile scans and the gather kernels read it (the decoder of gather_entry.hpp, cell steps instead of byte steps)
        const CellNeed need = entry_need<STENCIL>(pos, xf, yf, ix);
        using frac = frac_t<STENCIL>;
        const StencilEntry<STENCIL> e = decode_entry<STENCIL>(pos, STENCIL == 4 ? (frac)encode_frac_bicubic(c, px[p]) : (frac)xf,
                                                              STENCIL == 4 ? (frac)encode_frac_bicubic(c, py[p]) : (frac)yf, (uint32_t)ix);
        if (!same_need(c, need)) cls[p] = kEntryDisagrees;
        else if (pos == kInvalidPos) cls[p] = kUndefined;
        else cls[p] = STENCIL == 2 ? (is_nn(xf) ? (is_nn(yf) ? kNearestBoth : kLinearY) : (is_nn(yf) ? kLinearX : kInterior)) : kInterior;
        for (int64_t z = 0; z < nz; ++z) {
            const float* s = field + z * ix * iy;
            float taps[STENCIL][STENCIL];
            for (int i = 0; i < STENCIL; ++i)
                for (int j = 0; j < STENCIL; ++j) taps[i][j] = e.valid ? s[e.first + i * e.dy + j * e.dx] : 0.f;  // undefined: loads dropped
            out[p * nz + z] = e.valid ? e.combine(taps) : undefined_f();
        }
    }
}

}  // namespace

#define STENCIL_ARGS const float* field, int64_t ix, int64_t iy, int64_t nz, const double* px, const double* py, int64_t n, float* out, int* cls
extern "C" void stencil_math_nearest(STENCIL_ARGS) { eval<1>(field, ix, iy, nz, px, py, n, out, cls); }
extern "C" void stencil_math_bilinear(STENCIL_ARGS) { eval<2>(field, ix, iy, nz, px, py, n, out, cls); }
extern "C" void stencil_math_bicubic(STENCIL_ARGS) { eval<4>(field, ix, iy, nz, px, py, n, out, cls); }
