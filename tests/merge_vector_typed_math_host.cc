// fimex_amd/csrc/merge_vector_typed_math.hpp compiled for the CPU with a plain C++ compiler (fimex_amd/build.py:
// build_merge_vector_typed_math_host), used the way merge_vector_typed.hip uses it: a class per cell, the pair functions on every
// slice, the regridded pairs handed in through callables that count how often they are asked.
// tests/test_merge_vector_typed_math_host.py compares the results with the restatement of tests/merge_vector_typed_ref.py byte
// for byte.  packings: double[4][3], (fill, scale, offset) of inner u, inner v, outer u, outer v.
#include "merge_vector_typed_math.hpp"

#include <cstddef>

namespace mm = fimex_amd::merge_math;

namespace {

template <typename T>
struct Cells {
    mm::ComponentOps<T> opsU, opsV;
    T fillIu, fillIv, fillOu, fillOv;
    explicit Cells(const double* p)
        : opsU(mm::make_component_ops<T>(p[0], p[1], p[2], p[6], p[7], p[8])), opsV(mm::make_component_ops<T>(p[3], p[4], p[5], p[9], p[10], p[11])),
          fillIu(static_cast<T>(p[0])), fillIv(static_cast<T>(p[3])), fillOu(static_cast<T>(p[6])), fillOv(static_cast<T>(p[9]))
    {
    }
};

// steps 1 (the rotation and the rounding of it) and 2: regU, regV are the outer pair's counts regridded to the inner grid, not yet
// rotated.  *asked counts the cells whose outer pair was evaluated.
template <typename T>
int smooth(const T* innerU, const T* innerV, const float* regU, const float* regV, const double* matrix, const double* packings, T* su, T* sv,
           size_t nx, size_t ny, size_t nz, size_t tw, size_t bw, int useOuter, size_t* asked)
{
    const Cells<T> k(packings);
    *asked = 0;
    for (size_t y = 0; y < ny; ++y)
        for (size_t x = 0; x < nx; ++x) {
            const mm::SmoothClass c = mm::smooth_class(x, y, nx, ny, tw, bw);
            const size_t cell = y * nx + x;
            for (size_t z = 0; z < nz; ++z) {
                const size_t i = z * ny * nx + cell;
                const mm::StoredPair<T> s = mm::smooth_pair_typed<T>(c, innerU[i], innerV[i], [&] {
                    ++*asked;
                    return mm::rotate_pair_values(regU[i], regV[i], matrix[4 * cell], matrix[4 * cell + 1]);
                }, k.fillOu, k.fillOv, k.opsU, k.opsV, useOuter != 0);
                su[i] = s.u;
                sv[i] = s.v;
            }
        }
    return 0;
}

// steps 3 (the rotations and the roundings of it) and 4 on [nz][n] slices: regSU, regSV the smoothed pair's counts regridded to the
// target, regOU, regOV the outer pair's, neither rotated yet
template <typename T>
int overlay(const float* regSU, const float* regSV, const double* matrixST, const float* regOU, const float* regOV, const double* matrixOT,
            const double* packings, T* outU, T* outV, size_t n, size_t nz, size_t* asked)
{
    const Cells<T> k(packings);
    *asked = 0;
    for (size_t z = 0; z < nz; ++z)
        for (size_t cell = 0; cell < n; ++cell) {
            const size_t i = z * n + cell;
            const mm::Pair top = mm::rotate_pair_values(regSU[i], regSV[i], matrixST[4 * cell], matrixST[4 * cell + 1]);
            const mm::StoredPair<T> o = mm::regrid_overlay_pair_typed<T>(top, k.fillIu, k.fillIv, [&] {
                ++*asked;
                return mm::rotate_pair_values(regOU[i], regOV[i], matrixOT[4 * cell], matrixOT[4 * cell + 1]);
            }, k.fillOu, k.fillOv, k.opsU, k.opsV);
            outU[i] = o.u;
            outV[i] = o.v;
        }
    return 0;
}

}  // namespace

extern "C" {

int merge_vector_typed_math_smooth_short(const short* innerU, const short* innerV, const float* regU, const float* regV, const double* matrix,
                                         const double* packings, short* su, short* sv, size_t nx, size_t ny, size_t nz, size_t tw, size_t bw,
                                         int useOuter, size_t* asked)
{
    return smooth<short>(innerU, innerV, regU, regV, matrix, packings, su, sv, nx, ny, nz, tw, bw, useOuter, asked);
}

int merge_vector_typed_math_smooth_ushort(const unsigned short* innerU, const unsigned short* innerV, const float* regU, const float* regV,
                                          const double* matrix, const double* packings, unsigned short* su, unsigned short* sv, size_t nx, size_t ny,
                                          size_t nz, size_t tw, size_t bw, int useOuter, size_t* asked)
{
    return smooth<unsigned short>(innerU, innerV, regU, regV, matrix, packings, su, sv, nx, ny, nz, tw, bw, useOuter, asked);
}

int merge_vector_typed_math_overlay_short(const float* regSU, const float* regSV, const double* matrixST, const float* regOU, const float* regOV,
                                          const double* matrixOT, const double* packings, short* outU, short* outV, size_t n, size_t nz, size_t* asked)
{
    return overlay<short>(regSU, regSV, matrixST, regOU, regOV, matrixOT, packings, outU, outV, n, nz, asked);
}

int merge_vector_typed_math_overlay_ushort(const float* regSU, const float* regSV, const double* matrixST, const float* regOU, const float* regOV,
                                           const double* matrixOT, const double* packings, unsigned short* outU, unsigned short* outV, size_t n,
                                           size_t nz, size_t* asked)
{
    return overlay<unsigned short>(regSU, regSV, matrixST, regOU, regOV, matrixOT, packings, outU, outV, n, nz, asked);
}

}  // extern "C"
