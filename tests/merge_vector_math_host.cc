// fimex_amd/csrc/merge_vector_math.hpp compiled for the CPU with a plain C++ compiler (fimex_amd/build.py:
// build_merge_vector_math_host), used the way merge_vector.hip uses it: a class per cell, the pair functions on every slice, the
// regridded pairs handed in through callables that count how often they are asked.  tests/test_merge_vector_math_host.py compares
// the results with the restatement of tests/merge_vector_ref.py bit for bit.
#include "merge_vector_math.hpp"

#include <cstddef>

namespace mm = fimex_amd::merge_math;

extern "C" {

// interpolation.c:796-810 on [nz][n] slices with the reference's double[4 * n] matrix, in place
int merge_vector_math_rotate(const double* matrix, float* u, float* v, size_t n, size_t nz)
{
    for (size_t z = 0; z < nz; ++z)
        for (size_t i = 0; i < n; ++i) {
            const mm::Pair p = mm::rotate_pair_values(u[z * n + i], v[z * n + i], matrix[4 * i], matrix[4 * i + 1]);
            u[z * n + i] = p.u;
            v[z * n + i] = p.v;
        }
    return 0;
}

// steps 1 (the rotation of it) and 2: regU, regV are the outer pair regridded to the inner grid, not yet rotated.  *asked counts
// the cells whose outer pair was evaluated.
int merge_vector_math_smooth(const float* innerU, const float* innerV, const float* regU, const float* regV, const double* matrix, float* su, float* sv,
                             size_t nx, size_t ny, size_t nz, size_t tw, size_t bw, int useOuter, size_t* asked)
{
    *asked = 0;
    for (size_t y = 0; y < ny; ++y)
        for (size_t x = 0; x < nx; ++x) {
            const mm::SmoothClass c = mm::smooth_class(x, y, nx, ny, tw, bw);
            const size_t cell = y * nx + x;
            for (size_t z = 0; z < nz; ++z) {
                const size_t i = z * ny * nx + cell;
                const mm::Pair s = mm::smooth_pair(c, innerU[i], innerV[i], [&] {
                    ++*asked;
                    return mm::rotate_pair_values(regU[i], regV[i], matrix[4 * cell], matrix[4 * cell + 1]);
                }, useOuter != 0);
                su[i] = s.u;
                sv[i] = s.v;
            }
        }
    return 0;
}

// steps 3 (the rotations of it) and 4 on [nz][n] slices: regSU, regSV the smoothed pair regridded to the target, regOU, regOV the
// outer pair regridded to the target, neither rotated yet
int merge_vector_math_overlay(const float* regSU, const float* regSV, const double* matrixST, const float* regOU, const float* regOV,
                              const double* matrixOT, float* outU, float* outV, size_t n, size_t nz, size_t* asked)
{
    *asked = 0;
    for (size_t z = 0; z < nz; ++z)
        for (size_t cell = 0; cell < n; ++cell) {
            const size_t i = z * n + cell;
            const mm::Pair top = mm::rotate_pair_values(regSU[i], regSV[i], matrixST[4 * cell], matrixST[4 * cell + 1]);
            const mm::Pair o = mm::overlay_pair(top, [&] {
                ++*asked;
                return mm::rotate_pair_values(regOU[i], regOV[i], matrixOT[4 * cell], matrixOT[4 * cell + 1]);
            });
            outU[i] = o.u;
            outV[i] = o.v;
        }
    return 0;
}

}  // extern "C"
