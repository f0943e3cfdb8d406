// Host shim of fimex_amd/csrc/proj_math.hpp and projection_parse.hip for tests/test_projection_host.py: the string parser and the
// point math the kernels of projection.hip compile, run on the CPU point by point the way the kernels run them.  Built for the host
// only by fimex_amd/build.py (hipcc --cuda-host-only -ffp-contract=off) together with projection_parse.hip; needs no GPU.
// Every entry that parses returns 0, or 1 with the refusal's text in err[errLen].
#include "proj_math.hpp"

#include <cstring>

using namespace fimex_amd;

namespace {

template <class F>
int guarded(char* err, size_t errLen, F&& fn)
{
    try {
        fn();
        return 0;
    } catch (const std::exception& e) {
        if (err && errLen) {
            std::strncpy(err, e.what(), errLen - 1);
            err[errLen - 1] = 0;
        }
        return 1;
    }
}

}  // namespace

// pj_transform(src, dst) on x[n], y[n] in place (project_values_kernel)
extern "C" int projection_host_transform(const char* src, const char* dst, double* x, double* y, int64_t n, char* err, size_t errLen)
{
    return guarded(err, errLen, [&] {
        const ProjPair pair = parse_pair(src, dst);
        for (int64_t i = 0; i < n; ++i) transform_point(pair.src, pair.dst, x[i], y[i]);
    });
}

// the rotation matrix [n][4] of points given in both projections (vector_matrix_kernel with one output value per point)
extern "C" int projection_host_matrix(const char* in, const char* out, const double* inX, const double* inY, const double* outX,
                                      const double* outY, int64_t n, double deltaX, double deltaY, double* matrix, char* err, size_t errLen)
{
    return guarded(err, errLen, [&] {
        const ProjPair pair = parse_pair(in, out);
        for (int64_t i = 0; i < n; ++i)
            vector_matrix_point(pair.src, pair.dst, inX[i], inY[i], outX[i], outY[i], deltaX, deltaY, pair.dst.kind == kLatLong ? 1 : 0, matrix + 4 * i);
    });
}

// keep[n]: is point i (radians or metres in src) inside the box, in degrees of dst (a lane of bounding_box_kernel)
extern "C" int projection_host_bounding_box(const char* src, const char* dst, const double* x, const double* y, int64_t n, double south,
                                            double north, double west, double east, unsigned char* keep, char* err, size_t errLen)
{
    return guarded(err, errLen, [&] {
        const ProjPair pair = parse_pair(src, dst);
        for (int64_t i = 0; i < n; ++i) keep[i] = inside_bounding_box(pair.src, pair.dst, x[i], y[i], south, north, west, east) ? 1 : 0;
    });
}

// mesh_delta on field[oy][ox]; *beyond counts the reads that fall outside the field (they yield 0)
extern "C" double projection_host_mesh_delta(const double* field, int64_t ox, int64_t oy, int* beyond)
{
    *beyond = 0;
    const size_t n = (size_t)ox * (size_t)oy;
    return mesh_delta([&](size_t idx) { return idx < n ? field[idx] : (++*beyond, 0.); }, (size_t)ox, (size_t)oy);
}
