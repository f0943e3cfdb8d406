// Plan building on the device: the coordinate transforms the reference obtains from PROJ.4's pj_transform --
// mifi_project_values / mifi_project_axes (src/interpolation.c:1158-1244), the local rotation matrix
// mifi_get_vector_reproject_matrix (:719-788 -> :441-521 -> :330-438) and the bounding-box reduction of CDMExtractor -- for
// 4 M-cell target grids.  This file holds the kernels and their launchers; each kernel is a grid-stride loop around the point math
// of proj_math.hpp.  Which projection strings are supported and which are refused is said in projection_parse.hip.
#include "extract.hpp"
#include "proj_math.hpp"

#include <algorithm>
#include <vector>

namespace fimex_amd {

namespace {

__global__ void __launch_bounds__(kBlock) project_values_kernel(ProjParams src, ProjParams dst, double* __restrict__ x, double* __restrict__ y, size_t n)
{
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double px = x[i], py = y[i];
        transform_point(src, dst, px, py);
        x[i] = px;
        y[i] = py;
    }
}

// the [iy][ix] mesh of two axes, transformed (interpolation.c:1226-1234)
__global__ void __launch_bounds__(kBlock) project_axes_kernel(ProjParams src, ProjParams dst, const double* __restrict__ xAxis,
                                                              const double* __restrict__ yAxis, uint32_t ix, uint32_t iy,
                                                              double* __restrict__ outX, double* __restrict__ outY)
{
    const size_t n = (size_t)ix * iy, stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double px = xAxis[i % ix], py = yAxis[i / ix];
        transform_point(src, dst, px, py);
        outX[i] = px;
        outY[i] = py;
    }
}

// reduceLatLonBoundingBox (src/CDMExtractor.cc:484-511): which columns and rows of the mesh of two axes hold a point inside the
// box.  A wave takes 64 neighbouring ix of one iy; a lane tests its point (inside_bounding_box).  The flags are plain byte stores
// of the value 1, so lanes that race write the same thing.
__global__ void __launch_bounds__(kBlock) bounding_box_kernel(ProjParams src, ProjParams dst, const double* __restrict__ xAxis,
                                                              const double* __restrict__ yAxis, uint32_t nx, uint32_t ny, double south,
                                                              double north, double west, double east, unsigned char* __restrict__ xKeep,
                                                              unsigned char* __restrict__ yKeep)
{
    constexpr uint32_t kWaves = kBlock / kWave;
    const uint32_t tiles = (nx + kWave - 1) / kWave, lane = threadIdx.x % kWave;
    const size_t waves = (size_t)tiles * ny, stride = (size_t)gridDim.x * kWaves;
    for (size_t w = (size_t)blockIdx.x * kWaves + threadIdx.x / kWave; w < waves; w += stride) {
        const uint32_t iy = (uint32_t)(w / tiles), ix = (uint32_t)(w % tiles) * kWave + lane;
        bool keep = false;
        if (ix < nx) {
            keep = inside_bounding_box(src, dst, xAxis[ix], yAxis[iy], south, north, west, east);
            if (keep) xKeep[ix] = 1;
        }
        if (__any(keep) && lane == 0) yKeep[iy] = 1;
    }
}

// mifi_get_vector_reproject_matrix_points_proj_delta (interpolation.c:330-438): the matrix of every point (vector_matrix_point)
// outX / outY: the two axes of the output mesh (axes != 0) or one value per point
__global__ void __launch_bounds__(kBlock) vector_matrix_kernel(ProjParams in, ProjParams out, const double* __restrict__ inX,
                                                               const double* __restrict__ inY, const double* __restrict__ outX,
                                                               const double* __restrict__ outY, int axes, uint32_t ox, size_t n,
                                                               double deltaX, double deltaY, int outIsLatLong,
                                                               double* __restrict__ matrix)
{
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double outXf = axes ? outX[i % ox] : outX[i], outYf = axes ? outY[i / ox] : outY[i];
        double m[4];
        vector_matrix_point(in, out, inX[i], inY[i], outXf, outYf, deltaX, deltaY, outIsLatLong, m);
        matrix[4 * i + 0] = m[0];
        matrix[4 * i + 1] = m[1];
        matrix[4 * i + 2] = m[2];
        matrix[4 * i + 3] = m[3];
    }
}

uint32_t point_blocks(size_t n)
{
    const size_t want = ceil_div(n, (size_t)kBlock), cap = (size_t)std::max(1, tuning("PROJECT_MAX_BLOCKS", 256 * 8));
    return (uint32_t)(want < cap ? (want ? want : 1) : cap);
}

// an axis as the kernels want it: one of longitude / latitude type arrives in degrees (Projection.cc:81-90, interpolation.c:740-745)
void copy_axis(double* dst, const double* h_axis, size_t n, bool inDegree)
{
    for (size_t i = 0; i < n; ++i) dst[i] = inDegree ? h_axis[i] * kDegToRad : h_axis[i];
}

// stream-ordered scratch of one call, freed on the stream behind the work that uses it
struct AsyncBytes {
    void* p = nullptr;
    hipStream_t stream;
    AsyncBytes(size_t bytes, hipStream_t stream) : stream(stream) { FA_HIP(hipMallocAsync(&p, bytes, stream)); }
    ~AsyncBytes() { if (p) (void)hipFreeAsync(p, stream); }
    AsyncBytes(const AsyncBytes&) = delete;
    AsyncBytes& operator=(const AsyncBytes&) = delete;
};

}  // namespace

void launch_project_values(const char* projIn, const char* projOut, double* d_x, double* d_y, size_t n, hipStream_t stream)
{
    const ProjPair pair = parse_pair(projIn, projOut);
    const ProjParams &src = pair.src, &dst = pair.dst;
    if (n == 0) return;
    project_values_kernel<<<point_blocks(n), kBlock, 0, stream>>>(src, dst, d_x, d_y, n);
    FA_HIP(hipGetLastError());
}

void launch_project_axes(const char* projIn, const char* projOut, const double* h_xAxis, const double* h_yAxis, size_t ix, size_t iy,
                         double* d_outX, double* d_outY, hipStream_t stream)
{
    const ProjPair pair = parse_pair(projIn, projOut);
    const ProjParams &src = pair.src, &dst = pair.dst;
    if (ix * iy == 0) return;
    FA_REQUIRE(ix <= 0x7FFFFFFFu && iy <= 0x7FFFFFFFu, "axis too long");
    DeviceArray<double> d_axes(ix + iy);
    FA_HIP(hipMemcpyAsync(d_axes.get(), h_xAxis, ix * sizeof(double), hipMemcpyHostToDevice, stream));
    FA_HIP(hipMemcpyAsync(d_axes.get() + ix, h_yAxis, iy * sizeof(double), hipMemcpyHostToDevice, stream));
    project_axes_kernel<<<point_blocks(ix * iy), kBlock, 0, stream>>>(src, dst, d_axes.get(), d_axes.get() + ix, (uint32_t)ix, (uint32_t)iy, d_outX, d_outY);
    FA_HIP(hipGetLastError());
    FA_HIP(hipStreamSynchronize(stream));  // d_axes is released on return
}

void run_bounding_box(const char* projIn, const char* projLonLat, const double* h_xAxis, size_t nx, const double* h_yAxis, size_t ny,
                      bool axesInDegree, double south, double north, double west, double east, unsigned char* h_xKeep, unsigned char* h_yKeep,
                      hipStream_t stream)
{
    const ProjPair pair = parse_pair(projIn, projLonLat);
    if (nx * ny == 0) return;
    FA_REQUIRE(nx <= 0x7FFFFFFFu && ny <= 0x7FFFFFFFu, "axis too long");
    std::vector<double> axes(nx + ny);
    copy_axis(axes.data(), h_xAxis, nx, axesInDegree);
    copy_axis(axes.data() + nx, h_yAxis, ny, axesInDegree);
    const size_t axisBytes = (nx + ny) * sizeof(double);
    AsyncBytes scratch(axisBytes + nx + ny, stream);
    double* d_axes = static_cast<double*>(scratch.p);
    unsigned char* d_keep = static_cast<unsigned char*>(scratch.p) + axisBytes;
    FA_HIP(hipMemcpyAsync(d_axes, axes.data(), axisBytes, hipMemcpyHostToDevice, stream));
    FA_HIP(hipMemsetAsync(d_keep, 0, nx + ny, stream));
    const size_t waves = ceil_div(nx, (size_t)kWave) * ny;
    bounding_box_kernel<<<point_blocks(waves * kWave), kBlock, 0, stream>>>(pair.src, pair.dst, d_axes, d_axes + nx, (uint32_t)nx, (uint32_t)ny,
                                                                            south, north, west, east, d_keep, d_keep + nx);
    FA_HIP(hipGetLastError());
    FA_HIP(hipMemcpyAsync(h_xKeep, d_keep, nx, hipMemcpyDeviceToHost, stream));
    FA_HIP(hipMemcpyAsync(h_yKeep, d_keep + nx, ny, hipMemcpyDeviceToHost, stream));
    FA_HIP(hipStreamSynchronize(stream));  // axes and the caller's flags are in use until here
}

// mifi_get_vector_reproject_matrix, interpolation.c:719-788
void launch_vector_reproject_matrix(const char* projIn, const char* projOut, const double* h_outXAxis, const double* h_outYAxis,
                                    int xAxisType, int yAxisType, size_t ox, size_t oy, double* d_matrix, hipStream_t stream)
{
    const ProjPair pair = parse_pair(projIn, projOut);
    const ProjParams &in = pair.src, &out = pair.dst;
    const size_t n = ox * oy;
    if (n == 0) return;
    FA_REQUIRE(ox <= 0x7FFFFFFFu && oy <= 0x7FFFFFFFu, "axis too long");
    std::vector<double> axes(ox + oy);
    copy_axis(axes.data(), h_outXAxis, ox, xAxisType == FIMEX_AMD_LONGITUDE || xAxisType == FIMEX_AMD_LATITUDE);
    copy_axis(axes.data() + ox, h_outYAxis, oy, yAxisType == FIMEX_AMD_LONGITUDE || yAxisType == FIMEX_AMD_LATITUDE);
    DeviceArray<double> d_axes(ox + oy), d_inX(n), d_inY(n);
    FA_HIP(hipMemcpyAsync(d_axes.get(), axes.data(), axes.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    // positions of the output mesh in the input projection (:773)
    project_axes_kernel<<<point_blocks(n), kBlock, 0, stream>>>(out, in, d_axes.get(), d_axes.get() + ox, (uint32_t)ox, (uint32_t)oy, d_inX.get(), d_inY.get());
    FA_HIP(hipGetLastError());
    auto at = [&](size_t idx) {
        double v = 0;
        FA_HIP(hipMemcpyAsync(&v, d_inX.get() + idx, sizeof(double), hipMemcpyDeviceToHost, stream));
        FA_HIP(hipStreamSynchronize(stream));
        return v;
    };
    const double delta = mesh_delta(at, ox, oy);
    vector_matrix_kernel<<<point_blocks(n), kBlock, 0, stream>>>(in, out, d_inX.get(), d_inY.get(), d_axes.get(), d_axes.get() + ox, 1, (uint32_t)ox,
                                                                 n, delta, delta, out.kind == kLatLong ? 1 : 0, d_matrix);
    FA_HIP(hipGetLastError());
    FA_HIP(hipStreamSynchronize(stream));  // temporaries are released on return
}

// mifi_get_vector_reproject_matrix_field, interpolation.c:657-717: the mesh is given in the INPUT projection
void launch_vector_reproject_matrix_field(const char* projIn, const char* projOut, const double* h_inX, const double* h_inY, size_t ox,
                                          size_t oy, double* d_matrix, hipStream_t stream)
{
    const ProjPair pair = parse_pair(projIn, projOut);
    const ProjParams &in = pair.src, &out = pair.dst;
    const size_t n = ox * oy;
    if (n == 0) return;
    DeviceArray<double> d_in(2 * n), d_out(2 * n);
    FA_HIP(hipMemcpyAsync(d_in.get(), h_inX, n * sizeof(double), hipMemcpyHostToDevice, stream));
    FA_HIP(hipMemcpyAsync(d_in.get() + n, h_inY, n * sizeof(double), hipMemcpyHostToDevice, stream));
    FA_HIP(hipMemcpyAsync(d_out.get(), d_in.get(), 2 * n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    project_values_kernel<<<point_blocks(n), kBlock, 0, stream>>>(in, out, d_out.get(), d_out.get() + n, n);  // :696
    FA_HIP(hipGetLastError());
    const double delta = mesh_delta([&](size_t idx) { return h_inX[idx]; }, ox, oy);
    vector_matrix_kernel<<<point_blocks(n), kBlock, 0, stream>>>(in, out, d_in.get(), d_in.get() + n, d_out.get(), d_out.get() + n, 0, (uint32_t)ox, n,
                                                                 delta, delta, out.kind == kLatLong ? 1 : 0, d_matrix);
    FA_HIP(hipGetLastError());
    FA_HIP(hipStreamSynchronize(stream));
}

// mifi_get_vector_reproject_matrix_points, interpolation.c:607-655: a list of points in the OUTPUT projection (m or rad)
void launch_vector_reproject_matrix_points(const char* projIn, const char* projOut, int inputIsMetric, const double* h_outX,
                                           const double* h_outY, size_t on, double* d_matrix, hipStream_t stream)
{
    const ProjPair pair = parse_pair(projIn, projOut);
    const ProjParams &in = pair.src, &out = pair.dst;
    if (on == 0) return;
    DeviceArray<double> d_in(2 * on), d_out(2 * on);
    FA_HIP(hipMemcpyAsync(d_out.get(), h_outX, on * sizeof(double), hipMemcpyHostToDevice, stream));
    FA_HIP(hipMemcpyAsync(d_out.get() + on, h_outY, on * sizeof(double), hipMemcpyHostToDevice, stream));
    FA_HIP(hipMemcpyAsync(d_in.get(), d_out.get(), 2 * on * sizeof(double), hipMemcpyDeviceToDevice, stream));
    project_values_kernel<<<point_blocks(on), kBlock, 0, stream>>>(out, in, d_in.get(), d_in.get() + on, on);  // :635
    FA_HIP(hipGetLastError());
    const double delta = inputIsMetric ? 100 : 0.00001;  // :641
    vector_matrix_kernel<<<point_blocks(on), kBlock, 0, stream>>>(in, out, d_in.get(), d_in.get() + on, d_out.get(), d_out.get() + on, 0, 1, on, delta,
                                                                  delta, out.kind == kLatLong ? 1 : 0, d_matrix);
    FA_HIP(hipGetLastError());
    FA_HIP(hipStreamSynchronize(stream));
}

int projection_is_degree(const char* proj)
{
    const ProjParams p = parse_proj4(proj);
    return (p.kind == kLatLong || p.kind == kObTran) ? 1 : 0;
}

}  // namespace fimex_amd
