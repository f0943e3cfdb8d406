// The arithmetic of CDMPressureConversions' theta2T and specific2relative on a level description: the pressure of a
// level is Column::level(k), what verticalData4D(...)->asFloat() holds in the reference, evaluated in the kernel from ps for the
// formula kinds; no 3-D pressure field exists for them.
//   ThetaOp     ThetaTemperatureConverter::getDataSlice, src/CDMPressureConversions.cc:226-245, all in float
//   HumidityOp  HumidityConverter::getDataSlice, :313-333, with mifi_specific_to_relative_humidity
//               (src/vertical_coordinate_transformations.c:114-141) and the packing to short of :330
// The arithmetic is the reference's, operation by operation, with its operand types and rounding points.
//
// column_kernel is convert_kernel of vertical_levels.hip carrying the per-level inputs of an Op: a lane owns one column, consecutive
// lanes own x-adjacent columns, so every plane load and store (the 2-byte stores of the humidity included) is coalesced along x; nt
// is blockIdx.y.  The levels go in groups of kU: all loads of a group are issued before its first exp or powf.  A lane reads its own
// elements of a group before it writes them, so the output of ThetaOp may be its input.
#include "vertical_common.hpp"

#include <cmath>

namespace fimex_amd {

namespace {

struct ThetaOp {
    const float* theta;  // [nt][nz][plane]
    float* out;          // may be theta
    float addOffset;
    struct In {
        float theta;
    };
    __device__ In load(size_t i) const { return {theta[i]}; }
    __device__ void store(size_t i, In v, float p) const
    {
        const float psX1 = 1 / 1000.f;                              // :237-238
        const float Rcp = (float)(8.31432 / 0.0289644) / 1004.f;    // :235-239
        out[i] = ((v.theta + addOffset) * powf(p * psX1, Rcp)) - addOffset;  // :242, pow(float, float) is the float overload
    }
};

struct HumidityOp {
    const float* q;  // [nt][nz][plane]
    const float* T;
    short* out;
    struct In {
        float q, T;
    };
    __device__ In load(size_t i) const { return {q[i], T[i]}; }
    __device__ void store(size_t i, In v, float p) const
    {
        const float c1 = 610.78f, c2 = 17.269f, c3 = 273.16f, c4 = 35.86f;  // mifi_humidity_es, :114-121
        const float x = (c2 * (v.T - c3)) / (v.T - c4);                    // three float operations
        const float es = (float)((double)c1 * exp((double)x));              // exp and the product in double
        float rh = (float)(100. * (double)v.q * (double)p / ((double)es * 0.622));  // :135, left to right in double
        if (rh < 0.f) rh = 0;                                               // :136-139; NaN passes
        else if (rh > 100.f) rh = 100;
        // CDMPressureConversions.cc:330: (short)(25000.f * rh + 0.5), a float product, + 0.5 in double, truncation.  Outside short the
        // reference is undefined; this is what its x86-64 build does: truncate to int32, keep the low 16 bits; NaN gives 0
        const double s = (double)(25000.f * rh) + 0.5;
        const int i32 = (s != s || fabs(s) >= 2147483648.0) ? 0 : (int)s;
        out[i] = (short)(unsigned short)((unsigned)i32 & 0xffffu);
    }
};

template <int kKind, class Op>
__global__ void __launch_bounds__(kBlock) column_kernel(const Levels levels, size_t plane, const Op op)
{
    constexpr int kU = 4;
    const size_t cell = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= plane) return;
    Levels L = levels;
    L.kind = kKind;  // known to the compiler: Column::level is one expression here
    const unsigned nz = L.nz;
    const Column col(L, blockIdx.y, cell, plane);
    const size_t base = (size_t)blockIdx.y * nz * plane + cell;
    unsigned k = 0;
    for (; k + kU <= nz; k += kU) {
        typename Op::In v[kU];
        float p[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            v[u] = op.load(base + (size_t)(k + u) * plane);
            p[u] = col.level(k + u);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) op.store(base + (size_t)(k + u) * plane, v[u], p[u]);
    }
    for (; k < nz; ++k) op.store(base + (size_t)k * plane, op.load(base + (size_t)k * plane), col.level(k));
}

template <class Op>
void launch_columns(const fimex_amd_vertical_levels& pressure, size_t nx, size_t ny, size_t nt, const Op& op, hipStream_t stream)
{
    const size_t plane = nx * ny;
    if (plane == 0 || nt == 0 || pressure.nz == 0) return;
    const dim3 grid = column_grid(plane, nt);
    StreamScratch scratch(coefficient_count(pressure), stream);
    const Levels L = device_levels(pressure, scratch, stream);
    for_level_kind(pressure.kind, [&](auto kind) { column_kernel<decltype(kind)::value, Op><<<grid, kBlock, 0, stream>>>(L, plane, op); });
    FA_HIP(hipGetLastError());
}

}  // namespace

// every argument has been checked (capi_derived.hip); the pointers are device pointers except the coefficient arrays of the description
void launch_theta_to_temperature(const fimex_amd_vertical_levels& pressure, size_t nx, size_t ny, size_t nt, const float* d_theta, float addOffset,
                                 float* d_T, hipStream_t stream)
{
    launch_columns(pressure, nx, ny, nt, ThetaOp{d_theta, d_T, addOffset}, stream);
}

void launch_specific_to_relative_humidity(const fimex_amd_vertical_levels& pressure, size_t nx, size_t ny, size_t nt, const float* d_q,
                                          const float* d_T, short* d_rh, hipStream_t stream)
{
    launch_columns(pressure, nx, ny, nt, HumidityOp{d_q, d_T, d_rh}, stream);
}

}  // namespace fimex_amd
