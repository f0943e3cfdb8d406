// The level converters in front of the vertical interpolation: what the reference's VerticalConverter chain puts
// into verticalData4D for altitude, height and ocean depth, as the f32 field [nt][nz][ny][nx] vertical.hip takes as a FIELD.
//   altitude_kernel   PressureIntegrationToAltitudeConverter::getDataSlice (hypsometric equation, src/coordSys/verticalTransform/
//                     PressureIntegrationToAltitudeConverter.cc:185-208), optionally followed by AltitudeHeightConverter (:87-105)
//   convert_kernel    PressureToStandardAltitudeConverter, AltitudeStandardToPressureConverter, OceanSCoordinateGToDepthConverter
// The arithmetic is the reference's, operation by operation, with its operand types and rounding points.
//
// A lane owns one column; consecutive lanes own x-adjacent columns, so every plane load and store is coalesced along x; nt is
// blockIdx.y; no workgroup waits for another.  Along z the only dependency of the integration is one double add, so the levels
// go in groups of kAhead: all loads of a group (T, q, an explicit pressure level) are issued before its first logarithm.
#include "vertical_common.hpp"

#include <cmath>
#include <type_traits>

namespace fimex_amd {

namespace {

constexpr double kEarthGravity = 9.80665;                                          // MIFI_EARTH_GRAVITY
constexpr double kBarometricFactor = 8.31432 / (kEarthGravity * 0.0289644);        // vertical_coordinate_transformations.c:73-74
constexpr double kZMolWeightRatio = .60771704180064308681;                         // :77
constexpr double kStandardP = 1013.25, kStandardT = 288.15;                        // :90, :105
constexpr int kAhead = 8;  // levels whose loads are in flight together

struct AltitudeArgs {
    Levels p;            // pressure of every level
    const float* T;      // [nt][nz][plane]
    const float* q;      // [nt][nz][plane] or NULL
    const float* sap;    // [nt][plane]
    const float* sgp;    // [nt][plane]
    const double* topo;  // [plane] or NULL
    double topoFactor;
    float* out;          // [nt][nz][plane]
    size_t plane;
    int surfaceFirst;    // 1, 0 or FIMEX_AMD_VORDER_AUTO
};

// U levels of one column, i0 .. i0 + U - 1 counted from the surface: the body of the loop of :190-207
template <int U, bool kHumidity>
__device__ __forceinline__ void integrate_levels(const Column& col, const float* Tcol, const float* qcol, float* res, unsigned i0, unsigned nz,
                                                 bool up, bool height, double topoTerm, double& a, float& pLow)
{
    float p[U], T[U], q[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned k = up ? i0 + u : nz - 1 - (i0 + u);
        p[u] = col.level(k);
        T[u] = Tcol[(size_t)k * col.plane];
        q[u] = kHumidity ? qcol[(size_t)k * col.plane] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned k = up ? i0 + u : nz - 1 - (i0 + u);
        float Tv = T[u];
        if (kHumidity) Tv = (float)((1 + kZMolWeightRatio * (double)q[u]) * (double)Tv);  // mifi_virtual_temperature, :108-111
        const float ratio = pLow / p[u];                                                 // float division, correctly rounded
        const float lt = (float)(log((double)ratio) * (double)Tv * kBarometricFactor);  // mifi_barometric_layer_thickness, :154-157
        a += (double)lt;
        res[(size_t)k * col.plane] = height ? (float)(a + topoTerm) : (float)a;
        pLow = p[u];
    }
}

template <int kKind, bool kHumidity>
__global__ void __launch_bounds__(kBlock) altitude_kernel(const AltitudeArgs g)
{
    const size_t cell = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= g.plane) return;
    const size_t t = blockIdx.y;
    Levels L = g.p;
    L.kind = kKind;  // known to the compiler: Column::level is one expression here
    const unsigned nz = L.nz;
    bool up = g.surfaceFirst != 0;
    if (g.surfaceFirst < 0) {  // start_high_p of :105-122: the one column at index 0 of every other dimension, in every lane
        const Column first(L, 0, 0, g.plane);
        up = first.level(0) > first.level(nz - 1);
    }
    const Column col(L, t, cell, g.plane);
    const float* Tcol = g.T + t * nz * g.plane + cell;
    const float* qcol = kHumidity ? g.q + t * nz * g.plane + cell : nullptr;
    float* res = g.out + t * nz * g.plane + cell;
    double a = (double)g.sgp[t * g.plane + cell] / kEarthGravity;  // :187
    float pLow = g.sap[t * g.plane + cell];
    const bool height = g.topo != nullptr;
    const double topoTerm = height ? g.topoFactor * g.topo[cell] : 0.0;  // AltitudeHeightConverter.cc:101-102
    unsigned i = 0;
    for (; i + kAhead <= nz; i += kAhead) integrate_levels<kAhead, kHumidity>(col, Tcol, qcol, res, i, nz, up, height, topoTerm, a, pLow);
    for (; i < nz; ++i) integrate_levels<1, kHumidity>(col, Tcol, qcol, res, i, nz, up, height, topoTerm, a, pLow);
}

// The three elementwise conversions as the Op of convert_kernel: State is a column's part of it, input(k) what level k reads,
// value(x) the arithmetic on it.
template <int kKind, bool kToPressure>
struct StandardOp {
    Levels L;            // L.kind == kKind
    const double* topo;  // [plane] or NULL
    double topoFactor;
    struct State {
        const Levels& L;
        const float* fieldCol;
        size_t plane;
        double ps, pDiff;
        bool hasTopo;
        double topoTerm;
        __device__ State(const StandardOp& op, size_t t, size_t cell, size_t plane)
            : L(op.L), plane(plane), hasTopo(op.topo != nullptr), topoTerm(hasTopo ? op.topoFactor * op.topo[cell] : 0.0)
        {
            const Column col(op.L, t, cell, plane);
            fieldCol = col.fieldCol;
            ps = col.ps;
            pDiff = col.pDiff;
        }
        // the level as the inner converter's double data holds it: the formula of Column::level unrounded, a field or an axis
        // value promoted
        __device__ double input(unsigned k) const
        {
            switch (kKind) {
            case FIMEX_AMD_VLEVEL_FIELD: return (double)fieldCol[(size_t)k * plane];
            case FIMEX_AMD_VLEVEL_AXIS: return L.c0[k];
            case FIMEX_AMD_VLEVEL_SIGMA: return L.ptop + L.c0[k] * pDiff;
            case FIMEX_AMD_VLEVEL_HYBRID_SIGMA: return (L.c0[k] * L.p0) + (L.c1[k] * ps);
            default: return L.c0[k] + (L.c1[k] * ps);
            }
        }
        __device__ float value(double x) const
        {
            if (kToPressure) {  // mifi_barometric_pressure, :79-91, on the altitude x + topography (a height made an altitude first)
                const double C = -1 / (kBarometricFactor * kStandardT);
                if (hasTopo) x = x + topoTerm;
                return (float)(kStandardP * exp(C * x));
            }
            const double K = -kBarometricFactor * kStandardT;  // mifi_barometric_height, :94-106
            const double alt = K * log(x / kStandardP);
            return hasTopo ? (float)(alt + topoTerm) : (float)alt;
        }
    };
};

template <int kGeneration>
struct OceanDepthOp {
    const double* s;      // [nz], device
    const double* C;      // [nz], device
    double depth_c;
    const double* depth;  // [plane]
    const double* eta;    // [nt][plane] or NULL
    struct State {
        const OceanDepthOp& op;
        double h, zeta, inv;
        __device__ State(const OceanDepthOp& op, size_t t, size_t cell, size_t plane)
            : op(op), h(op.depth[cell]), zeta(op.eta ? op.eta[t * plane + cell] : 0.0)
        {
            inv = (kGeneration == 1) ? 1 / h : 1 / (h + op.depth_c);  // vertical_coordinate_transformations.c:161, :170
        }
        __device__ double input(unsigned k) const
        {
            if (kGeneration == 1) {  // mifi_ocean_s_g1_z, :159-167
                const double S = op.depth_c * op.s[k] + (h - op.depth_c) * op.C[k];
                return S + zeta * (1 + S * inv);
            }
            const double S = inv * (op.depth_c * op.s[k] + h * op.C[k]);  // mifi_ocean_s_g2_z, :168-176
            return zeta + (zeta + h) * S;
        }
        __device__ float value(double z) const { return (float)(-1. * z); }  // positive down, OceanSCoordinateGToDepthConverter.cc:102
    };
};

template <class Op>
__global__ void __launch_bounds__(kBlock) convert_kernel(const Op op, size_t plane, unsigned nz, float* __restrict__ out)
{
    constexpr int kU = 4;
    const size_t cell = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= plane) return;
    const size_t t = blockIdx.y;
    const typename Op::State col(op, t, cell, plane);
    float* res = out + t * nz * plane + cell;
    unsigned k = 0;
    for (; k + kU <= nz; k += kU) {
        double x[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) x[u] = col.input(k + u);
#pragma unroll
        for (int u = 0; u < kU; ++u) res[(size_t)(k + u) * plane] = col.value(x[u]);
    }
    for (; k < nz; ++k) res[(size_t)k * plane] = col.value(col.input(k));
}

}  // namespace

bool vertical_order_known(int surfaceFirst) { return surfaceFirst == FIMEX_AMD_VORDER_AUTO || surfaceFirst == 0 || surfaceFirst == 1; }

// every argument has been checked (capi.hip); the pointers are device pointers except the coefficient arrays of the description
void launch_vertical_altitude(const fimex_amd_vertical_levels& pressure, size_t nx, size_t ny, size_t nt, const float* d_T, const float* d_q,
                              const float* d_sap, const float* d_sgp, int surfaceFirst, const double* d_topo, double topoFactor, float* d_out,
                              hipStream_t stream)
{
    const size_t plane = nx * ny;
    if (plane == 0 || nt == 0 || pressure.nz == 0) return;
    const dim3 grid = column_grid(plane, nt);
    StreamScratch scratch(coefficient_count(pressure), stream);
    AltitudeArgs g{};
    g.p = device_levels(pressure, scratch, stream);
    g.T = d_T;
    g.q = d_q;
    g.sap = d_sap;
    g.sgp = d_sgp;
    g.topo = d_topo;
    g.topoFactor = topoFactor;
    g.out = d_out;
    g.plane = plane;
    g.surfaceFirst = surfaceFirst;
    for_level_kind(pressure.kind, [&](auto kind) {
        if (d_q) altitude_kernel<decltype(kind)::value, true><<<grid, kBlock, 0, stream>>>(g);
        else altitude_kernel<decltype(kind)::value, false><<<grid, kBlock, 0, stream>>>(g);
    });
    FA_HIP(hipGetLastError());
}

void launch_vertical_standard(bool toPressure, const fimex_amd_vertical_levels& levels, size_t nx, size_t ny, size_t nt, const double* d_topo,
                              double topoFactor, float* d_out, hipStream_t stream)
{
    const size_t plane = nx * ny;
    if (plane == 0 || nt == 0 || levels.nz == 0) return;
    const dim3 grid = column_grid(plane, nt);
    StreamScratch scratch(coefficient_count(levels), stream);
    const Levels L = device_levels(levels, scratch, stream);
    for_level_kind(levels.kind, [&](auto kind) {
        constexpr int k = decltype(kind)::value;
        if (toPressure) convert_kernel<<<grid, kBlock, 0, stream>>>(StandardOp<k, true>{L, d_topo, topoFactor}, plane, L.nz, d_out);
        else convert_kernel<<<grid, kBlock, 0, stream>>>(StandardOp<k, false>{L, d_topo, topoFactor}, plane, L.nz, d_out);
    });
    FA_HIP(hipGetLastError());
}

void launch_vertical_ocean_depth(int generation, size_t nx, size_t ny, size_t nz, size_t nt, const double* h_s, const double* h_C, double depth_c,
                                 const double* d_depth, const double* d_eta, float* d_out, hipStream_t stream)
{
    const size_t plane = nx * ny;
    if (plane == 0 || nt == 0 || nz == 0) return;
    const dim3 grid = column_grid(plane, nt);
    StreamScratch scratch(2 * nz, stream);
    double* s = scratch.take(nz);
    double* C = scratch.take(nz);
    upload(s, h_s, nz, stream);
    upload(C, h_C, nz, stream);
    if (generation == 1) convert_kernel<<<grid, kBlock, 0, stream>>>(OceanDepthOp<1>{s, C, depth_c, d_depth, d_eta}, plane, (unsigned)nz, d_out);
    else convert_kernel<<<grid, kBlock, 0, stream>>>(OceanDepthOp<2>{s, C, depth_c, d_depth, d_eta}, plane, (unsigned)nz, d_out);
    FA_HIP(hipGetLastError());
}

}  // namespace fimex_amd
