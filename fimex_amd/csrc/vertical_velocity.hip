// Vertical velocity on model levels: what CDMProcessor::addVerticalVelocity computes with mifi_griddistance and
// mifi_compute_vertical_velocity (src/interpolation.c:1539-1595, :1597-1773), operation by operation, with the reference's operand
// types and rounding points.
//   griddistance_kernel  the great-circle distance to the right and to the lower neighbour, the copies into the last column and
//                        the reference's rule for the last row (g[p] = g[p - ny], applied from left to right)
//   hydrostatic_kernel   pass A: each column from the surface upward, the geopotential z of every level k >= 1 as a double into
//                        stream-ordered scratch
//   velocity_kernel      pass B: each column from k = 1 downward, the divergence sum and w, the border copies included
//
// A lane owns one column; consecutive lanes own x-adjacent columns, so every plane load and store is coalesced along x; no
// workgroup waits for another.  Pass B reads u, v and z of the four neighbour columns through the cache: its workgroup is a tile of
// kTileX x kTileY columns, so the y-neighbours are rows of the same tile.  A border lane computes the value of the interior cell
// the reference copies from, so no lane reads another lane's store.  The host loops over nt: the scratch holds one time step, and
// the stream orders pass A of the next step behind pass B of this one.
#include "vertical_common.hpp"

#include <cmath>
#include <vector>

namespace fimex_amd {

namespace {

constexpr double kDegToRad = .017453292519943296;            // DEG_TO_RAD of PROJ.4's proj_api.h
constexpr double kEarthRadius = 6371000;                     // MIFI_EARTH_RADIUS_M
constexpr double kGasConstantDryAir = 8.31432 / 0.0289644;   // MIFI_GAS_CONSTANT / MIFI_MOLAR_MASS_DRY_AIR, :1600
constexpr double kEarthGravity = 9.80665;                    // MIFI_EARTH_GRAVITY
constexpr int kAhead = 4;                                    // levels whose loads are in flight together
constexpr int kTileX = 64, kTileY = 4;                       // pass B: a wave per row, kBlock lanes
static_assert(kTileX * kTileY == kBlock, "a tile is one workgroup");

// mifi_great_circle_angle (:305-308) of two points in degrees, times the earth's radius, rounded to float as the assignment does
__device__ __forceinline__ float great_circle_m(const double* lon, const double* lat, size_t p, size_t q)
{
    const double lat0 = kDegToRad * lat[p], lon0 = kDegToRad * lon[p], lat1 = kDegToRad * lat[q], lon1 = kDegToRad * lon[q];
    return (float)(kEarthRadius * acos(sin(lat0) * sin(lat1) + cos(lat0) * cos(lat1) * cos(lon1 - lon0)));
}

// nx * ny >= 2.  Every lane finds the cell whose distances the reference's copies leave in its own cell and computes them.
__global__ void __launch_bounds__(kBlock) griddistance_kernel(size_t nx, size_t ny, const double* __restrict__ lon, const double* __restrict__ lat,
                                                              float* __restrict__ distX, float* __restrict__ distY)
{
    const size_t n = nx * ny, p = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    if (nx == 1 || ny == 1) {  // :1546-1557
        const size_t s = p < n - 1 ? p : n - 2;
        const float d = great_circle_m(lon, lat, s, s + 1);
        distX[p] = d;
        distY[p] = d;
        return;
    }
    size_t i = p % nx, j = p / nx;
    if (j == ny - 1) {    // :1588-1592: g[p] = g[p - ny] for i = 0 .. nx-1 in turn; a source inside the last row has been
        i %= ny;          // overwritten before it is read, which is the chain i -> i - ny down to i < ny
        const size_t s = (ny - 1) * nx + i - ny;
        i = s % nx;
        j = s / nx;       // < ny - 1
    }
    if (i == nx - 1) i = nx - 2;  // :1582-1586
    const size_t s = i + nx * j;
    distX[p] = great_circle_m(lon, lat, s, s + 1);
    distY[p] = great_circle_m(lon, lat, s, s + nx);
}

struct VelocityArgs {
    unsigned nx, ny, nz;
    size_t plane;
    double dx, dy, rdx_2, rdy_2;
    const float *distX, *distY, *zs;  // [plane]
    const float *ps;                  // [plane], this time step
    const float *u, *v, *t;           // [nz][plane], this time step
    float* w;                         // [nz][plane], this time step
    const double *ah, *bh;            // [nz + 1], half levels
    double* z;                        // [nz - 1][plane]: level k at k - 1
};

// the pressure variables of one cell, :1686-1690
struct Layer {
    double pm, dp, dlnp, alfa;
    __device__ __forceinline__ Layer(const VelocityArgs& g, unsigned k, double ps)
    {
        pm = g.ah[k] + g.bh[k] * ps;
        const double pp = g.ah[k + 1] + g.bh[k + 1] * ps;
        dp = pp - pm;
        dlnp = log(pp / pm);
        alfa = 1. - pm * dlnp / dp;
    }
};

// dp alone, for the neighbours
__device__ __forceinline__ double layer_dp(const VelocityArgs& g, unsigned k, double ps)
{
    const double pm = g.ah[k] + g.bh[k] * ps;
    const double pp = g.ah[k + 1] + g.bh[k + 1] * ps;
    return pp - pm;
}

// U levels kHigh, kHigh - 1, ... of one column, all >= 1: the body of the loop of :1705-1714
template <int U>
__device__ __forceinline__ void hydrostatic_levels(const VelocityArgs& g, size_t cell, double ps, unsigned kHigh, double& sum)
{
    float T[U];
#pragma unroll
    for (int u = 0; u < U; ++u) T[u] = g.t[(size_t)(kHigh - u) * g.plane + cell];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned k = kHigh - u;
        const Layer l(g, k, ps);
        const double rt = kGasConstantDryAir * (double)T[u];
        g.z[(size_t)(k - 1) * g.plane + cell] = sum + rt * l.alfa;
        sum += rt * l.dlnp;
    }
}

// z of level 0 is never read (w exists from level 1 on), so the march ends at level 1
__global__ void __launch_bounds__(kBlock) hydrostatic_kernel(const VelocityArgs g)
{
    const size_t cell = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= g.plane) return;
    const double ps = (double)g.ps[cell];
    double sum = (double)g.zs[cell] * kEarthGravity;  // :1702
    unsigned k = g.nz - 1;                            // nz >= 2 here
    for (; k >= kAhead; k -= kAhead) hydrostatic_levels<kAhead>(g, cell, ps, k, sum);
    for (; k >= 1; --k) hydrostatic_levels<1>(g, cell, ps, k, sum);
}

// what pass B keeps of a column in registers
struct Neighbour {
    double ps, mapRatio;  // the ratio that multiplies this neighbour's wind: Y for the x-neighbours, X for the y-neighbours
};

// U levels k0 .. k0 + U - 1 (all >= 1) of the column at c, written to the column at own: the loops of :1726-1758
template <int U>
__device__ __forceinline__ void velocity_levels(const VelocityArgs& g, size_t c, size_t own, unsigned k0, double ps, double rhxy, double cx, double cy,
                                                const Neighbour& left, const Neighbour& right, const Neighbour& up, const Neighbour& down,
                                                double& sum)
{
    const size_t nx = g.nx;
    float uL[U], uR[U], vU[U], vD[U], T[U];
    double zL[U], zR[U], zU[U], zD[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const size_t at = (size_t)(k0 + u) * g.plane + c, zat = (size_t)(k0 + u - 1) * g.plane + c;
        uL[u] = g.u[at - 1];
        uR[u] = g.u[at + 1];
        vU[u] = g.v[at - nx];
        vD[u] = g.v[at + nx];
        T[u] = g.t[at];
        zL[u] = g.z[zat - 1];
        zR[u] = g.z[zat + 1];
        zU[u] = g.z[zat - nx];
        zD[u] = g.z[zat + nx];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned k = k0 + u;
        const Layer l(g, k, ps);
        const double uuL = left.mapRatio * (double)uL[u] * layer_dp(g, k, left.ps);  // :1729-1730
        const double uuR = right.mapRatio * (double)uR[u] * layer_dp(g, k, right.ps);
        const double vvU = up.mapRatio * (double)vU[u] * layer_dp(g, k, up.ps);
        const double vvD = down.mapRatio * (double)vD[u] * layer_dp(g, k, down.ps);
        const double div = rhxy * (g.rdx_2 * (uuR - uuL) + g.rdy_2 * (vvD - vvU));      // :1736-1737
        const double w1 = kGasConstantDryAir * (double)T[u] * (l.dlnp * sum + l.alfa * div) / l.dp;
        const double w2 = cx * (zR[u] - zL[u]) + cy * (zD[u] - zU[u]);                   // :1741-1742
        g.w[(size_t)k * g.plane + own] = (float)((w1 + w2) / kEarthGravity);
        sum = sum + div;
    }
}

// The lane at (i, j) computes the cell (ic, jc) = (i, j) clamped into the interior and stores it at (i, j): the row copies of
// :1747-1752 followed by the column copies of :1753-1758 leave exactly that value in a border cell, corners included.
__global__ void __launch_bounds__(kBlock) velocity_kernel(const VelocityArgs g)
{
    const unsigned i = blockIdx.x * kTileX + threadIdx.x, j = blockIdx.y * kTileY + threadIdx.y;
    if (i >= g.nx || j >= g.ny) return;
    const unsigned ic = min(max(i, 1u), g.nx - 2), jc = min(max(j, 1u), g.ny - 2);  // nx, ny >= 3
    const size_t nx = g.nx, own = (size_t)j * nx + i, c = (size_t)jc * nx + ic;
    g.w[own] = 0.f;  // :1722
    if (g.nz < 2) return;
    const double mapRatioX = (double)g.distX[c] / g.dx, mapRatioY = (double)g.distY[c] / g.dy;  // :1643-1647
    const double rhx = 1 / mapRatioX, rhy = 1 / mapRatioY, rhxy = rhx * rhy;
    const double cx = rhx * g.rdx_2, cy = rhy * g.rdy_2;
    const Neighbour left{(double)g.ps[c - 1], (double)g.distY[c - 1] / g.dy}, right{(double)g.ps[c + 1], (double)g.distY[c + 1] / g.dy};
    const Neighbour up{(double)g.ps[c - nx], (double)g.distX[c - nx] / g.dx}, down{(double)g.ps[c + nx], (double)g.distX[c + nx] / g.dx};
    const double ps = (double)g.ps[c];
    double sum = 0;  // :1721
    unsigned k = 1;
    for (; k + kAhead <= g.nz; k += kAhead) velocity_levels<kAhead>(g, c, own, k, ps, rhxy, cx, cy, left, right, up, down, sum);
    for (; k < g.nz; ++k) velocity_levels<1>(g, c, own, k, ps, rhxy, cx, cy, left, right, up, down, sum);
}

// mifi_omega_to_vertical_wind_f (src/vertical_coordinate_transformations.c:195-209) as an Op of convert_kernel's kind: the level
// pressure is Column::level(k), what verticalData4D(...)->asFloat() holds (CDMPressureConversions.cc:417-427)
template <int kKind>
__global__ void __launch_bounds__(kBlock) omega_kernel(const Levels levels, size_t plane, const float* omega, const float* __restrict__ t, float* w)
{
    constexpr int kU = 4;
    const float mR_g = (float)(-(8.31432 / (kEarthGravity * 0.0289644)));  // (float)-BAROMETRIC_FACTOR, :202
    const size_t cell = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= plane) return;
    Levels L = levels;
    L.kind = kKind;
    const unsigned nz = L.nz;
    const Column col(L, blockIdx.y, cell, plane);
    const size_t base = (size_t)blockIdx.y * nz * plane + cell;
    unsigned k = 0;
    for (; k + kU <= nz; k += kU) {  // omega may be w: a lane reads its own elements of a group before it writes them
        float o[kU], T[kU], p[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            o[u] = omega[base + (size_t)(k + u) * plane];
            T[u] = t[base + (size_t)(k + u) * plane];
            p[u] = col.level(k + u);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) w[base + (size_t)(k + u) * plane] = mR_g * o[u] * T[u] / p[u];
    }
    for (; k < nz; ++k) w[base + (size_t)k * plane] = mR_g * omega[base + (size_t)k * plane] * t[base + (size_t)k * plane] / col.level(k);
}

}  // namespace

// every argument has been checked (capi.hip)
void launch_griddistance(size_t nx, size_t ny, const double* d_lon, const double* d_lat, float* d_distX, float* d_distY, hipStream_t stream)
{
    const size_t n = nx * ny;
    if (n == 1) {  // :1542-1545; the caller reports the reference's MIFI_ERROR
        FA_HIP(hipMemsetAsync(d_distX, 0, sizeof(float), stream));
        FA_HIP(hipMemsetAsync(d_distY, 0, sizeof(float), stream));
        return;
    }
    FA_REQUIRE(ceil_div(n, kBlock) <= 0x7fffffffu, "horizontal plane too large");
    griddistance_kernel<<<(unsigned)ceil_div(n, kBlock), kBlock, 0, stream>>>(nx, ny, d_lon, d_lat, d_distX, d_distY);
    FA_HIP(hipGetLastError());
}

void launch_vertical_velocity(size_t nx, size_t ny, size_t nz, size_t nt, double dx, double dy, const float* d_distX, const float* d_distY,
                              const double* h_ap, const double* h_b, const float* d_zs, const float* d_ps, const float* d_u, const float* d_v,
                              const float* d_t, float* d_w, hipStream_t stream)
{
    const size_t plane = nx * ny;
    FA_REQUIRE(nx <= 0x7fffffffu && ny <= (size_t)65535 * kTileY && nz < 0x7fffffffu, "grid too large");
    FA_REQUIRE(ceil_div(plane, kBlock) <= 0x7fffffffu, "horizontal plane too large");
    std::vector<double> ah(nz + 1), bh(nz + 1);  // :1653-1663, in the reference's order
    ah[0] = 0.0;
    bh[0] = 0.0;
    ah[nz] = 0.0;
    bh[nz] = 1.0;
    for (size_t k = nz - 1; k > 0; --k) {
        ah[k] = 2.0 * h_ap[k] - ah[k + 1];
        bh[k] = 2.0 * h_b[k] - bh[k + 1];
    }
    StreamScratch scratch(2 * (nz + 1) + (nz - 1) * plane, stream);
    VelocityArgs g{};
    g.nx = (unsigned)nx;
    g.ny = (unsigned)ny;
    g.nz = (unsigned)nz;
    g.plane = plane;
    g.dx = dx;
    g.dy = dy;
    g.rdx_2 = 1 / (2 * dx);  // :1635-1636
    g.rdy_2 = 1 / (2 * dy);
    g.distX = d_distX;
    g.distY = d_distY;
    g.zs = d_zs;
    double* d_ah = scratch.take(nz + 1);
    double* d_bh = scratch.take(nz + 1);
    upload(d_ah, ah.data(), nz + 1, stream);
    upload(d_bh, bh.data(), nz + 1, stream);
    g.ah = d_ah;
    g.bh = d_bh;
    g.z = scratch.take((nz - 1) * plane);
    const dim3 tiles((unsigned)ceil_div(nx, kTileX), (unsigned)ceil_div(ny, kTileY), 1);
    for (size_t t = 0; t < nt; ++t) {
        g.ps = d_ps + t * plane;
        g.u = d_u + t * nz * plane;
        g.v = d_v + t * nz * plane;
        g.t = d_t + t * nz * plane;
        g.w = d_w + t * nz * plane;
        if (nz > 1) hydrostatic_kernel<<<(unsigned)ceil_div(plane, kBlock), kBlock, 0, stream>>>(g);
        velocity_kernel<<<tiles, dim3(kTileX, kTileY, 1), 0, stream>>>(g);
    }
    FA_HIP(hipGetLastError());
}

void launch_omega_to_vertical_wind(const fimex_amd_vertical_levels& pressure, size_t nx, size_t ny, size_t nt, const float* d_omega,
                                   const float* d_t, float* d_w, hipStream_t stream)
{
    const size_t plane = nx * ny;
    if (plane == 0 || nt == 0 || pressure.nz == 0) return;
    const dim3 grid = column_grid(plane, nt);
    StreamScratch scratch(coefficient_count(pressure), stream);
    const Levels L = device_levels(pressure, scratch, stream);
    switch (pressure.kind) {
    case FIMEX_AMD_VLEVEL_FIELD: omega_kernel<FIMEX_AMD_VLEVEL_FIELD><<<grid, kBlock, 0, stream>>>(L, plane, d_omega, d_t, d_w); break;
    case FIMEX_AMD_VLEVEL_AXIS: omega_kernel<FIMEX_AMD_VLEVEL_AXIS><<<grid, kBlock, 0, stream>>>(L, plane, d_omega, d_t, d_w); break;
    case FIMEX_AMD_VLEVEL_SIGMA: omega_kernel<FIMEX_AMD_VLEVEL_SIGMA><<<grid, kBlock, 0, stream>>>(L, plane, d_omega, d_t, d_w); break;
    case FIMEX_AMD_VLEVEL_HYBRID_SIGMA: omega_kernel<FIMEX_AMD_VLEVEL_HYBRID_SIGMA><<<grid, kBlock, 0, stream>>>(L, plane, d_omega, d_t, d_w); break;
    default: omega_kernel<FIMEX_AMD_VLEVEL_HYBRID_SIGMA_AP><<<grid, kBlock, 0, stream>>>(L, plane, d_omega, d_t, d_w); break;
    }
    FA_HIP(hipGetLastError());
}

}  // namespace fimex_amd
