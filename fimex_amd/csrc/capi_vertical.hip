// extern "C" boundary, vertical: interpolation (vertical.hip), the level converters (vertical_levels.hip), grid distances and
// vertical velocity (vertical_velocity.hip).  Each entry pair is one template over the call type (host_call.hpp).
#include "capi_checks.hpp"
#include "host_call.hpp"

using namespace fimex_amd;

namespace {

// ---- vertical interpolation

// everything fimex_amd_vertical_interpolate_* refuses before any work is queued; returns false when there is nothing to do
bool check_vertical_call(int method, size_t nx, size_t ny, size_t nt, const void* in, const fimex_amd_vertical_levels* inLevels,
                         const fimex_amd_vertical_levels* outLevels, const double* level1, size_t nzo, const void* out)
{
    if (!check_vertical_search(method, nx, ny, nt, inLevels, outLevels, level1, nzo, true)) return false;
    FA_REQUIRE(in != nullptr && out != nullptr, "NULL data buffer");
    const char *i0 = static_cast<const char*>(in), *o0 = static_cast<const char*>(out);
    const size_t cells = nx * ny * nt * sizeof(float);
    FA_REQUIRE(o0 + cells * nzo <= i0 || i0 + cells * inLevels->nz <= o0, "the output buffer overlaps the input buffer");
    return true;
}

template <class Call>
void vertical_interpolate(Call&& c, int method, size_t nx, size_t ny, size_t nt, const float* in, const fimex_amd_vertical_levels* inLevels,
                          const fimex_amd_vertical_levels* outLevels, const double* level1, size_t nzo, const double* validMin,
                          const double* validMax, float clampMin, float clampMax, float* out)
{
    if (!check_vertical_call(method, nx, ny, nt, in, inLevels, outLevels, level1, nzo, out)) return;
    (void)current_device_checked();
    const size_t plane = nx * ny;
    const fimex_amd_vertical_levels li = levels_on(c, *inLevels, plane, nt);
    fimex_amd_vertical_levels lo{};
    if (outLevels) lo = levels_on(c, *outLevels, plane, nt);
    launch_vertical_interpolate(method, nx, ny, nt, c.in(in, nt * inLevels->nz * plane), li, outLevels ? &lo : nullptr, level1, nzo,
                                c.in(validMin, plane), c.in(validMax, plane), clampMin, clampMax, c.out(out, nt * nzo * plane), c.stream());
    c.finish();
}

template <class Call>
void vertical_levels(Call&& c, const fimex_amd_vertical_levels* levels, size_t nx, size_t ny, size_t nt, float* out, const char* nullOut)
{
    const bool nonEmpty = nx * ny * nt > 0;
    check_vertical_levels(levels, "the", nonEmpty);
    if (!nonEmpty || levels->nz == 0) return;
    FA_REQUIRE(out != nullptr, nullOut);
    (void)current_device_checked();
    const fimex_amd_vertical_levels l = levels_on(c, *levels, nx * ny, nt);
    launch_vertical_levels(l, nx, ny, nt, c.out(out, nt * levels->nz * nx * ny), c.stream());
    c.finish();
}

// ---- vertical level converters

// false: nothing to do
bool check_altitude_call(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* T, const float* q,
                         const float* sap, const float* sgp, int surfaceFirst, const double* topo, const float* out)
{
    FA_REQUIRE(vertical_order_known(surfaceFirst), "unknown surfaceFirst " + std::to_string(surfaceFirst) + " (1, 0 or -1 for the reference's rule)");
    const bool nonEmpty = nx * ny * nt > 0;
    check_vertical_levels(pressure, "pressure", nonEmpty);
    if (!nonEmpty) return false;
    FA_REQUIRE(pressure->nz > 0, "no levels (nz == 0)");
    FA_REQUIRE(T != nullptr, "NULL air temperature");
    FA_REQUIRE(sap != nullptr, "NULL surface pressure");
    FA_REQUIRE(sgp != nullptr, "NULL surface geopotential");
    FA_REQUIRE(out != nullptr, "NULL output buffer");
    const size_t cells = nx * ny * nt, vol = cells * pressure->nz * sizeof(float);
    require_no_overlap(out, vol, {{T, vol, "the air temperature"}, {q, vol, "the specific humidity"},
                                  {sap, cells * sizeof(float), "the surface pressure"}, {sgp, cells * sizeof(float), "the surface geopotential"},
                                  {topo, nx * ny * sizeof(double), "the topography"}});
    require_no_overlap_with_levels(out, vol, *pressure, cells);
    return true;
}

bool check_standard_call(const fimex_amd_vertical_levels* levels, const char* which, size_t nx, size_t ny, size_t nt, const double* topo,
                         const float* out)
{
    const bool nonEmpty = nx * ny * nt > 0;
    check_vertical_levels(levels, which, nonEmpty);
    if (!nonEmpty) return false;
    FA_REQUIRE(levels->nz > 0, "no levels (nz == 0)");
    FA_REQUIRE(out != nullptr, "NULL output buffer");
    const size_t cells = nx * ny * nt, vol = cells * levels->nz * sizeof(float);
    require_no_overlap(out, vol, {{topo, nx * ny * sizeof(double), "the topography"}});
    require_no_overlap_with_levels(out, vol, *levels, cells);
    return true;
}

bool check_ocean_call(int generation, size_t nx, size_t ny, size_t nz, size_t nt, const double* s, const double* C, const double* depth,
                      const double* eta, const float* out)
{
    FA_REQUIRE(generation == 1 || generation == 2, "unknown ocean s-coordinate generation " + std::to_string(generation) + " (1 or 2)");
    FA_REQUIRE(nz <= 0x7fffffffu, "nz out of range");
    if (nx * ny * nt == 0) return false;
    FA_REQUIRE(nz > 0, "no levels (nz == 0)");
    FA_REQUIRE(s != nullptr && C != nullptr, "NULL s[nz] or C[nz]");
    FA_REQUIRE(depth != nullptr, "NULL depth");
    FA_REQUIRE(out != nullptr, "NULL output buffer");
    require_no_overlap(out, nx * ny * nt * nz * sizeof(float), {{depth, nx * ny * sizeof(double), "the depth"},
                                                                {eta, nx * ny * nt * sizeof(double), "eta"}});
    return true;
}

template <class Call>
void altitude_integrate(Call&& c, const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* airTemperature,
                        const float* specificHumidity, const float* surfacePressure, const float* surfaceGeopotential, int surfaceFirst,
                        const double* topo, double topoFactor, float* out)
{
    if (!check_altitude_call(pressure, nx, ny, nt, airTemperature, specificHumidity, surfacePressure, surfaceGeopotential, surfaceFirst, topo,
                             out))
        return;
    (void)current_device_checked();
    const size_t plane = nx * ny, vol = nt * pressure->nz * plane;
    const fimex_amd_vertical_levels l = levels_on(c, *pressure, plane, nt);
    launch_vertical_altitude(l, nx, ny, nt, c.in(airTemperature, vol), c.in(specificHumidity, vol), c.in(surfacePressure, nt * plane),
                             c.in(surfaceGeopotential, nt * plane), surfaceFirst, c.in(topo, plane), topoFactor, c.out(out, vol), c.stream());
    c.finish();
}

template <class Call>
void standard(Call&& c, bool toPressure, const fimex_amd_vertical_levels* levels, size_t nx, size_t ny, size_t nt, const double* topo,
              double topoFactor, float* out)
{
    if (!check_standard_call(levels, toPressure ? "altitude" : "pressure", nx, ny, nt, topo, out)) return;
    (void)current_device_checked();
    const size_t plane = nx * ny;
    const fimex_amd_vertical_levels l = levels_on(c, *levels, plane, nt);
    launch_vertical_standard(toPressure, l, nx, ny, nt, c.in(topo, plane), topoFactor, c.out(out, nt * levels->nz * plane), c.stream());
    c.finish();
}

template <class Call>
void ocean_depth(Call&& c, int generation, size_t nx, size_t ny, size_t nz, size_t nt, const double* s, const double* C, double depth_c,
                 const double* depth, const double* eta, float* out)
{
    if (!check_ocean_call(generation, nx, ny, nz, nt, s, C, depth, eta, out)) return;
    (void)current_device_checked();
    const size_t plane = nx * ny;
    launch_vertical_ocean_depth(generation, nx, ny, nz, nt, s, C, depth_c, c.in(depth, plane), c.in(eta, nt * plane),
                                c.out(out, nt * nz * plane), c.stream());
    c.finish();
}

// ---- vertical velocity on model levels

// true: the reference's "no grid" case of one point, which writes zeros and returns MIFI_ERROR
bool check_griddistance_call(size_t nx, size_t ny, const double* lon, const double* lat, const float* distX, const float* distY)
{
    FA_REQUIRE(nx > 0 && ny > 0, "empty grid (nx * ny == 0)");
    FA_REQUIRE(lon != nullptr && lat != nullptr, "NULL longitude or latitude");
    FA_REQUIRE(distX != nullptr && distY != nullptr, "NULL output buffer");
    const size_t n = nx * ny;
    FA_REQUIRE(distX + n <= distY || distY + n <= distX, "gridDistX overlaps gridDistY");
    for (const float* out : {distX, distY})
        require_no_overlap(out, n * sizeof(float), {{lon, n * sizeof(double), "the longitudes"}, {lat, n * sizeof(double), "the latitudes"}});
    return n == 1;
}

void check_velocity_call(size_t nx, size_t ny, size_t nz, size_t nt, const float* distX, const float* distY, const double* ap, const double* b,
                         const float* zs, const float* ps, const float* u, const float* v, const float* t, const float* w)
{
    // the reference reads outside its arrays on such grids
    FA_REQUIRE(nx >= 3 && ny >= 3, "the vertical velocity needs nx >= 3 and ny >= 3 (got " + std::to_string(nx) + " x " + std::to_string(ny) + ")");
    FA_REQUIRE(nz > 0, "no levels (nz == 0)");
    FA_REQUIRE(ap != nullptr && b != nullptr, "NULL ap[nz] or b[nz]");
    FA_REQUIRE(distX != nullptr && distY != nullptr, "NULL grid distance");
    FA_REQUIRE(nt == 0 || (zs != nullptr && ps != nullptr), "NULL orography or surface pressure");
    FA_REQUIRE(nt == 0 || (u != nullptr && v != nullptr && t != nullptr), "NULL wind or temperature");
    FA_REQUIRE(nt == 0 || w != nullptr, "NULL output buffer");
    const size_t plane = nx * ny, vol = nt * nz * plane * sizeof(float);
    require_no_overlap(w, vol, {{distX, plane * sizeof(float), "gridDistX"}, {distY, plane * sizeof(float), "gridDistY"},
                                {zs, plane * sizeof(float), "the orography"}, {ps, nt * plane * sizeof(float), "the surface pressure"},
                                {u, vol, "the x wind"}, {v, vol, "the y wind"}, {t, vol, "the air temperature"}});
}

// false: nothing to do
bool check_omega_call(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* omega, const float* t,
                      const float* w)
{
    const bool nonEmpty = nx * ny * nt > 0;
    check_vertical_levels(pressure, "pressure", nonEmpty);
    if (!nonEmpty) return false;
    FA_REQUIRE(pressure->nz > 0, "no levels (nz == 0)");
    FA_REQUIRE(omega != nullptr, "NULL omega");
    FA_REQUIRE(t != nullptr, "NULL air temperature");
    FA_REQUIRE(w != nullptr, "NULL output buffer");
    const size_t cells = nx * ny * nt, vol = cells * pressure->nz * sizeof(float);
    if (w != omega) require_no_overlap(w, vol, {{omega, vol, "omega (other than in place)"}});
    require_no_overlap(w, vol, {{t, vol, "the air temperature"}});
    require_no_overlap_with_levels(w, vol, *pressure, cells);
    return true;
}

// FIMEX_AMD_ERROR after the zeros are written for a grid of one point, as the reference returns MIFI_ERROR.  The one call that
// takes its HostCall from outside c_guard, for the sake of that return value: the temporary's destructor (a wait and hipFree,
// neither of which throws) runs after the guard has returned.
template <class Call>
int griddistance(Call&& c, size_t nx, size_t ny, const double* lon, const double* lat, float* gridDistX, float* gridDistY)
{
    bool noGrid = false;
    const int rc = c_guard([&] {
        noGrid = check_griddistance_call(nx, ny, lon, lat, gridDistX, gridDistY);
        (void)current_device_checked();
        const size_t n = nx * ny;
        launch_griddistance(nx, ny, c.in(lon, n), c.in(lat, n), c.out(gridDistX, n), c.out(gridDistY, n), c.stream());
        c.finish();
        if (noGrid) set_last_error("a grid of one point has no grid distance: zeros written");
    });
    return noGrid ? FIMEX_AMD_ERROR : rc;
}

template <class Call>
void vertical_velocity(Call&& c, size_t nx, size_t ny, size_t nz, size_t nt, double dx, double dy, const float* gridDistX,
                       const float* gridDistY, const double* ap, const double* b, const float* zs, const float* ps, const float* u,
                       const float* v, const float* t, float* w)
{
    check_velocity_call(nx, ny, nz, nt, gridDistX, gridDistY, ap, b, zs, ps, u, v, t, w);
    if (nt == 0) return;
    (void)current_device_checked();
    const size_t plane = nx * ny, vol = nt * nz * plane;
    launch_vertical_velocity(nx, ny, nz, nt, dx, dy, c.in(gridDistX, plane), c.in(gridDistY, plane), ap, b, c.in(zs, plane),
                             c.in(ps, nt * plane), c.in(u, vol), c.in(v, vol), c.in(t, vol), c.out(w, vol), c.stream());
    c.finish();
}

// host form: the copy of omega is converted in place, as the reference does, and lands in w
template <class Call>
void omega_to_vertical_wind(Call&& c, const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* omega,
                            const float* t, float* w)
{
    if (!check_omega_call(pressure, nx, ny, nt, omega, t, w)) return;
    (void)current_device_checked();
    const size_t plane = nx * ny, vol = nt * pressure->nz * plane;
    const fimex_amd_vertical_levels l = levels_on(c, *pressure, plane, nt);
    const Through<float> o = c.through(omega, w, vol);
    launch_omega_to_vertical_wind(l, nx, ny, nt, o.in, c.in(t, vol), o.out, c.stream());
    c.finish();
}

}  // namespace

extern "C" {

int fimex_amd_vertical_interpolate_device(int method, size_t nx, size_t ny, size_t nt, const float* d_in,
                                          const fimex_amd_vertical_levels* inLevels, const fimex_amd_vertical_levels* outLevels,
                                          const double* level1, size_t nzo, const double* d_validMin, const double* d_validMax,
                                          float clampMin, float clampMax, float* d_out, void* stream)
{
    return c_guard([&] {
        vertical_interpolate(DeviceCall{as_stream(stream)}, method, nx, ny, nt, d_in, inLevels, outLevels, level1, nzo, d_validMin, d_validMax,
                             clampMin, clampMax, d_out);
    });
}

int fimex_amd_vertical_interpolate_host(int method, size_t nx, size_t ny, size_t nt, const float* in,
                                        const fimex_amd_vertical_levels* inLevels, const fimex_amd_vertical_levels* outLevels,
                                        const double* level1, size_t nzo, const double* validMin, const double* validMax,
                                        float clampMin, float clampMax, float* out)
{
    return c_guard([&] {
        vertical_interpolate(HostCall(), method, nx, ny, nt, in, inLevels, outLevels, level1, nzo, validMin, validMax, clampMin, clampMax, out);
    });
}

int fimex_amd_vertical_levels_device(const fimex_amd_vertical_levels* levels, size_t nx, size_t ny, size_t nt, float* d_out, void* stream)
{
    return c_guard([&] { vertical_levels(DeviceCall{as_stream(stream)}, levels, nx, ny, nt, d_out, "NULL device buffer"); });
}

int fimex_amd_vertical_levels_host(const fimex_amd_vertical_levels* levels, size_t nx, size_t ny, size_t nt, float* out)
{
    return c_guard([&] { vertical_levels(HostCall(), levels, nx, ny, nt, out, "NULL argument"); });
}

int fimex_amd_vertical_altitude_integrate_device(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt,
                                                 const float* d_airTemperature, const float* d_specificHumidity,
                                                 const float* d_surfacePressure, const float* d_surfaceGeopotential, int surfaceFirst,
                                                 const double* d_topo, double topoFactor, float* d_out, void* stream)
{
    return c_guard([&] {
        altitude_integrate(DeviceCall{as_stream(stream)}, pressure, nx, ny, nt, d_airTemperature, d_specificHumidity, d_surfacePressure,
                           d_surfaceGeopotential, surfaceFirst, d_topo, topoFactor, d_out);
    });
}

int fimex_amd_vertical_altitude_integrate_host(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt,
                                               const float* airTemperature, const float* specificHumidity, const float* surfacePressure,
                                               const float* surfaceGeopotential, int surfaceFirst, const double* topo, double topoFactor,
                                               float* out)
{
    return c_guard([&] {
        altitude_integrate(HostCall(), pressure, nx, ny, nt, airTemperature, specificHumidity, surfacePressure, surfaceGeopotential, surfaceFirst,
                           topo, topoFactor, out);
    });
}

int fimex_amd_vertical_standard_altitude_device(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt,
                                                const double* d_topo, double topoFactor, float* d_out, void* stream)
{
    return c_guard([&] { standard(DeviceCall{as_stream(stream)}, false, pressure, nx, ny, nt, d_topo, topoFactor, d_out); });
}

int fimex_amd_vertical_standard_altitude_host(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const double* topo,
                                              double topoFactor, float* out)
{
    return c_guard([&] { standard(HostCall(), false, pressure, nx, ny, nt, topo, topoFactor, out); });
}

int fimex_amd_vertical_standard_pressure_device(const fimex_amd_vertical_levels* altitude, size_t nx, size_t ny, size_t nt,
                                                const double* d_topo, double topoFactor, float* d_out, void* stream)
{
    return c_guard([&] { standard(DeviceCall{as_stream(stream)}, true, altitude, nx, ny, nt, d_topo, topoFactor, d_out); });
}

int fimex_amd_vertical_standard_pressure_host(const fimex_amd_vertical_levels* altitude, size_t nx, size_t ny, size_t nt, const double* topo,
                                              double topoFactor, float* out)
{
    return c_guard([&] { standard(HostCall(), true, altitude, nx, ny, nt, topo, topoFactor, out); });
}

int fimex_amd_vertical_ocean_depth_device(int generation, size_t nx, size_t ny, size_t nz, size_t nt, const double* s, const double* C,
                                          double depth_c, const double* d_depth, const double* d_eta, float* d_out, void* stream)
{
    return c_guard([&] { ocean_depth(DeviceCall{as_stream(stream)}, generation, nx, ny, nz, nt, s, C, depth_c, d_depth, d_eta, d_out); });
}

int fimex_amd_vertical_ocean_depth_host(int generation, size_t nx, size_t ny, size_t nz, size_t nt, const double* s, const double* C,
                                        double depth_c, const double* depth, const double* eta, float* out)
{
    return c_guard([&] { ocean_depth(HostCall(), generation, nx, ny, nz, nt, s, C, depth_c, depth, eta, out); });
}

int fimex_amd_griddistance_device(size_t nx, size_t ny, const double* d_lon, const double* d_lat, float* d_gridDistX, float* d_gridDistY,
                                  void* stream)
{
    return griddistance(DeviceCall{as_stream(stream)}, nx, ny, d_lon, d_lat, d_gridDistX, d_gridDistY);
}

int fimex_amd_griddistance_host(size_t nx, size_t ny, const double* lon, const double* lat, float* gridDistX, float* gridDistY)
{
    return griddistance(HostCall(), nx, ny, lon, lat, gridDistX, gridDistY);
}

int fimex_amd_vertical_velocity_device(size_t nx, size_t ny, size_t nz, size_t nt, double dx, double dy, const float* d_gridDistX,
                                       const float* d_gridDistY, const double* ap, const double* b, const float* d_zs, const float* d_ps,
                                       const float* d_u, const float* d_v, const float* d_t, float* d_w, void* stream)
{
    return c_guard([&] {
        vertical_velocity(DeviceCall{as_stream(stream)}, nx, ny, nz, nt, dx, dy, d_gridDistX, d_gridDistY, ap, b, d_zs, d_ps, d_u, d_v, d_t, d_w);
    });
}

int fimex_amd_vertical_velocity_host(size_t nx, size_t ny, size_t nz, size_t nt, double dx, double dy, const float* gridDistX,
                                     const float* gridDistY, const double* ap, const double* b, const float* zs, const float* ps, const float* u,
                                     const float* v, const float* t, float* w)
{
    return c_guard([&] { vertical_velocity(HostCall(), nx, ny, nz, nt, dx, dy, gridDistX, gridDistY, ap, b, zs, ps, u, v, t, w); });
}

int fimex_amd_omega_to_vertical_wind_device(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* d_omega,
                                            const float* d_t, float* d_w, void* stream)
{
    return c_guard([&] { omega_to_vertical_wind(DeviceCall{as_stream(stream)}, pressure, nx, ny, nt, d_omega, d_t, d_w); });
}

int fimex_amd_omega_to_vertical_wind_host(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* omega,
                                          const float* t, float* w)
{
    return c_guard([&] { omega_to_vertical_wind(HostCall(), pressure, nx, ny, nt, omega, t, w); });
}

}  // extern "C"
