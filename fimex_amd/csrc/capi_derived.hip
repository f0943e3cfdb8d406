// extern "C" boundary, derived data (8f n9): the scaled conversion between stored types (scaled_convert.hip), theta2T and
// specific2relative on a level description (pressure_convert.hip), accumulate / deaccumulate (time_accumulate.hip).  Each entry
// pair is one template over the call type (host_call.hpp).
#include "capi_checks.hpp"
#include "host_call.hpp"

#include "../../include/fimex_amd_derived_host.h"

using namespace fimex_amd;

namespace {

// The byte counts below are plain size_t products, as in the other capi_*.hip files: sizes whose product wraps are not refused.

template <class Call>
void convert_scaled(Call&& c, const void* in, int inType, size_t n, double oldFill, double oldScale, double oldOffset, int outType, double newFill,
                    double newScale, double newOffset, void* out)
{
    const size_t inBytes = n * cdm_type_size(inType), outBytes = n * cdm_type_size(outType);  // throws for NAT and STRING
    FA_REQUIRE(scaled_fill_representable(outType, newFill), "newFill " + std::to_string(newFill) + " is not representable in the output type");
    if (n == 0) return;
    FA_REQUIRE(in != nullptr && out != nullptr, "NULL data buffer");
    if (out != in || inBytes != outBytes) require_no_overlap(out, outBytes, {{in, inBytes, "the input buffer (in place needs types of one size)"}});
    (void)current_device_checked();
    launch_convert_scaled(c.in_bytes(in, inBytes), inType, n, oldFill, oldScale, oldOffset, outType, newFill, newScale, newOffset,
                          c.out_bytes(out, outBytes), c.stream());
    c.finish();
}

// false: nothing to do
bool check_pressure_call(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt)
{
    const bool nonEmpty = nx * ny * nt > 0;
    check_vertical_levels(pressure, "pressure", nonEmpty);
    if (!nonEmpty) return false;
    FA_REQUIRE(pressure->nz > 0, "no levels (nz == 0)");
    return true;
}

// host form: the copy of theta is converted in place, as the reference does, and lands in T
template <class Call>
void theta_to_temperature(Call&& c, const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* theta, float addOffset,
                          float* T)
{
    if (!check_pressure_call(pressure, nx, ny, nt)) return;
    FA_REQUIRE(theta != nullptr, "NULL potential temperature");
    FA_REQUIRE(T != nullptr, "NULL output buffer");
    const size_t plane = nx * ny, cells = plane * nt, vol = cells * pressure->nz;
    if (T != theta) require_no_overlap(T, vol * sizeof(float), {{theta, vol * sizeof(float), "theta (other than in place)"}});
    require_no_overlap_with_levels(T, vol * sizeof(float), *pressure, cells);
    (void)current_device_checked();
    const fimex_amd_vertical_levels l = levels_on(c, *pressure, plane, nt);
    const Through<float> th = c.through(theta, T, vol);
    launch_theta_to_temperature(l, nx, ny, nt, th.in, addOffset, th.out, c.stream());
    c.finish();
}

template <class Call>
void specific_to_relative_humidity(Call&& c, const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* q,
                                   const float* T, short* rh)
{
    if (!check_pressure_call(pressure, nx, ny, nt)) return;
    FA_REQUIRE(q != nullptr, "NULL specific humidity");
    FA_REQUIRE(T != nullptr, "NULL air temperature");
    FA_REQUIRE(rh != nullptr, "NULL output buffer");
    const size_t plane = nx * ny, cells = plane * nt, vol = cells * pressure->nz;
    require_no_overlap(rh, vol * sizeof(short), {{q, vol * sizeof(float), "the specific humidity"}, {T, vol * sizeof(float), "the air temperature"}});
    require_no_overlap_with_levels(rh, vol * sizeof(short), *pressure, cells);
    (void)current_device_checked();
    const fimex_amd_vertical_levels l = levels_on(c, *pressure, plane, nt);
    launch_specific_to_relative_humidity(l, nx, ny, nt, c.in(q, vol), c.in(T, vol), c.out(rh, vol), c.stream());
    c.finish();
}

// prevBytes: the size of an element of prev (a double for accumulate, the stored type for deaccumulate)
template <class Call>
void along_time(Call&& c, bool accumulate, const void* in, int cdmType, size_t n, size_t nt, size_t firstPos, const void* prev, double* out)
{
    const size_t elem = cdm_type_size(cdmType), prevBytes = n * (accumulate ? sizeof(double) : elem);
    if (n == 0 || nt == 0) return;
    FA_REQUIRE(in != nullptr && out != nullptr, "NULL data buffer");
    FA_REQUIRE(firstPos == 0 || prev != nullptr, "a batch that starts behind position 0 needs prev, the position in front of it");
    if (firstPos == 0) prev = nullptr;
    require_no_overlap(out, n * nt * sizeof(double), {{in, n * nt * elem, "the input buffer"}, {prev, prevBytes, "prev"}});
    (void)current_device_checked();
    const void* d_in = c.in_bytes(in, n * nt * elem);
    const void* d_prev = prev ? c.in_bytes(prev, prevBytes) : nullptr;
    double* d_out = c.out(out, n * nt);
    if (accumulate) launch_accumulate(d_in, cdmType, n, nt, firstPos, static_cast<const double*>(d_prev), d_out, c.stream());
    else launch_deaccumulate(d_in, cdmType, n, nt, firstPos, d_prev, d_out, c.stream());
    c.finish();
}

}  // namespace

extern "C" {

int fimex_amd_convert_scaled_device(const void* d_in, int inType, size_t n, double oldFill, double oldScale, double oldOffset, int outType,
                                    double newFill, double newScale, double newOffset, void* d_out, void* stream)
{
    return c_guard([&] {
        convert_scaled(DeviceCall{as_stream(stream)}, d_in, inType, n, oldFill, oldScale, oldOffset, outType, newFill, newScale, newOffset, d_out);
    });
}

int fimex_amd_convert_scaled_host(const void* in, int inType, size_t n, double oldFill, double oldScale, double oldOffset, int outType,
                                  double newFill, double newScale, double newOffset, void* out)
{
    return c_guard([&] { convert_scaled(HostCall(), in, inType, n, oldFill, oldScale, oldOffset, outType, newFill, newScale, newOffset, out); });
}

int fimex_amd_theta_to_temperature_device(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* d_theta,
                                          float addOffset, float* d_T, void* stream)
{
    return c_guard([&] { theta_to_temperature(DeviceCall{as_stream(stream)}, pressure, nx, ny, nt, d_theta, addOffset, d_T); });
}

int fimex_amd_theta_to_temperature_host(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* theta,
                                        float addOffset, float* T)
{
    return c_guard([&] { theta_to_temperature(HostCall(), pressure, nx, ny, nt, theta, addOffset, T); });
}

int fimex_amd_specific_to_relative_humidity_device(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* d_q,
                                                   const float* d_T, short* d_rh, void* stream)
{
    return c_guard([&] { specific_to_relative_humidity(DeviceCall{as_stream(stream)}, pressure, nx, ny, nt, d_q, d_T, d_rh); });
}

int fimex_amd_specific_to_relative_humidity_host(const fimex_amd_vertical_levels* pressure, size_t nx, size_t ny, size_t nt, const float* q,
                                                 const float* T, short* rh)
{
    return c_guard([&] { specific_to_relative_humidity(HostCall(), pressure, nx, ny, nt, q, T, rh); });
}

int fimex_amd_accumulate_device(const void* d_in, int cdmType, size_t n, size_t nt, size_t firstPos, const double* d_prev, double* d_out,
                                void* stream)
{
    return c_guard([&] { along_time(DeviceCall{as_stream(stream)}, true, d_in, cdmType, n, nt, firstPos, d_prev, d_out); });
}

int fimex_amd_accumulate_host(const void* in, int cdmType, size_t n, size_t nt, size_t firstPos, const double* prev, double* out)
{
    return c_guard([&] { along_time(HostCall(), true, in, cdmType, n, nt, firstPos, prev, out); });
}

int fimex_amd_deaccumulate_device(const void* d_in, int cdmType, size_t n, size_t nt, size_t firstPos, const void* d_prev, double* d_out,
                                  void* stream)
{
    return c_guard([&] { along_time(DeviceCall{as_stream(stream)}, false, d_in, cdmType, n, nt, firstPos, d_prev, d_out); });
}

int fimex_amd_deaccumulate_host(const void* in, int cdmType, size_t n, size_t nt, size_t firstPos, const void* prev, double* out)
{
    return c_guard([&] { along_time(HostCall(), false, in, cdmType, n, nt, firstPos, prev, out); });
}

}  // extern "C"
