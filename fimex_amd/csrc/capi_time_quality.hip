// extern "C" boundary, time axis and quality mask (8f n10): the slice mapping of CDMTimeInterpolator on the host, a series onto a
// new time axis (time_interpolate.hip), the status rules of CDMQualityExtractor (quality.hip).  Each entry pair is one template
// over the call type (host_call.hpp).  Everything that can be refused without a device is refused before one is touched.
#include "capi_checks.hpp"
#include "host_call.hpp"

#include "../../include/fimex_amd_time_quality_host.h"

#include <algorithm>
#include <limits>
#include <vector>

using namespace fimex_amd;

namespace {

// The byte counts below are plain size_t products, as in the other capi_*.hip files: sizes whose product wraps are not refused.

// src/CDMTimeInterpolator.cc:161-188 on doubles
void time_mapping(const double* oldTimes, size_t nOld, const double* newTimes, size_t nNew, size_t* t1, size_t* t2)
{
    FA_REQUIRE(nOld > 0, "no old times (nOld == 0)");
    FA_REQUIRE(oldTimes != nullptr, "NULL old times");
    for (size_t i = 1; i < nOld; ++i)
        FA_REQUIRE(oldTimes[i - 1] < oldTimes[i], "the old times are not strictly ascending at position " + std::to_string(i));
    FA_REQUIRE(nOld > 1 || oldTimes[0] == oldTimes[0], "the old time is NaN");
    if (nNew == 0) return;
    FA_REQUIRE(newTimes != nullptr && t1 != nullptr && t2 != nullptr, "NULL new times or mapping");
    size_t lastPos = 0;
    for (size_t i = 0; i < nNew; ++i) {
        size_t pos = (size_t)(std::lower_bound(oldTimes + lastPos, oldTimes + nOld, newTimes[i]) - oldTimes);  // :167-168
        if (pos == nOld) pos--;  // extrapolation at the end, from the last two
        t2[i] = pos;
        if (pos != 0) {
            t1[i] = pos - 1;
        } else {  // extrapolation at the beginning
            t1[i] = pos;
            if (pos + 1 != nOld) t2[i] = pos + 1;
        }
        lastPos = pos;  // :185
    }
}

// f and the branch of mifi_get_values_linear_weak_extrapol_f it selects (blend_math.hpp)
TimeStep time_step(size_t t1, size_t t2, double a, double b, double x)
{
    const blend_math::Blend c = blend_math::classify(blend_math::kLinearWeakExtrapol, a, b, x);
    return TimeStep{(uint32_t)t1, (uint32_t)t2, c.f, c.cls};
}

template <class Call>
void time_interpolate(Call&& c, const void* in, int cdmType, size_t n, const double* oldTimes, size_t nOld, const double* newTimes, size_t nNew,
                      float* out)
{
    const size_t elem = cdm_type_size(cdmType);  // throws for NAT and STRING
    std::vector<size_t> t1(nNew), t2(nNew);
    time_mapping(oldTimes, nOld, newTimes, nNew, t1.data(), t2.data());
    if (n == 0 || nNew == 0) return;
    FA_REQUIRE(nOld <= std::numeric_limits<uint32_t>::max(), "more input slices than 32 bits count");
    FA_REQUIRE(in != nullptr && out != nullptr, "NULL data buffer");
    require_no_overlap(out, nNew * n * sizeof(float), {{in, nOld * n * elem, "the input buffer"}});
    std::vector<TimeStep> steps(nNew);
    for (size_t i = 0; i < nNew; ++i) steps[i] = time_step(t1[i], t2[i], oldTimes[t1[i]], oldTimes[t2[i]], newTimes[i]);
    (void)current_device_checked();
    launch_time_interpolate(c.in_bytes(in, nOld * n * elem), cdmType, n, steps.data(), nNew, c.out(out, nNew * n), c.stream());
    c.finish();
}

template <class Call>
void quality_mask(Call&& c, void* data, int dataType, size_t nData, const void* status, int statusType, size_t nStatus, int mode,
                  const double* values, size_t nValues, double limit, double validMin, double validMax, double statusFill, double fillValue)
{
    const size_t dataBytes = nData * cdm_type_size(dataType), statusBytes = nStatus * cdm_type_size(statusType);  // throws for NAT and STRING
    FA_REQUIRE(quality_mode_known(mode), "unknown quality mode " + std::to_string(mode));
    std::vector<double> sorted;
    if (mode == FIMEX_AMD_QUALITY_VALUES) {
        FA_REQUIRE(nValues > 0 && values != nullptr, "no status values to keep");
        sorted.assign(values, values + nValues);
        for (double v : sorted) FA_REQUIRE(v == v, "NaN among the status values");
        std::sort(sorted.begin(), sorted.end());  // src/CDMQualityExtractor.cc:287
    }
    FA_REQUIRE(quality_fill_representable(dataType, fillValue), "fillValue " + std::to_string(fillValue) + " is not representable in the data type");
    if (nData == 0) return;
    FA_REQUIRE(nStatus > 0 && nData % nStatus == 0, "incompatible sizes of data and status: " + std::to_string(nData) + " <> " + std::to_string(nStatus));
    FA_REQUIRE(data != nullptr && status != nullptr, "NULL data or status buffer");
    const bool own = status == data;
    if (own) FA_REQUIRE(statusType == dataType && nStatus == nData, "the data as its own status needs one type and one size");
    else require_no_overlap(data, dataBytes, {{status, statusBytes, "the status (other than the data itself)"}});
    (void)current_device_checked();
    void* d_data = c.inout(static_cast<unsigned char*>(data), dataBytes);
    const void* d_status = own ? d_data : c.in_bytes(status, statusBytes);
    const QualityRule rule{mode, limit, validMin, validMax, statusFill, sorted.data(), sorted.size()};
    launch_quality_mask(d_data, dataType, nData, d_status, statusType, nStatus, rule, fillValue, c.stream());
    c.finish();
}

}  // namespace

extern "C" {

int fimex_amd_time_mapping(const double* oldTimes, size_t nOld, const double* newTimes, size_t nNew, size_t* t1, size_t* t2)
{
    return c_guard([&] { time_mapping(oldTimes, nOld, newTimes, nNew, t1, t2); });
}

int fimex_amd_time_interpolate_device(const void* d_in, int cdmType, size_t n, const double* oldTimes, size_t nOld, const double* newTimes,
                                      size_t nNew, float* d_out, void* stream)
{
    return c_guard([&] { time_interpolate(DeviceCall{as_stream(stream)}, d_in, cdmType, n, oldTimes, nOld, newTimes, nNew, d_out); });
}

int fimex_amd_time_interpolate_host(const void* in, int cdmType, size_t n, const double* oldTimes, size_t nOld, const double* newTimes, size_t nNew,
                                    float* out)
{
    return c_guard([&] { time_interpolate(HostCall(), in, cdmType, n, oldTimes, nOld, newTimes, nNew, out); });
}

int fimex_amd_quality_mask_device(void* d_data, int dataType, size_t nData, const void* d_status, int statusType, size_t nStatus, int mode,
                                  const double* values, size_t nValues, double limit, double validMin, double validMax, double statusFill,
                                  double fillValue, void* stream)
{
    return c_guard([&] {
        quality_mask(DeviceCall{as_stream(stream)}, d_data, dataType, nData, d_status, statusType, nStatus, mode, values, nValues, limit, validMin,
                     validMax, statusFill, fillValue);
    });
}

int fimex_amd_quality_mask_host(void* data, int dataType, size_t nData, const void* status, int statusType, size_t nStatus, int mode,
                                const double* values, size_t nValues, double limit, double validMin, double validMax, double statusFill,
                                double fillValue)
{
    return c_guard([&] {
        quality_mask(HostCall(), data, dataType, nData, status, statusType, nStatus, mode, values, nValues, limit, validMin, validMax, statusFill,
                     fillValue);
    });
}

}  // extern "C"
