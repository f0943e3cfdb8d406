// extern "C" boundary, extraction (8f n11): the plan of a reduction and its apply (extract.hip), the index arithmetic of reduceAxes
// on the host, the bounding box on the mesh of two axes (projection.hip).  The apply pair is one template over the call type
// (host_call.hpp).  Everything that can be refused without a device is refused before one is touched.
#include "capi_checks.hpp"
#include "extract.hpp"
#include "host_call.hpp"

#include "../../include/fimex_amd_extract_host.h"

#include <algorithm>
#include <memory>
#include <optional>
#include <sstream>
#include <vector>

using namespace fimex_amd;

namespace {

template <class Call>
void extract_apply(Call&& c, PlanDevice& dev, const fimex_amd_extract_plan* plan, const void* in, int cdmType, void* out)
{
    FA_REQUIRE(plan != nullptr, "NULL extract plan");
    const size_t elem = cdm_type_size(cdmType);  // throws for NAT and STRING
    if (plan->info.outElements == 0) return;
    FA_REQUIRE(in != nullptr && out != nullptr, "NULL data buffer");
    FA_REQUIRE(reinterpret_cast<uintptr_t>(in) % elem == 0 && reinterpret_cast<uintptr_t>(out) % elem == 0,
               "a data buffer is not aligned to its element size of " + std::to_string(elem) + " bytes");
    size_t inBytes = 0;
    FA_REQUIRE(!__builtin_mul_overflow(plan->info.inElements, elem, &inBytes), "the source holds more bytes than size_t counts");
    const size_t outBytes = plan->info.outElements * elem;
    require_no_overlap(out, outBytes, {{in, inBytes, "the input buffer"}});
    dev.enter(plan->device);
    launch_extract(*plan, c.in_bytes(in, inBytes), elem, c.out_bytes(out, outBytes), c.stream());
    c.finish();
}

// src/CDMExtractor.cc:369-406 with slope 1 and offset 0
void axis_range(const double* axis, size_t n, double startVal, double endVal, size_t* start, size_t* size)
{
    FA_REQUIRE(start != nullptr && size != nullptr, "NULL start or size");
    FA_REQUIRE(startVal == startVal && endVal == endVal, "a bound of the range is NaN");
    *start = *size = 0;
    if (n == 0) return;
    FA_REQUIRE(axis != nullptr, "NULL axis");
    std::vector<double> v(axis, axis + n);
    for (size_t i = 0; i < n; ++i) FA_REQUIRE(v[i] == v[i], "the axis is NaN at position " + std::to_string(i));
    double roundingDelta = 1e-5;
    if (n > 1 && v[0] != v[1]) roundingDelta = .01 * std::fabs(v[0] - v[1]);  // :370-373
    const double startValX = startVal - roundingDelta, endValX = endVal + roundingDelta;
    const bool isReverse = n > 1 && v[0] > v[1];  // :380-384
    if (isReverse) std::reverse(v.begin(), v.end());
    const long startPos = std::lower_bound(v.begin(), v.end(), startValX) - v.begin();  // val included
    const long endPos = std::upper_bound(v.begin(), v.end(), endValX) - v.begin();      // val excluded
    *size = (size_t)std::max(endPos - startPos, 0l);
    *start = isReverse ? n - *size - (size_t)startPos : (size_t)startPos;  // :401-402
}

// type2string of the reference: operator<< with the stream's default precision
std::string number(double v)
{
    std::ostringstream s;
    s << v;
    return s.str();
}

void bounding_box(const char* projIn, const char* projLonLat, const double* xAxis, size_t nx, const double* yAxis, size_t ny, int axesInDegree,
                  double south, double north, double west, double east, size_t* xPositions, size_t* nX, size_t* yPositions, size_t* nY)
{
    // :442-447; a NaN bound passes these as it does there and then keeps nothing
    FA_REQUIRE(!(south > north), "reduceLatLonBoundingBox south > north: " + number(south) + ">" + number(north));
    FA_REQUIRE(!(south < -90. || south > 90), "reduceLatLonBoundingBox south outside domain: " + number(south));
    FA_REQUIRE(!(north < -90. || north > 90), "reduceLatLonBoundingBox north outside domain: " + number(north));
    FA_REQUIRE(!(west < -180. || west > 180), "reduceLatLonBoundingBox west outside domain: " + number(west));
    FA_REQUIRE(!(east < -180. || east > 180), "reduceLatLonBoundingBox east outside domain: " + number(east));
    FA_REQUIRE(projIn != nullptr && projLonLat != nullptr, "NULL projection string");
    FA_REQUIRE(nX != nullptr && nY != nullptr, "NULL position count");
    *nX = *nY = 0;
    if (nx == 0 || ny == 0) return;  // :481-482
    FA_REQUIRE(xAxis != nullptr && yAxis != nullptr && xPositions != nullptr && yPositions != nullptr, "NULL axis or position array");
    (void)current_device_checked();
    std::vector<unsigned char> keep(nx + ny);
    {
        ScopedStream stream;
        run_bounding_box(projIn, projLonLat, xAxis, nx, yAxis, ny, axesInDegree != 0, south, north, west, east, keep.data(), keep.data() + nx,
                         stream.get());
    }
    for (size_t i = 0; i < nx; ++i)
        if (keep[i]) xPositions[(*nX)++] = i;
    for (size_t i = 0; i < ny; ++i)
        if (keep[nx + i]) yPositions[(*nY)++] = i;
}

}  // namespace

extern "C" {

int fimex_amd_extract_describe(const fimex_amd_extract_dim* dims, size_t nDims, fimex_amd_extract_info* info)
{
    return c_guard([&] {
        FA_REQUIRE(info != nullptr, "NULL argument");
        *info = extract_normalise(dims, nDims).info;
    });
}

int fimex_amd_extract_plan_create(const fimex_amd_extract_dim* dims, size_t nDims, fimex_amd_extract_plan** plan)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL argument");
        *plan = nullptr;
        const ExtractTables tables = extract_normalise(dims, nDims);
        auto p = std::make_unique<fimex_amd_extract_plan>();
        p->device = current_device_checked();
        build_extract_plan(*p, tables);
        *plan = p.release();
    });
}

int fimex_amd_extract_plan_destroy(fimex_amd_extract_plan* plan)
{
    return c_guard([&] { delete plan; });
}

int fimex_amd_extract_plan_info(const fimex_amd_extract_plan* plan, fimex_amd_extract_info* info)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr && info != nullptr, "NULL argument");
        *info = plan->info;
    });
}

int fimex_amd_extract_apply_device(const fimex_amd_extract_plan* plan, const void* d_in, int cdmType, void* d_out, void* stream)
{
    return c_guard([&] {
        PlanDevice dev{false, {}};
        extract_apply(DeviceCall{as_stream(stream)}, dev, plan, d_in, cdmType, d_out);
    });
}

int fimex_amd_extract_apply_host(const fimex_amd_extract_plan* plan, const void* in, int cdmType, void* out)
{
    return c_guard([&] {
        PlanDevice dev{true, {}};  // outlives the HostCall: its buffers go while the plan's device is current
        extract_apply(HostCall(), dev, plan, in, cdmType, out);
    });
}

int fimex_amd_extract_axis_range(const double* axis, size_t n, double startVal, double endVal, size_t* start, size_t* size)
{
    return c_guard([&] { axis_range(axis, n, startVal, endVal, start, size); });
}

int fimex_amd_extract_bounding_box_host(const char* proj_input, const char* proj_lonlat, const double* xAxis, size_t nx, const double* yAxis,
                                        size_t ny, int axesInDegree, double south, double north, double west, double east, size_t* xPositions,
                                        size_t* nX, size_t* yPositions, size_t* nY)
{
    return c_guard([&] {
        bounding_box(proj_input, proj_lonlat, xAxis, nx, yAxis, ny, axesInDegree, south, north, west, east, xPositions, nX, yPositions, nY);
    });
}

}  // extern "C"
