// extern "C" boundary, vectors and projections: the vector reprojection plan and its applies (vector.hip), the proj-level entries
// (projection.hip), the coordinate searches (coordsearch.hip), points2position (convert.hip), and the regrid of a vector pair
// with its rotation (staged2_vector.hip, or the three launches it replaces), on float slices and on the pair's stored types
// (staged2_vector_typed.hip, or the five launches it replaces).
#include "capi_checks.hpp"
#include "host_call.hpp"

#include "../../include/fimex_amd_vector_regrid_host.h"
#include "../../include/fimex_amd_vector_regrid_typed_host.h"

#include <memory>
#include <string>

using namespace fimex_amd;

namespace fimex_amd {

// CDMInterpolator.cc:259-277 on device buffers: the fused kernel where it serves the plan and the batch, else the chain it
// replaces, launch for launch; returns the path taken (declared in plan.hpp: the chain of merge_vector.hip runs it too)
int apply_vector_pair(const fimex_amd_regrid_plan& plan, const fimex_amd_vector_plan& vec, const float* d_u, const float* d_v, size_t nz,
                      float* d_uOut, float* d_vOut, hipStream_t stream)
{
    if (dispatch::vector_fused(dispatch_switches(), plan_facts(plan), nz)) {
        launch_staged2_apply_vector(plan, vec, d_u, d_v, nz, d_uOut, d_vOut, stream);
        return 1;
    }
    apply_plan_device(plan, d_u, nz, d_uOut, stream);
    apply_plan_device(plan, d_v, nz, d_vOut, stream);
    launch_vector_values(vec, d_uOut, d_vOut, nz, stream);
    return 0;
}

// CDMInterpolator.cc:251-285 on device buffers in the components' stored types: the kernel on the stored type (path 2) where it
// serves the pair, else the chain it replaces -- to float, the float pair, back to the stored types -- on temporaries that are
// released after the stream has been waited for; returns the path taken (the chain: what apply_vector_pair took).  Declared in
// plan.hpp: the chain of merge_vector_typed.hip runs it too
int apply_vector_pair_typed(const fimex_amd_regrid_plan& plan, const fimex_amd_vector_plan& vec, const void* d_u, int uType, double uBad,
                            const void* d_v, int vType, double vBad, size_t nz, void* d_uOut, void* d_vOut, hipStream_t stream)
{
    if (dispatch::vector_typed_fused(dispatch_switches(), plan_facts(plan), {nz, uType, vType, aligned4(d_u) && aligned4(d_v)}) &&
        launch_staged2_apply_vector_typed(plan, vec, d_u, d_v, uType, uBad, vBad, nz, d_uOut, d_vOut, stream))
        return 2;
    const size_t nIn = nz * plan.inX * plan.inY, nOut = nz * plan.outX * plan.outY;
    DeviceArray<float> fu(nIn), fv(nIn), fuOut(nOut), fvOut(nOut);
    launch_data2interpolation(d_u, uType, nIn, uBad, fu.get(), stream);
    launch_data2interpolation(d_v, vType, nIn, vBad, fv.get(), stream);
    const int taken = apply_vector_pair(plan, vec, fu.get(), fv.get(), nz, fuOut.get(), fvOut.get(), stream);
    launch_interpolation2data(fuOut.get(), nOut, uType, uBad, d_uOut, stream);
    launch_interpolation2data(fvOut.get(), nOut, vType, vBad, d_vOut, stream);
    FA_HIP(hipStreamSynchronize(stream));  // the temporaries are released on return
    return taken;
}

}  // namespace fimex_amd

namespace {

template <class Call>
void points2position(Call&& c, double* points, size_t n, const double* axis, int num, int axis_type)
{
    if (n == 0) return;
    FA_REQUIRE(points != nullptr && axis != nullptr, "NULL argument");
    (void)current_device_checked();
    launch_points2position(c.inout(points, n), n, axis, num, axis_type, c.stream());
    c.finish();
}

template <class Call>
void project_values(Call&& c, const char* proj_input, const char* proj_output, double* x, double* y, size_t num, const char* nullArray)
{
    FA_REQUIRE(num == 0 || (x != nullptr && y != nullptr), nullArray);
    (void)current_device_checked();
    launch_project_values(proj_input, proj_output, c.inout(x, num), c.inout(y, num), num, c.stream());
    c.finish();
}

template <class Call>
void project_axes(Call&& c, const char* proj_input, const char* proj_output, const double* in_x_axis, const double* in_y_axis, size_t ix,
                  size_t iy, double* outX, double* outY)
{
    const size_t n = ix * iy;
    FA_REQUIRE(n == 0 || (in_x_axis != nullptr && in_y_axis != nullptr && outX != nullptr && outY != nullptr), "NULL argument");
    (void)current_device_checked();
    launch_project_axes(proj_input, proj_output, in_x_axis, in_y_axis, ix, iy, c.out(outX, n), c.out(outY, n), c.stream());
    c.finish();
}

template <class Call>
void vector_reproject_matrix(Call&& c, const char* proj_input, const char* proj_output, const double* out_x_axis, const double* out_y_axis,
                             int xType, int yType, size_t ox, size_t oy, double* matrix)
{
    FA_REQUIRE(ox * oy == 0 || (out_x_axis != nullptr && out_y_axis != nullptr && matrix != nullptr), "NULL argument");
    (void)current_device_checked();
    launch_vector_reproject_matrix(proj_input, proj_output, out_x_axis, out_y_axis, xType, yType, ox, oy, c.out(matrix, 4 * ox * oy), c.stream());
    c.finish();
}

void check_coord_search_host(const double* px, const double* py, size_t nPoints, const double* lon, const double* lat, size_t n)
{
    FA_REQUIRE(nPoints == 0 || (px != nullptr && py != nullptr), "NULL argument");
    FA_REQUIRE(n == 0 || (lon != nullptr && lat != nullptr), "NULL argument");
}

// what every form of regrid_apply_vector refuses; the buffers are the caller's own pointers, host or device, and their sizes count
// elements of uElem bytes (u, uOut) and vElem bytes (v, vOut)
void check_vector_pair_sized(const fimex_amd_regrid_plan& plan, const fimex_amd_vector_plan& vec, const void* u, size_t uElem, const void* v,
                             size_t vElem, size_t nz, const void* uOut, const void* vOut)
{
    FA_REQUIRE(plan.kind != PlanKind::Forward, "a vector pair is regridded with a backward plan, this is a forward plan");
    FA_REQUIRE(vec.ox == plan.outX && vec.oy == plan.outY, "the vector plan's grid (ox, oy) differs from the regrid plan's output grid (outX, outY)");
    FA_REQUIRE(vec.device == plan.device, "the regrid plan and the vector plan live on different devices");
    const size_t inCells = nz * plan.inX * plan.inY, outCells = nz * plan.outX * plan.outY;
    const Span b[4] = {{u, inCells * uElem, "u"}, {v, inCells * vElem, "v"}, {uOut, outCells * uElem, "uOut"}, {vOut, outCells * vElem, "vOut"}};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j) {
            const char *p = static_cast<const char*>(b[i].p), *q = static_cast<const char*>(b[j].p);
            FA_REQUIRE(!b[i].bytes || !b[j].bytes || p + b[i].bytes <= q || q + b[j].bytes <= p,
                       std::string("buffers overlap: ") + b[i].name + " and " + b[j].name);
        }
}

void check_vector_pair(const fimex_amd_regrid_plan& plan, const fimex_amd_vector_plan& vec, const float* u, const float* v, size_t nz,
                       const float* uOut, const float* vOut)
{
    check_vector_pair_sized(plan, vec, u, sizeof(float), v, sizeof(float), nz, uOut, vOut);
}

}  // namespace

extern "C" {

int fimex_amd_vector_plan_create(const double* matrix, size_t ox, size_t oy, fimex_amd_vector_plan** out)
{
    return c_guard([&] {
        FA_REQUIRE(out != nullptr, "plan output pointer is NULL");
        *out = nullptr;
        FA_REQUIRE(matrix != nullptr, "matrix is NULL");
        auto plan = std::make_unique<fimex_amd_vector_plan>();
        plan->device = current_device_checked();
        plan->ox = ox;
        plan->oy = oy;
        build_vector_plan(*plan, matrix);
        *out = plan.release();
    });
}

int fimex_amd_vector_plan_destroy(fimex_amd_vector_plan* plan)
{
    return c_guard([&] {
        if (!plan) return;
        ScopedDevice dev(plan->device);
        delete plan;
    });
}

// the vector reprojection pairs differ in their refusals and in their device policy (the host form switches to the plan's
// device, the device form demands it or, for direction_scaled, switches too): each keeps its own body

int fimex_amd_vector_reproject_values_host(const fimex_amd_vector_plan* plan, float* u, float* v, size_t size)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL plan");
        const size_t layer = plan->ox * plan->oy;
        const size_t oz = size / layer;  // CachedVectorReprojection.cc:41
        if (oz == 0) return;
        FA_REQUIRE(u != nullptr && v != nullptr, "NULL buffer");
        ScopedDevice dev(plan->device);
        HostCall hc;
        launch_vector_values(*plan, hc.inout(u, oz * layer), hc.inout(v, oz * layer), oz, hc.stream());
        hc.finish();
    });
}

int fimex_amd_vector_reproject_values_device(const fimex_amd_vector_plan* plan, float* d_u, float* d_v, size_t oz, void* stream)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL plan");
        if (oz == 0) return;
        FA_REQUIRE(d_u != nullptr && d_v != nullptr, "NULL device buffer");
        require_current_device(plan->device);
        launch_vector_values(*plan, d_u, d_v, oz, as_stream(stream));
    });
}

int fimex_amd_regrid_apply_vector_device(const fimex_amd_regrid_plan* plan, const fimex_amd_vector_plan* vec, const float* d_u, const float* d_v,
                                         size_t nz, float* d_uOut, float* d_vOut, void* stream, int* path)
{
    return c_guard([&] {
        if (path) *path = 0;
        FA_REQUIRE(plan != nullptr, "NULL regrid plan");
        FA_REQUIRE(vec != nullptr, "NULL vector plan");
        FA_REQUIRE(nz == 0 || (d_u != nullptr && d_v != nullptr && d_uOut != nullptr && d_vOut != nullptr), "NULL device buffer");
        check_vector_pair(*plan, *vec, d_u, d_v, nz, d_uOut, d_vOut);
        if (nz == 0) return;
        require_current_device(plan->device);
        const int taken = apply_vector_pair(*plan, *vec, d_u, d_v, nz, d_uOut, d_vOut, as_stream(stream));
        if (path) *path = taken;
    });
}

int fimex_amd_regrid_apply_vector_host(const fimex_amd_regrid_plan* plan, const fimex_amd_vector_plan* vec, const float* u, const float* v,
                                       size_t size, float* uOut, float* vOut, size_t outCapacity, size_t* newSize)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL regrid plan");
        FA_REQUIRE(vec != nullptr, "NULL vector plan");
        FA_REQUIRE(newSize != nullptr, "NULL argument");
        const size_t inLayer = plan->inX * plan->inY, outLayer = plan->outX * plan->outY;
        const size_t nz = inLayer ? size / inLayer : 0;  // CachedInterpolation.cc:121
        *newSize = outLayer * nz;                         // :122
        FA_REQUIRE(nz == 0 || (u != nullptr && v != nullptr && uOut != nullptr && vOut != nullptr), "NULL buffer");
        check_vector_pair(*plan, *vec, u, v, nz, uOut, vOut);
        if (nz == 0) return;
        FA_REQUIRE(outCapacity >= *newSize, "output buffers too small");
        ScopedDevice dev(plan->device);
        HostCall hc;
        const float *d_u = hc.in(u, nz * inLayer), *d_v = hc.in(v, nz * inLayer);
        apply_vector_pair(*plan, *vec, d_u, d_v, nz, hc.out(uOut, nz * outLayer), hc.out(vOut, nz * outLayer), hc.stream());
        hc.finish();
    });
}

int fimex_amd_regrid_apply_vector_typed_device(const fimex_amd_regrid_plan* plan, const fimex_amd_vector_plan* vec, const void* d_u, int uType,
                                               double uBad, const void* d_v, int vType, double vBad, size_t nz, void* d_uOut, void* d_vOut,
                                               void* stream, int* path)
{
    return c_guard([&] {
        if (path) *path = 0;
        FA_REQUIRE(plan != nullptr, "NULL regrid plan");
        FA_REQUIRE(vec != nullptr, "NULL vector plan");
        const size_t uElem = cdm_type_size(uType), vElem = cdm_type_size(vType);  // throws for NAT and STRING
        FA_REQUIRE(nz == 0 || (d_u != nullptr && d_v != nullptr && d_uOut != nullptr && d_vOut != nullptr), "NULL device buffer");
        check_vector_pair_sized(*plan, *vec, d_u, uElem, d_v, vElem, nz, d_uOut, d_vOut);
        if (nz == 0) return;
        require_current_device(plan->device);
        const int taken = apply_vector_pair_typed(*plan, *vec, d_u, uType, uBad, d_v, vType, vBad, nz, d_uOut, d_vOut, as_stream(stream));
        if (path) *path = taken;
    });
}

int fimex_amd_regrid_apply_vector_typed_host(const fimex_amd_regrid_plan* plan, const fimex_amd_vector_plan* vec, const void* u, int uType,
                                             double uBad, const void* v, int vType, double vBad, size_t size, void* uOut, void* vOut,
                                             size_t outCapacity, size_t* newSize)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL regrid plan");
        FA_REQUIRE(vec != nullptr, "NULL vector plan");
        FA_REQUIRE(newSize != nullptr, "NULL argument");
        const size_t uElem = cdm_type_size(uType), vElem = cdm_type_size(vType);  // throws for NAT and STRING
        const size_t inLayer = plan->inX * plan->inY, outLayer = plan->outX * plan->outY;
        const size_t nz = inLayer ? size / inLayer : 0;  // CachedInterpolation.cc:121
        *newSize = outLayer * nz;                         // :122
        FA_REQUIRE(nz == 0 || (u != nullptr && v != nullptr && uOut != nullptr && vOut != nullptr), "NULL buffer");
        check_vector_pair_sized(*plan, *vec, u, uElem, v, vElem, nz, uOut, vOut);
        if (nz == 0) return;
        FA_REQUIRE(outCapacity >= *newSize, "output buffers too small");
        ScopedDevice dev(plan->device);
        HostCall hc;  // only stored-type bytes cross to the device and back
        const void *d_u = hc.in_bytes(u, nz * inLayer * uElem), *d_v = hc.in_bytes(v, nz * inLayer * vElem);
        apply_vector_pair_typed(*plan, *vec, d_u, uType, uBad, d_v, vType, vBad, nz, hc.out_bytes(uOut, nz * outLayer * uElem),
                                hc.out_bytes(vOut, nz * outLayer * vElem), hc.stream());
        hc.finish();
    });
}

int fimex_amd_vector_reproject_direction_host(const fimex_amd_vector_plan* plan, float* angles, size_t size)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL plan");
        const size_t layer = plan->ox * plan->oy;
        const size_t oz = size / layer;  // CachedVectorReprojection.cc:52
        if (oz == 0) return;
        FA_REQUIRE(angles != nullptr, "NULL buffer");
        ScopedDevice dev(plan->device);
        HostCall hc;
        launch_vector_direction(*plan, hc.inout(angles, oz * layer), oz, hc.stream());
        hc.finish();
    });
}

int fimex_amd_vector_reproject_direction_device(const fimex_amd_vector_plan* plan, float* d_angles, size_t oz, void* stream)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL plan");
        if (oz == 0) return;
        FA_REQUIRE(d_angles != nullptr, "NULL device buffer");
        require_current_device(plan->device);
        launch_vector_direction(*plan, d_angles, oz, as_stream(stream));
    });
}

int fimex_amd_vector_reproject_direction_scaled_device(const fimex_amd_vector_plan* plan, float* d_angles, size_t oz, double scale,
                                                       double offset, void* stream)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr && (oz == 0 || d_angles != nullptr), "NULL argument");
        ScopedDevice dev(plan->device);
        launch_vector_direction_scaled(*plan, d_angles, oz, scale, offset, as_stream(stream));
    });
}

int fimex_amd_vector_reproject_direction_scaled_host(const fimex_amd_vector_plan* plan, float* angles, size_t size, double scale, double offset)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL argument");
        const size_t layer = plan->ox * plan->oy, oz = layer ? size / layer : 0;
        if (oz == 0) return;
        FA_REQUIRE(angles != nullptr, "NULL argument");
        ScopedDevice dev(plan->device);
        HostCall hc;
        launch_vector_direction_scaled(*plan, hc.inout(angles, oz * layer), oz, scale, offset, hc.stream());
        hc.finish();
    });
}

int fimex_amd_rotate_vector_typed_host(const fimex_amd_vector_plan* plan, const void* xData, int xType, double xFill, const void* yData,
                                       int yType, double yFill, size_t size, int returnX, int outType, double outFill, void* outData)
{
    return c_guard([&] {
        FA_REQUIRE(plan != nullptr, "NULL argument");
        const size_t ex = cdm_type_size(xType), ey = cdm_type_size(yType), eo = cdm_type_size(outType);
        const size_t layer = plan->ox * plan->oy, oz = layer ? size / layer : 0;
        if (size == 0) return;
        FA_REQUIRE(xData != nullptr && yData != nullptr && outData != nullptr, "NULL argument");
        ScopedDevice dev(plan->device);
        DeviceArray<float> d_u(size), d_v(size);  // before hc: released after hc has waited for its stream
        HostCall hc;
        hipStream_t st = hc.stream();
        float *u = d_u.get(), *v = d_v.get();
        launch_data2interpolation(hc.in_bytes(xData, size * ex), xType, size, xFill, u, st);   // CDMProcessor.cc:607-608
        launch_data2interpolation(hc.in_bytes(yData, size * ey), yType, size, yFill, v, st);
        launch_vector_values(*plan, u, v, oz, st);                     // :612 (whole slices only, as the reference)
        launch_interpolation2data(returnX ? u : v, size, outType, outFill, hc.out_bytes(outData, size * eo), st);  // :614-618
        hc.finish();
    });
}

int fimex_amd_points2position_device(double* d_points, size_t n, const double* axis, int num, int axis_type, void* stream)
{
    return c_guard([&] { points2position(DeviceCall{as_stream(stream)}, d_points, n, axis, num, axis_type); });
}

int fimex_amd_points2position_host(double* points, size_t n, const double* axis, int num, int axis_type)
{
    return c_guard([&] { points2position(HostCall(), points, n, axis, num, axis_type); });
}

int fimex_amd_project_values_device(const char* proj_input, const char* proj_output, double* d_x, double* d_y, size_t num, void* stream)
{
    return c_guard([&] { project_values(DeviceCall{as_stream(stream)}, proj_input, proj_output, d_x, d_y, num, "NULL device buffer"); });
}

int fimex_amd_project_values_host(const char* proj_input, const char* proj_output, double* x, double* y, size_t num)
{
    return c_guard([&] { project_values(HostCall(), proj_input, proj_output, x, y, num, "NULL argument"); });
}

int fimex_amd_project_axes_device(const char* proj_input, const char* proj_output, const double* in_x_axis, const double* in_y_axis,
                                  size_t ix, size_t iy, double* d_outX, double* d_outY, void* stream)
{
    return c_guard([&] { project_axes(DeviceCall{as_stream(stream)}, proj_input, proj_output, in_x_axis, in_y_axis, ix, iy, d_outX, d_outY); });
}

int fimex_amd_project_axes_host(const char* proj_input, const char* proj_output, const double* in_x_axis, const double* in_y_axis,
                                size_t ix, size_t iy, double* outX, double* outY)
{
    return c_guard([&] { project_axes(HostCall(), proj_input, proj_output, in_x_axis, in_y_axis, ix, iy, outX, outY); });
}

int fimex_amd_get_vector_reproject_matrix_device(const char* proj_input, const char* proj_output, const double* out_x_axis,
                                                 const double* out_y_axis, int xType, int yType, size_t ox, size_t oy,
                                                 double* d_matrix, void* stream)
{
    return c_guard([&] {
        vector_reproject_matrix(DeviceCall{as_stream(stream)}, proj_input, proj_output, out_x_axis, out_y_axis, xType, yType, ox, oy, d_matrix);
    });
}

int fimex_amd_get_vector_reproject_matrix_host(const char* proj_input, const char* proj_output, const double* out_x_axis,
                                               const double* out_y_axis, int xType, int yType, size_t ox, size_t oy, double* matrix)
{
    return c_guard([&] { vector_reproject_matrix(HostCall(), proj_input, proj_output, out_x_axis, out_y_axis, xType, yType, ox, oy, matrix); });
}

int fimex_amd_get_vector_reproject_matrix_field_host(const char* proj_input, const char* proj_output, const double* in_x_field,
                                                     const double* in_y_field, size_t ox, size_t oy, double* matrix)
{
    return c_guard([&] {
        const size_t n = ox * oy;
        FA_REQUIRE(n == 0 || (in_x_field != nullptr && in_y_field != nullptr && matrix != nullptr), "NULL argument");
        (void)current_device_checked();
        HostCall hc;
        launch_vector_reproject_matrix_field(proj_input, proj_output, in_x_field, in_y_field, ox, oy, hc.out(matrix, 4 * n), hc.stream());
        hc.finish();
    });
}

int fimex_amd_get_vector_reproject_matrix_points_host(const char* proj_input, const char* proj_output, int inputIsMetric,
                                                      const double* out_x_points, const double* out_y_points, size_t on, double* matrix)
{
    return c_guard([&] {
        FA_REQUIRE(on == 0 || (out_x_points != nullptr && out_y_points != nullptr && matrix != nullptr), "NULL argument");
        (void)current_device_checked();
        HostCall hc;
        launch_vector_reproject_matrix_points(proj_input, proj_output, inputIsMetric, out_x_points, out_y_points, on, hc.out(matrix, 4 * on),
                                              hc.stream());
        hc.finish();
    });
}

int fimex_amd_projection_is_degree(const char* proj)
{
    int r = -1;
    const int rc = c_guard([&] { r = projection_is_degree(proj); });
    return rc == FIMEX_AMD_OK ? r : -1;
}

// the coordinate searches refuse differently in their two forms: each keeps its own body

int fimex_amd_coord_nearest_host(double* px, double* py, size_t nPoints, const double* lon, const double* lat, size_t orgX, size_t orgY)
{
    return c_guard([&] {
        const size_t n = orgX * orgY;
        check_coord_search_host(px, py, nPoints, lon, lat, n);
        (void)current_device_checked();
        HostCall hc;
        launch_coord_nearest(hc.inout(px, nPoints), hc.inout(py, nPoints), nPoints, hc.in(lon, n), hc.in(lat, n), orgX, orgY, hc.stream());
        hc.finish();
    });
}

int fimex_amd_coord_nearest_device(double* d_px, double* d_py, size_t nPoints, const double* d_lon, const double* d_lat, size_t orgX, size_t orgY,
                                   void* stream)
{
    return c_guard([&] {
        FA_REQUIRE(nPoints == 0 || (d_px != nullptr && d_py != nullptr && d_lon != nullptr && d_lat != nullptr), "NULL device buffer");
        (void)current_device_checked();
        launch_coord_nearest(d_px, d_py, nPoints, d_lon, d_lat, orgX, orgY, as_stream(stream));
    });
}

int fimex_amd_coord_kdtree_host(double maxDist, double* px, double* py, size_t nPoints, const double* lon, const double* lat, size_t orgX, size_t orgY)
{
    return c_guard([&] {
        const size_t n = orgX * orgY;
        check_coord_search_host(px, py, nPoints, lon, lat, n);
        (void)current_device_checked();
        HostCall hc;
        launch_coord_kdtree(maxDist, hc.inout(px, nPoints), hc.inout(py, nPoints), nPoints, hc.in(lon, n), hc.in(lat, n), orgX, orgY,
                            hc.stream());
        hc.finish();
    });
}

int fimex_amd_coord_kdtree_device(double maxDist, double* d_px, double* d_py, size_t nPoints, const double* d_lon, const double* d_lat, size_t orgX,
                                  size_t orgY, void* stream)
{
    return c_guard([&] {
        FA_REQUIRE(nPoints == 0 || (d_px != nullptr && d_py != nullptr && d_lon != nullptr && d_lat != nullptr), "NULL device buffer");
        (void)current_device_checked();
        launch_coord_kdtree(maxDist, d_px, d_py, nPoints, d_lon, d_lat, orgX, orgY, as_stream(stream));
    });
}

int fimex_amd_grid_distance_host(const double* lon, const double* lat, size_t orgX, size_t orgY, double* maxGridDistance)
{
    return c_guard([&] {
        const size_t n = orgX * orgY;
        FA_REQUIRE(n > 0 && lon != nullptr && lat != nullptr && maxGridDistance != nullptr, "NULL or empty argument");
        (void)current_device_checked();
        HostCall hc;
        *maxGridDistance = grid_distance(hc.in(lon, n), hc.in(lat, n), orgX, orgY, hc.stream());  // waits for its result: nothing to copy back
    });
}

}  // extern "C"
