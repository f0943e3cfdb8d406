// extern "C" boundary, fills (fill_rects.hip), the 1-D blends (convert.hip) and scan_sum (fill_sum.hip).
#include "host_call.hpp"

using namespace fimex_amd;

namespace {

// one fill in place, on the caller's device field or on a copy of the caller's host field
template <class Call, class Run>
void fill_in_place(Call&& c, size_t n, float* field, const char* nullField, Run&& run)
{
    if (n == 0) return;
    FA_REQUIRE(field != nullptr, nullField);
    (void)current_device_checked();
    run(c.inout(field, n), c.stream());
    c.finish();
}

// validates its arguments even for n == 0
template <class Call>
void get_values_1d_f(Call&& c, int kind, const float* A, const float* B, float* out, size_t n, double a, double b, double x, const char* nullArray)
{
    FA_REQUIRE(n == 0 || (A != nullptr && B != nullptr && out != nullptr), nullArray);
    (void)current_device_checked();
    if (!launch_get_values_1d_f(kind, c.in(A, n), c.in(B, n), c.out(out, n), n, a, b, x, c.stream()))
        throw Error("log blend needs positive coordinates (src/interpolation.c:1137, 1149)");
    c.finish();
}

}  // namespace

extern "C" {

int fimex_amd_fill2d_host(size_t nx, size_t ny, size_t nz, float* field, float relaxCrit, float corrEff, size_t maxLoop,
                          size_t* nChanged)
{
    return c_guard([&] {
        fill_in_place(HostCall(), nx * ny * nz, field, "NULL buffer",
                      [&](float* d, hipStream_t st) { run_fill2d(nx, ny, nz, d, relaxCrit, corrEff, maxLoop, nChanged, st); });
    });
}

int fimex_amd_fill2d_device(size_t nx, size_t ny, size_t nz, float* d_field, float relaxCrit, float corrEff, size_t maxLoop,
                            size_t* nChanged, void* stream)
{
    return c_guard([&] {
        fill_in_place(DeviceCall{as_stream(stream)}, nx * ny * nz, d_field, "NULL device buffer",
                      [&](float* d, hipStream_t st) { run_fill2d(nx, ny, nz, d, relaxCrit, corrEff, maxLoop, nChanged, st); });
    });
}

int fimex_amd_creepfill2d_host(size_t nx, size_t ny, size_t nz, float* field, unsigned short repeat, char setWeight,
                               size_t* nChanged)
{
    return c_guard([&] {
        fill_in_place(HostCall(), nx * ny * nz, field, "NULL buffer",
                      [&](float* d, hipStream_t st) { run_creepfill(nx, ny, nz, d, false, 0.f, repeat, setWeight, nChanged, st); });
    });
}

int fimex_amd_creepfill2d_device(size_t nx, size_t ny, size_t nz, float* d_field, unsigned short repeat, char setWeight,
                                 size_t* nChanged, void* stream)
{
    return c_guard([&] {
        fill_in_place(DeviceCall{as_stream(stream)}, nx * ny * nz, d_field, "NULL device buffer",
                      [&](float* d, hipStream_t st) { run_creepfill(nx, ny, nz, d, false, 0.f, repeat, setWeight, nChanged, st); });
    });
}

int fimex_amd_creepfillval2d_host(size_t nx, size_t ny, size_t nz, float* field, float defaultVal, unsigned short repeat,
                                  char setWeight, size_t* nChanged)
{
    return c_guard([&] {
        fill_in_place(HostCall(), nx * ny * nz, field, "NULL buffer",
                      [&](float* d, hipStream_t st) { run_creepfill(nx, ny, nz, d, true, defaultVal, repeat, setWeight, nChanged, st); });
    });
}

int fimex_amd_creepfillval2d_device(size_t nx, size_t ny, size_t nz, float* d_field, float defaultVal, unsigned short repeat,
                                    char setWeight, size_t* nChanged, void* stream)
{
    return c_guard([&] {
        fill_in_place(DeviceCall{as_stream(stream)}, nx * ny * nz, d_field, "NULL device buffer",
                      [&](float* d, hipStream_t st) { run_creepfill(nx, ny, nz, d, true, defaultVal, repeat, setWeight, nChanged, st); });
    });
}

int fimex_amd_get_values_1d_f_device(int kind, const float* d_A, const float* d_B, float* d_out, size_t n, double a, double b, double x, void* stream)
{
    return c_guard([&] { get_values_1d_f(DeviceCall{as_stream(stream)}, kind, d_A, d_B, d_out, n, a, b, x, "NULL device buffer"); });
}

int fimex_amd_get_values_1d_f_host(int kind, const float* A, const float* B, float* out, size_t n, double a, double b, double x)
{
    return c_guard([&] { get_values_1d_f(HostCall(), kind, A, B, out, n, a, b, x, "NULL argument"); });
}

int fimex_amd_get_values_linear_d_device(const double* d_A, const double* d_B, double* d_out, size_t n, double a, double b, double x, void* stream)
{
    return c_guard([&] {
        FA_REQUIRE(n == 0 || (d_A != nullptr && d_B != nullptr && d_out != nullptr), "NULL device buffer");
        (void)current_device_checked();
        launch_get_values_linear_d(d_A, d_B, d_out, n, a, b, x, as_stream(stream));
    });
}

int fimex_amd_scan_sum_device(const float* d_values, size_t n, int mode, double average, int algo, double* sum, size_t* nUndefined, void* stream)
{
    return c_guard([&] {
        FA_REQUIRE(sum != nullptr && (d_values != nullptr || n == 0), "NULL argument");
        (void)current_device_checked();
        run_scan_sum(d_values, n, mode, average, algo, sum, nUndefined, as_stream(stream));
    });
}

}  // extern "C"
