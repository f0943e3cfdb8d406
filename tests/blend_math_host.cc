// fimex_amd/csrc/blend_math.hpp compiled for the CPU with a plain C++ compiler (fimex_amd/build.py: build_blend_math_host), used
// the two ways the library uses it: classify once and evaluate the branch over n elements (convert.hip, time_interpolate.hip),
// and fold the branch into a stored factor, then evaluate from that factor (as vertical_plan.hip's entries and apply do).  tests/test_blend_math_host.py
// compares the results with the oracle's orc_get_values_1d_f bit for bit.
#include "blend_math.hpp"

#include <cstddef>

namespace bm = fimex_amd::blend_math;

extern "C" {

// the branch and the factor of one call; returns the class
int blend_math_classify(int kind, double a, double b, double x, float* f)
{
    const bm::Blend c = bm::classify(kind, a, b, x);
    *f = c.f;
    return (int)c.cls;
}

// mifi_get_values_*_f as fimex_amd_get_values_1d_f gives it: 1 (MIFI_OK) or -1 (MIFI_ERROR); on the error nothing is written
int blend_math_direct_f(int kind, const float* A, const float* B, float* out, size_t n, double a, double b, double x)
{
    const bm::Blend c = bm::classify(kind, a, b, x);
    if (c.cls == bm::Class::Error) return -1;
    for (size_t i = 0; i < n; ++i) out[i] = bm::value(c.cls, c.f, A[i], B[i]);
    return 1;
}

// the same call through a plan entry, as the vertical kernels give it: an undefined entry (the error included) is
// MIFI_UNDEFINED_F; returns whether the entry is defined, *f its stored factor
int blend_math_entry_f(int kind, const float* A, const float* B, float* out, size_t n, double a, double b, double x, float* f)
{
    float stored = 0.f;
    const bool defined = bm::fold(bm::classify(kind, a, b, x), stored);
    *f = defined ? stored : 0.f;
    for (size_t i = 0; i < n; ++i) out[i] = defined ? FA_BM_VALUE_OF_FOLDED(*f, A[i], B[i]) : bm::undefined_f();
    return defined ? 1 : 0;
}

// mifi_get_values_linear_d
int blend_math_linear_d(const double* A, const double* B, double* out, size_t n, double a, double b, double x)
{
    const bm::BlendOf<double> c = bm::classify_linear<double>(a, b, x);
    for (size_t i = 0; i < n; ++i) out[i] = bm::value(c.cls, c.f, A[i], B[i]);
    return 1;
}

}  // extern "C"
