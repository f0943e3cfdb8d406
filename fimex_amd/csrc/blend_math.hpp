// The seven 1-D blends between two fields, mifi_get_values_{nearest, linear, linear_weak_extrapol, linear_no_extrapol,
// linear_const_extrapol, log, log_log}_f (src/interpolation.c:1030-1156) and mifi_get_values_linear_d (:1064-1083), stated once
// for host and device: the factor, the coordinates of the two log kinds, the branch a factor selects (classify) and the value
// of an element on that branch (value).  convert.hip and capi_time_quality.hip run classify once per call or output step on the
// host, where the branch then picks a copy or a kernel; vertical.hip and vertical_plan.hip take the factor and the log coordinates
// per cell on the device and keep their own fold of the branch rule, the machine code that was measured.
// tests/blend_math_host.cc compiles it with a plain C++ compiler, so it includes nothing of HIP and uses no device builtin.
// Compile with -ffp-contract=off: A + f * (B - A) is a subtraction, a multiply and an add, as in the reference.
//
// Where two callers treat a result differently without a stated reason, the difference is kept and named at its line
// ("differs:"), here and in the callers.
#pragma once

#include <cmath>

#include "../../include/fimex_amd.h"

#if defined(__HIPCC__)
#define FA_BM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FA_BM_HD inline
#endif

namespace fimex_amd {
namespace blend_math {

// The kinds, in the order of the seven functions above: the values of FIMEX_AMD_1D_* (fimex_amd_get_values_1d_f_*) themselves.  The
// vertical entries name the same seven by FIMEX_AMD_VINT_METHOD_* (mifi_vertical_interpol_method of include/fimex/mifi_constants.h,
// mapped by CDMVerticalInterpolator.cc:333-341); the two search kernels switch on those codes themselves (vertical.hip: blend).
enum Kind : int {
    kNearest = FIMEX_AMD_1D_NEAREST, kLinear = FIMEX_AMD_1D_LINEAR, kLinearWeakExtrapol = FIMEX_AMD_1D_LINEAR_WEAK_EXTRAPOL,
    kLinearNoExtrapol = FIMEX_AMD_1D_LINEAR_NO_EXTRAPOL, kLinearConstExtrapol = FIMEX_AMD_1D_LINEAR_CONST_EXTRAPOL,
    kLog = FIMEX_AMD_1D_LOG, kLogLog = FIMEX_AMD_1D_LOG_LOG
};

FA_BM_HD bool kind_known(int kind) { return kind >= kNearest && kind <= kLogLog; }

// MIFI_UNDEFINED_F as every kernel writes it (common.hpp)
FA_BM_HD float undefined_f() { return __builtin_bit_cast(float, 0x7fc00000u); }

// ---- the factor: the double quotient narrowed once to float (:1051, :1087, :1117), or kept for mifi_get_values_linear_d (:1066)
template <typename T>
FA_BM_HD T factor(double a, double b, double x)
{
    return (a == b) ? 0 : ((x - a) / (b - a));
}

// ---- the coordinates of the log kinds; false: MIFI_ERROR
// mifi_get_values_log_f, :1134-1139
FA_BM_HD bool log_coordinates(double& a, double& b, double& x)
{
    if (a <= 0 || b <= 0 || x <= 0) return false;
    a = log(a);
    b = log(b);
    x = log(x);
    return true;
}

// mifi_get_values_log_log_f with the call of mifi_get_values_log_f in it, :1146-1153.  The reference drops the status of that inner
// call and would return MIFI_OK with nothing written; no input gets there: past the outer guard a > 0, so log(a + e) >= 1, and a NaN
// passes both guards.
FA_BM_HD bool loglog_coordinates(double& a, double& b, double& x)
{
    if (a <= 0 || b <= 0 || x <= 0) return false;
    const double la = log(a + M_E), lb = log(b + M_E), lx = log(x + M_E);
    if (la <= 0 || lb <= 0 || lx <= 0) return false;
    a = log(la);
    b = log(lb);
    x = log(lx);
    return true;
}

// ---- the branch.  0 to 3 travel to the device as kernel arguments (time_interpolate.hip) and keep their values.
enum class Class : unsigned char {
    CopyA = 0,      // the reference's memcpy of field A: no 0 * NaN from the other field
    CopyB = 1,
    Blend = 2,      // A + f * (B - A)
    Undefined = 3,  // MIFI_UNDEFINED_F, :1100
    Error = 4       // MIFI_ERROR: the function has written nothing
};

template <typename T>
struct BlendOf {
    Class cls;
    T f;  // as computed; 0 or 1 on the copies of nearest and const_extrapol, 0 on the error
};
using Blend = BlendOf<float>;

// the branch of mifi_get_values_linear_f, :1052-1060, and with T = double of mifi_get_values_linear_d, :1067-1081
template <typename T>
FA_BM_HD BlendOf<T> branch_linear(T f)
{
    return BlendOf<T>{f == 0 ? Class::CopyA : f == 1 ? Class::CopyB : Class::Blend, f};
}

template <typename T = float>
FA_BM_HD BlendOf<T> classify_linear(double a, double b, double x)
{
    return branch_linear(factor<T>(a, b, x));
}

// the branch of mifi_get_values_linear_conf_extrapol_f, :1088-1102
FA_BM_HD Blend branch_conf_extrapol(float left, float right, float f)
{
    if (f == 0) return Blend{Class::CopyA, f};
    if (f == 1) return Blend{Class::CopyB, f};
    return Blend{((f >= left) && (f <= right)) ? Class::Blend : Class::Undefined, f};
}

// All seven: the coordinates of the log kinds first, then the one factor every kind but nearest takes, then the kind's branch.
FA_BM_HD Blend classify(int kind, double a, double b, double x)
{
    if (kind == kNearest) return Blend{Class::CopyA, 0.f};  // :1030-1034
    if (kind == kLog && !log_coordinates(a, b, x)) return Blend{Class::Error, 0.f};        // :1131-1142
    if (kind == kLogLog && !loglog_coordinates(a, b, x)) return Blend{Class::Error, 0.f};  // :1144-1156
    const float f = factor<float>(a, b, x);
    switch (kind) {
    case kLinearWeakExtrapol: return branch_conf_extrapol(-1.f, 2.f, f);  // :1106-1109
    case kLinearNoExtrapol: return branch_conf_extrapol(0.f, 1.f, f);     // :1110-1113
    case kLinearConstExtrapol:  // :1115-1126; a NaN factor blends
        if (f >= 1) return Blend{Class::CopyB, 1.f};
        if (f <= 0) return Blend{Class::CopyA, 0.f};
        return Blend{Class::Blend, f};
    default: return branch_linear(f);  // kLinear, and kLog / kLogLog on their coordinates
    }
}

// ---- the value of one element on a branch; float (:1045, :1100) or double (:1079, where only the first three branches occur)
template <typename T>
FA_BM_HD T value(Class cls, T f, T A, T B)
{
    return cls == Class::CopyA ? A : cls == Class::CopyB ? B : cls == Class::Blend ? A + f * (B - A) : (T)undefined_f();
}

// ---- a branch folded into one stored factor and back (the entries of vertical_plan.hip): a copy of A is f == 0, a copy of B
// f == 1, so that nearest and the clamped ends of const_extrapol need no class of their own.  false: the element is undefined.
// vertical_plan.hip's entry_factor is this fold in the form its kernel was measured with; tests/test_blend_math_host.py pins this
// one and the text below to the reference, tests/test_gpu_vertical_plan.py the kernel's.
FA_BM_HD bool fold(const Blend& c, float& f)
{
    f = c.f;
    return c.cls <= Class::Blend;
}

// value(the class of f, f, A, B) as text, for the one caller: plan_apply_kernel expands it in place, because behind a function,
// inlined or not, its instances for two and four variables come out with other registers (signed char x 2: 58 scalar spills for 53).
#define FA_BM_VALUE_OF_FOLDED(f, A, B) (((f) == 0) ? (A) : ((f) == 1) ? (B) : (A) + (f) * ((B) - (A)))

}  // namespace blend_math
}  // namespace fimex_amd
