// What vertical.hip (the one-shot interpolation) and vertical_plan.hip (the same search stored as a plan) share: the
// search for the pair of input levels around a target, by bisection (monotonic_pair) or by the reference's walk (walk_pairs), and
// the host code that fills the search's arguments and picks the group size.  One statement of each, so that a plan followed by its
// apply gives the bits of the one-shot kernel.  The factor and the log coordinates of the blends are blend_math.hpp's; the three
// functions below give them the names the two kernels use.  The kernels keep their own copy of the loop around the search: on shared
// functions (the monotonicity scan, the group loop) they came out as other machine code, and they are to stay the code that was
// measured (profiles/vertical_blend_resource_usage.md).  monotonic_pair, walk_pairs and Column also compile for the host:
// tests/vertical_search_host.hip runs them on the CPU against the reference's sequential search.  Everything has internal linkage,
// as in vertical_common.hpp.
#pragma once
#include "vertical_common.hpp"

#include <cfloat>
#include <cmath>

namespace fimex_amd {

namespace {

__device__ inline float linear_factor(double a, double b, double x) { return blend_math::factor<float>(a, b, x); }
__device__ inline bool log_coordinates(double& a, double& b, double& x) { return blend_math::log_coordinates(a, b, x); }
__device__ inline bool loglog_coordinates(double& a, double& b, double& x) { return blend_math::loglog_coordinates(a, b, x); }

// The pair find_closest_neighbor_distinct_elements returns for a column whose levels are strictly increasing (mono > 0) or
// strictly decreasing (mono < 0), found by bisection instead of the walk.  In such a column the differences the walk compares
// are monotone in the index, so its result is fixed by the levels next to x -- as long as those differences, which it takes in
// double and compares with < and <=, are themselves strictly ordered (they tie when x is so far away that x - level rounds to
// the same double for two levels) and none of them reaches DBL_MAX, the walk's "none found" mark.  Returns false where that is
// not certain (and for columns of 32768 levels or more): the caller then walks the column.
//   cnt = number of levels <= x.  Increasing, 0 < cnt < n: (cnt - 1, cnt), but (0, 0) for x == level 0, whose highDiff starts
//   at 0 (Utils.h:263-268).  Decreasing: (q, q - 1) with q = n - cnt.  Beyond the end the column is walked TOWARDS, the fallback
//   (Utils.h:204-236) ends on (n - 1, n - 2); beyond the end it starts from, it never finds a second level: (0, 0).
// returns first | second << 16, or -1 where the walk has to decide
__host__ __device__ __noinline__ int monotonic_pair(const Column& in, int n, int mono, double x)
{
    if (mono == 0 || !(x == x) || n > 0x7fff) return -1;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double cm = (double)in.level((unsigned)(mono > 0 ? mid : n - 1 - mid));  // ascending view of the column
        if (cm <= x) lo = mid + 1;
        else hi = mid;
    }
    const int cnt = lo;
    const double c0 = (double)in.level(0u), c1 = (double)in.level(1u);
    const bool beyondFirst = (mono > 0) ? (cnt == 0) : (cnt == n);  // x before (or, decreasing, on) the level the walk starts from
    const bool beyondLast = (mono > 0) ? (cnt == n) : (cnt == 0);   // x beyond the level the walk ends on
    if (beyondFirst) {
        if (x == c0) return 0;  // decreasing only: lowDiff == highDiff == 0 and nothing is closer
        return fabs(x - c1) > fabs(x - c0) ? 0 : -1;
    }
    if (beyondLast) {
        const double d1 = fabs(x - (double)in.level((unsigned)(n - 1))), d2 = fabs(x - (double)in.level((unsigned)(n - 2)));
        if (!(d1 < d2)) return -1;
        if (n > 2 && !(d2 < fabs(x - (double)in.level((unsigned)(n - 3))))) return -1;
        return (n - 1) | ((n - 2) << 16);
    }
    const int low = (mono > 0) ? (cnt - 1) : (n - cnt);    // the closest level <= x
    const int high = (mono > 0) ? cnt : (n - cnt - 1);     // the closest level > x
    const double dl = x - (double)in.level((unsigned)low), dh = (double)in.level((unsigned)high) - x;
    if (!(dl < DBL_MAX) || !(dh < DBL_MAX)) return -1;
    if (mono > 0) {
        if (low == 0) return dl == 0 ? 0 : (1 << 16);
        if (!(x - (double)in.level((unsigned)(low - 1)) > dl)) return -1;  // the walk keeps the FIRST level with the smallest difference
    } else if (high > 0) {
        if (!((double)in.level((unsigned)(high - 1)) - x > dh)) return -1;
    }
    return low | (high << 16);
}

// find_closest_neighbor_distinct_elements (Utils.h:251-290) with its fallback find_closest_distinct_elements (:204-236) for
// kGroup values of x in one walk over the column (a second one where a value extrapolates), every comparison as written
template <int kGroup>
__host__ __device__ inline void walk_pairs(const Column& in, unsigned nzi, const double (&x)[kGroup], unsigned (&first)[kGroup], unsigned (&second)[kGroup])
{
    const double maxDiff = DBL_MAX;
    double lowDiff[kGroup], highDiff[kGroup];
    bool fallback = false;
    const float c0 = in.level(0);
#pragma unroll
    for (int g = 0; g < kGroup; ++g) {
        lowDiff[g] = x[g] - c0;
        highDiff[g] = c0 - x[g];
        if (lowDiff[g] < 0) lowDiff[g] = maxDiff;
        if (highDiff[g] < 0) highDiff[g] = maxDiff;
        first[g] = second[g] = 0;  // lowest / highest
    }
    for (unsigned k = 1; k < nzi; ++k) {
        const float cur = in.level(k);
#pragma unroll
        for (int g = 0; g < kGroup; ++g) {
            if (cur <= x[g]) {
                const double diff = x[g] - cur;
                if (diff < lowDiff[g]) { lowDiff[g] = diff; first[g] = k; }
            } else {
                const double diff = cur - x[g];
                if (diff < highDiff[g]) { highDiff[g] = diff; second[g] = k; }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < kGroup; ++g) fallback |= (lowDiff[g] == maxDiff || highDiff[g] == maxDiff);
    if (!fallback) return;
    // extrapolating
    double v1Diff[kGroup], v2Diff[kGroup];
    float v1[kGroup];
    unsigned r1[kGroup], r2[kGroup];
    bool need[kGroup];
#pragma unroll
    for (int g = 0; g < kGroup; ++g) {
        need[g] = (lowDiff[g] == maxDiff || highDiff[g] == maxDiff);
        v1[g] = c0;
        v1Diff[g] = fabs(x[g] - c0);
        v2Diff[g] = v1Diff[g];
        r1[g] = r2[g] = 0;
    }
    for (unsigned k = 0; k < nzi; ++k) {
        const float cur = in.level(k);
#pragma unroll
        for (int g = 0; g < kGroup; ++g) {
            const double vDiff = fabs(x[g] - cur);
            if (vDiff <= v2Diff[g]) {
                if (vDiff < v1Diff[g]) {
                    r2[g] = r1[g];
                    v2Diff[g] = v1Diff[g];
                    v1[g] = cur;
                    r1[g] = k;
                    v1Diff[g] = vDiff;
                } else if (cur != v1[g]) {
                    r2[g] = k;
                    v2Diff[g] = vDiff;
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < kGroup; ++g)
        if (need[g]) { first[g] = r1[g]; second[g] = r2[g]; }
}

// ---- host: the arguments and the group size, for both kernels (VintArgs and PlanArgs name the search's fields alike)

// doubles of scratch that fill_search_args takes
size_t search_scratch_doubles(const fimex_amd_vertical_levels& inLevels, const fimex_amd_vertical_levels* outLevels, size_t nzo)
{
    return coefficient_count(inLevels) + (outLevels ? coefficient_count(*outLevels) : nzo);
}

// Fills the search's fields of a kernel's arguments from the two level descriptions (the pointers in them are device pointers except the coefficients, which
// go up with h_level1 into scratch of search_scratch_doubles: the caller owns it, it has to outlive the launch).
// outLevels == NULL: fixed levels.
template <class Args>
void fill_search_args(Args& a, int method, const fimex_amd_vertical_levels& inLevels, const fimex_amd_vertical_levels* outLevels,
                      const double* h_level1, size_t nzo, const double* d_validMin, const double* d_validMax, size_t plane,
                      StreamScratch& scratch, hipStream_t stream)
{
    a.in = device_levels(inLevels, scratch, stream);
    if (outLevels) a.out = device_levels(*outLevels, scratch, stream);
    else {
        a.out.kind = -1;
        double* l1 = scratch.take(nzo);
        upload(l1, h_level1, nzo, stream);
        a.level1 = l1;
    }
    a.validMin = d_validMin;
    a.validMax = d_validMax;
    a.plane = plane;
    a.nzo = (unsigned)nzo;
    a.method = method;
    a.bisect = tuning("VERTICAL_BISECT", 1);
}

// f(std::integral_constant<int, kGroup>): output levels per walk of a column, measured: 4 is faster than 8,
// whose registers leave 2 waves per SIMD
template <class F>
void for_search_group(F&& f)
{
    if (tuning("VERTICAL_GROUP", 4) == 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 4>{});
}

}  // namespace

}  // namespace fimex_amd
