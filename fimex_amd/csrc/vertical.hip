// Vertical interpolation of [nt][nzi][ny][nx] to fixed or template levels: the loop of
// CDMVerticalInterpolator::getLevelDataSlice, src/CDMVerticalInterpolator.cc:441-504, restated per column.
//
// A lane owns one column; consecutive lanes own x-adjacent columns, so every load of a level plane, a data plane or ps is
// coalesced along x.  In a column whose levels are strictly monotonic the pair of input levels around a target comes from a
// bisection (monotonic_pair); otherwise, and wherever the bisection cannot be sure, from the reference's walk: output levels
// go in groups of kGroup and the scan of include/fimex/Utils.h:251-290 runs once over the column's input levels for the whole
// group, with its state (lowDiff, highDiff, lowest, highest per output level) in registers.  Levels given by a formula are recomputed from ps in every pass (two FP64 operations, no memory), an explicit
// level field is re-read (nzo / kGroup times, from L2 / Infinity Cache: the lanes of a workgroup come back to the lines they
// have just read).  The data column is not streamed at all: once a pair of input levels is known the two values are fetched
// from their planes, neighbouring lanes mostly from the same two.  No workgroup waits for another one.
#include "vertical_common.hpp"

#include <cfloat>
#include <cmath>
#include <vector>

namespace fimex_amd {

namespace {

struct VintArgs {
    Levels in, out;         // out.kind < 0: fixed levels (level1)
    const double* level1;   // device, [nzo]
    const double* validMin; // [plane] or NULL
    const double* validMax;
    const float* data;      // [nt][nzi][plane]
    float* result;          // [nt][nzo][plane]
    size_t plane;
    unsigned nzo;
    int method;
    int bisect;  // 0: every column is walked (tuning build)
    float clampMin, clampMax;
};

// mifi_get_values_linear_f with n = 1, src/interpolation.c:1049-1062
__device__ inline float blend_linear(float A, float B, double a, double b, double x)
{
    const float f = (a == b) ? 0 : ((x - a) / (b - a));
    if (f == 0) return A;
    if (f == 1) return B;
    return A + f * (B - A);
}

// :1085-1104
__device__ inline float blend_conf_extrapol(float left, float right, float A, float B, double a, double b, double x)
{
    const float f = (a == b) ? 0 : ((x - a) / (b - a));
    if (f == 0) return A;
    if (f == 1) return B;
    if ((f >= left) && (f <= right)) return A + f * (B - A);
    return undefined_f();
}

// intFunc(&v0, &v1, out, 1, a, b, x) of :482 for the seven methods of :333-341
__device__ inline float blend(int method, float A, float B, double a, double b, double x)
{
    switch (method) {
    case FIMEX_AMD_VINT_METHOD_NN: return A;  // :1030-1034
    case FIMEX_AMD_VINT_METHOD_LIN: return blend_linear(A, B, a, b, x);
    case FIMEX_AMD_VINT_METHOD_LIN_WEAK_EXTRA: return blend_conf_extrapol(-1.f, 2.f, A, B, a, b, x);
    case FIMEX_AMD_VINT_METHOD_LIN_NO_EXTRA: return blend_conf_extrapol(0.f, 1.f, A, B, a, b, x);
    case FIMEX_AMD_VINT_METHOD_LIN_CONST_EXTRA: {  // :1115-1126
        const float f = (a == b) ? 0 : ((x - a) / (b - a));
        if (f >= 1) return B;
        if (f <= 0) return A;
        return A + f * (B - A);
    }
    case FIMEX_AMD_VINT_METHOD_LOG:  // :1131-1142; MIFI_ERROR leaves the reference's element unset: NaN here
        if (a <= 0 || b <= 0 || x <= 0) return undefined_f();
        return blend_linear(A, B, log(a), log(b), log(x));
    default: {  // LOGLOG, :1144-1156
        if (a <= 0 || b <= 0 || x <= 0) return undefined_f();
        const double la = log(a + M_E), lb = log(b + M_E), lx = log(x + M_E);
        if (la <= 0 || lb <= 0 || lx <= 0) return undefined_f();
        return blend_linear(A, B, log(la), log(lb), log(lx));
    }
    }
}

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
__device__ __noinline__ int monotonic_pair(const Column& in, int n, int mono, double x)
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
__device__ inline void walk_pairs(const Column& in, unsigned nzi, const double (&x)[kGroup], unsigned (&first)[kGroup], unsigned (&second)[kGroup])
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

// kGroup: output levels walked together
template <int kGroup>
__global__ void __launch_bounds__(kBlock) vertical_kernel(const VintArgs a)
{
    const size_t cell = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= a.plane) return;
    const size_t t = blockIdx.y;
    const unsigned nzi = a.in.nz;
    const bool fixed = a.out.kind < 0;
    const Column in(a.in, t, cell, a.plane);
    const Column out(fixed ? a.in : a.out, t, cell, a.plane);
    const double vMin = a.validMin ? a.validMin[cell] : 0.0, vMax = a.validMax ? a.validMax[cell] : 0.0;
    const float* dataCol = a.data + t * nzi * a.plane + cell;
    float* resCol = a.result + t * a.nzo * a.plane + cell;

    int mono = 0;  // +1 / -1: the column's levels are strictly increasing / decreasing (a NaN level makes it neither)
    if (a.bisect && nzi >= 2) {
        bool inc = true, dec = true;
        float prev = in.level(0);
        for (unsigned k = 1; k < nzi; ++k) {
            const float cur = in.level(k);
            inc &= prev < cur;
            dec &= prev > cur;
            prev = cur;
        }
        mono = inc ? 1 : dec ? -1 : 0;
    }

    for (unsigned k0 = 0; k0 < a.nzo; k0 += kGroup) {
        double x[kGroup];
        unsigned first[kGroup], second[kGroup];  // pos.first / pos.second of :476
        bool walk[kGroup], anyWalk = false;
#pragma unroll
        for (int g = 0; g < kGroup; ++g) {
            const unsigned k = min(k0 + g, a.nzo - 1);  // a short last group repeats its last level; only k0 + g < nzo is stored
            x[g] = fixed ? a.level1[k] : (double)out.level(k);  // :451
            const int pair = monotonic_pair(in, (int)nzi, mono, x[g]);
            walk[g] = pair < 0;
            first[g] = (unsigned)pair & 0xffffu;
            second[g] = (unsigned)pair >> 16;
            anyWalk |= walk[g];
        }
        if (anyWalk) {
            unsigned wFirst[kGroup], wSecond[kGroup];
            walk_pairs<kGroup>(in, nzi, x, wFirst, wSecond);
#pragma unroll
            for (int g = 0; g < kGroup; ++g)
                if (walk[g]) { first[g] = wFirst[g]; second[g] = wSecond[g]; }
        }
#pragma unroll
        for (int g = 0; g < kGroup; ++g) {
            if (k0 + g >= a.nzo) break;
            bool range = true;  // :454-471
            if (a.validMin && a.validMax) range = (x[g] >= vMin) && (x[g] <= vMax);
            else if (a.validMin) range = (x[g] >= vMin);
            else if (a.validMax) range = (x[g] <= vMax);
            float v = undefined_f();
            if (range && first[g] != second[g]) {  // nzi == 0 never gets here: the host refuses it
                const float v0 = dataCol[(size_t)first[g] * a.plane], v1 = dataCol[(size_t)second[g] * a.plane];
                const float l0 = in.level(first[g]), l1 = in.level(second[g]);
                v = blend(a.method, v0, v1, (double)l0, (double)l1, x[g]);
            }
            // :494-504 (a NaN bound compares false, as the reference's isnan() test skips it)
            if (v < a.clampMin) v = a.clampMin;
            if (v > a.clampMax) v = a.clampMax;
            resCol[(size_t)(k0 + g) * a.plane] = v;
        }
    }
}

__global__ void __launch_bounds__(kBlock) levels_kernel(const Levels L, size_t plane, float* __restrict__ result)
{
    const size_t cell = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= plane) return;
    const size_t t = blockIdx.y;
    const Column col(L, t, cell, plane);
    float* res = result + t * L.nz * plane + cell;
    for (unsigned k = 0; k < L.nz; ++k) res[(size_t)k * plane] = col.level(k);
}

}  // namespace

// unknown kind, NULL where the kind needs an array
void check_vertical_levels(const fimex_amd_vertical_levels* l, const char* which, bool nonEmpty)
{
    const std::string w(which);
    FA_REQUIRE(l != nullptr, "NULL " + w + " level description");
    FA_REQUIRE(l->nz <= 0x7fffffffu, w + " levels: nz out of range");
    const bool need = nonEmpty && l->nz > 0;
    switch (l->kind) {
    case FIMEX_AMD_VLEVEL_FIELD:
        FA_REQUIRE(!need || l->field != nullptr, w + " levels: kind FIELD needs the level field");
        break;
    case FIMEX_AMD_VLEVEL_AXIS:
        FA_REQUIRE(l->nz == 0 || l->axis != nullptr, w + " levels: kind AXIS needs axis[nz]");
        break;
    case FIMEX_AMD_VLEVEL_SIGMA:
        FA_REQUIRE(l->nz == 0 || l->sigma != nullptr, w + " levels: kind SIGMA needs sigma[nz]");
        FA_REQUIRE(!need || l->ps != nullptr, w + " levels: kind SIGMA needs ps");
        break;
    case FIMEX_AMD_VLEVEL_HYBRID_SIGMA:
        FA_REQUIRE(l->nz == 0 || (l->a != nullptr && l->b != nullptr), w + " levels: kind HYBRID_SIGMA needs a[nz] and b[nz]");
        FA_REQUIRE(!need || l->ps != nullptr, w + " levels: kind HYBRID_SIGMA needs ps");
        break;
    case FIMEX_AMD_VLEVEL_HYBRID_SIGMA_AP:
        FA_REQUIRE(l->nz == 0 || (l->ap != nullptr && l->b != nullptr), w + " levels: kind HYBRID_SIGMA_AP needs ap[nz] and b[nz]");
        FA_REQUIRE(!need || l->ps != nullptr, w + " levels: kind HYBRID_SIGMA_AP needs ps");
        break;
    default:
        throw Error("unknown vertical level kind " + std::to_string(l->kind));
    }
}


bool vertical_method_known(int method) { return method >= FIMEX_AMD_VINT_METHOD_LIN && method <= FIMEX_AMD_VINT_METHOD_LIN_CONST_EXTRA; }

// every argument has been checked (capi.hip); the pointers in the two descriptions are device pointers except the coefficients
void launch_vertical_interpolate(int method, size_t nx, size_t ny, size_t nt, const float* d_in, const fimex_amd_vertical_levels& inLevels,
                                 const fimex_amd_vertical_levels* outLevels, const double* h_level1, size_t nzo, const double* d_validMin,
                                 const double* d_validMax, float clampMin, float clampMax, float* d_out, hipStream_t stream)
{
    const size_t plane = nx * ny;
    if (plane == 0 || nt == 0 || nzo == 0) return;
    const dim3 grid = column_grid(plane, nt);
    StreamScratch scratch(coefficient_count(inLevels) + (outLevels ? coefficient_count(*outLevels) : nzo), stream);
    VintArgs a{};
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
    a.data = d_in;
    a.result = d_out;
    a.plane = plane;
    a.nzo = (unsigned)nzo;
    a.method = method;
    a.clampMin = clampMin;
    a.clampMax = clampMax;
    a.bisect = tuning("VERTICAL_BISECT", 1);
    // output levels per walk of a column, measured: 4 is faster than 8, whose registers leave 2 waves per SIMD
    if (tuning("VERTICAL_GROUP", 4) == 8) vertical_kernel<8><<<grid, kBlock, 0, stream>>>(a);
    else vertical_kernel<4><<<grid, kBlock, 0, stream>>>(a);
    FA_HIP(hipGetLastError());
}

void launch_vertical_levels(const fimex_amd_vertical_levels& levels, size_t nx, size_t ny, size_t nt, float* d_out, hipStream_t stream)
{
    const size_t plane = nx * ny;
    if (plane == 0 || nt == 0 || levels.nz == 0) return;
    const dim3 grid = column_grid(plane, nt);
    StreamScratch scratch(coefficient_count(levels), stream);
    const Levels L = device_levels(levels, scratch, stream);
    levels_kernel<<<grid, kBlock, 0, stream>>>(L, plane, d_out);
    FA_HIP(hipGetLastError());
}

}  // namespace fimex_amd
