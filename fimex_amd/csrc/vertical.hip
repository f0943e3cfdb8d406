// Vertical interpolation of [nt][nzi][ny][nx] to fixed or template levels: the loop of
// CDMVerticalInterpolator::getLevelDataSlice, src/CDMVerticalInterpolator.cc:441-504, restated per column.
//
// A lane owns one column; consecutive lanes own x-adjacent columns, so every load of a level plane, a data plane or ps is
// coalesced along x.  The search (vertical_search.hpp) is what vertical_plan.hip shares; the factor and the log coordinates
// of the blend are blend_math.hpp's.  In a column whose levels are strictly monotonic the pair of input levels around a target comes from a
// bisection (monotonic_pair); otherwise, and wherever the bisection cannot be sure, from the reference's walk: output levels
// go in groups of kGroup and the scan of include/fimex/Utils.h:251-290 runs once over the column's input levels for the whole
// group, with its state (lowDiff, highDiff, lowest, highest per output level) in registers.  Levels given by a formula are recomputed from ps in every pass (two FP64 operations, no memory), an explicit
// level field is re-read (nzo / kGroup times, from L2 / Infinity Cache: the lanes of a workgroup come back to the lines they
// have just read).  The data column is not streamed at all: once a pair of input levels is known the two values are fetched
// from their planes, neighbouring lanes mostly from the same two.  No workgroup waits for another one.
#include "vertical_search.hpp"

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
    const float f = linear_factor(a, b, x);
    if (f == 0) return A;
    if (f == 1) return B;
    return A + f * (B - A);
}

// :1085-1104
__device__ inline float blend_conf_extrapol(float left, float right, float A, float B, double a, double b, double x)
{
    const float f = linear_factor(a, b, x);
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
        const float f = linear_factor(a, b, x);
        if (f >= 1) return B;
        if (f <= 0) return A;
        return A + f * (B - A);
    }
    case FIMEX_AMD_VINT_METHOD_LOG:  // :1131-1142; MIFI_ERROR leaves the reference's element unset: NaN here
        if (!log_coordinates(a, b, x)) return undefined_f();
        return blend_linear(A, B, a, b, x);
    default:  // LOGLOG, :1144-1156
        if (!loglog_coordinates(a, b, x)) return undefined_f();
        return blend_linear(A, B, a, b, x);
    }
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

bool check_vertical_search(int method, size_t nx, size_t ny, size_t nt, const fimex_amd_vertical_levels* inLevels,
                           const fimex_amd_vertical_levels* outLevels, const double* level1, size_t nzo, bool emptyIsDone)
{
    FA_REQUIRE(vertical_method_known(method), "unknown vertical interpolation method " + std::to_string(method));
    const bool nonEmpty = nx * ny * nt > 0;
    check_vertical_levels(inLevels, "input", nonEmpty);
    if (outLevels) {
        check_vertical_levels(outLevels, "template", nonEmpty);
        FA_REQUIRE(outLevels->nz == nzo, "nzo differs from the template's number of levels");
    }
    // differs: on an empty grid the one-shot entries have nothing to do and ask no more; the plan's create asks regardless
    if (emptyIsDone && !nonEmpty) return false;
    FA_REQUIRE(outLevels != nullptr || level1 != nullptr, "fixed levels need level1[nzo]");
    FA_REQUIRE(inLevels->nz > 0, "no input levels (nzi == 0)");
    FA_REQUIRE(nzo > 0, "no output levels (nzo == 0)");
    return true;
}

// every argument has been checked (capi.hip); the pointers in the two descriptions are device pointers except the coefficients
void launch_vertical_interpolate(int method, size_t nx, size_t ny, size_t nt, const float* d_in, const fimex_amd_vertical_levels& inLevels,
                                 const fimex_amd_vertical_levels* outLevels, const double* h_level1, size_t nzo, const double* d_validMin,
                                 const double* d_validMax, float clampMin, float clampMax, float* d_out, hipStream_t stream)
{
    const size_t plane = nx * ny;
    if (plane == 0 || nt == 0 || nzo == 0) return;
    const dim3 grid = column_grid(plane, nt);
    StreamScratch scratch(search_scratch_doubles(inLevels, outLevels, nzo), stream);
    VintArgs a{};
    fill_search_args(a, method, inLevels, outLevels, h_level1, nzo, d_validMin, d_validMax, plane, scratch, stream);
    a.data = d_in;
    a.result = d_out;
    a.clampMin = clampMin;
    a.clampMax = clampMax;
    for_search_group([&](auto group) { vertical_kernel<decltype(group)::value><<<grid, kBlock, 0, stream>>>(a); });
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
