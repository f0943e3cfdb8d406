// Vertical interpolation in two halves: a plan that holds the search of vertical.hip, and an apply that only
// gathers two values per output cell, blends, clamps and stores -- on the variable's stored type, for several variables at once.
//
// Build: vertical_kernel's shape and search (vertical_search.hpp: a lane per column, output levels in groups of kGroup,
// bisection or the reference's walk), storing the pair and the folded factor (blend_math.hpp) of every output cell instead of
// gathering data.
//
// Apply: a workgroup owns kBlock groups of 16 bytes of output along x and walks the output levels, so that the lines of an input
// plane it has just read are still in L2 when the next level comes back to them.  Per group a lane loads its entries (16-byte
// loads), fetches the two data values per cell -- one 16-byte load per side where the cells of the group share the level and
// the address allows it, as they mostly do: neighbouring columns bracket a target with the same two levels -- and stores 16 bytes.
// A row of a level starts off a 16-byte boundary where the plane is no multiple of the group: the cells in front of the first
// whole group and behind the last go one by one.  The variables of a launch are compile-time many, their pointers are indexed
// by constants and stay in SGPRs.  No LDS, no atomics, no workgroup waits for another.
#include "vertical_plan.hpp"
#include "typed_convert.hpp"
#include "vertical_search.hpp"

#include <algorithm>
#include <vector>

namespace fimex_amd {

namespace {

struct PlanArgs {
    Levels in, out;          // out.kind < 0: fixed levels (level1)
    const double* level1;    // device, [nzo]
    const double* validMin;  // [plane] or NULL
    const double* validMax;
    uint32_t* pair;          // [nt][nzo][plane]
    float* factor;
    size_t plane;
    unsigned nzo;
    int method;
    int bisect;  // 0: every column is walked (tuning build)
};

// intFunc of src/CDMVerticalInterpolator.cc:333-341 (src/interpolation.c:1030-1156 with n = 1) folded into one factor: the cell's
// value is f == 0 ? A : f == 1 ? B : A + f * (B - A) for every method.  false: the cell is undefined.
__device__ inline bool entry_factor(int method, double a, double b, double x, float& f)
{
    if (method == FIMEX_AMD_VINT_METHOD_NN) {  // :1030-1034
        f = 0.f;
        return true;
    }
    if (method == FIMEX_AMD_VINT_METHOD_LOG && !log_coordinates(a, b, x)) return false;
    if (method == FIMEX_AMD_VINT_METHOD_LOGLOG && !loglog_coordinates(a, b, x)) return false;
    f = linear_factor(a, b, x);
    switch (method) {
    case FIMEX_AMD_VINT_METHOD_LIN_CONST_EXTRA:  // :1115-1126
        if (f >= 1) f = 1.f;
        else if (f <= 0) f = 0.f;
        return true;
    case FIMEX_AMD_VINT_METHOD_LIN_WEAK_EXTRA: return f == 0 || f == 1 || ((f >= -1.f) && (f <= 2.f));  // :1085-1104
    case FIMEX_AMD_VINT_METHOD_LIN_NO_EXTRA: return f == 0 || f == 1 || ((f >= 0.f) && (f <= 1.f));
    default: return true;
    }
}

// vertical_kernel (vertical.hip) up to the pair of input levels; kGroup: output levels walked together
template <int kGroup>
__global__ void __launch_bounds__(kBlock) plan_build_kernel(const PlanArgs a)
{
    const size_t cell = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= a.plane) return;
    const size_t t = blockIdx.y;
    const unsigned nzi = a.in.nz;
    const bool fixed = a.out.kind < 0;
    const Column in(a.in, t, cell, a.plane);
    const Column out(fixed ? a.in : a.out, t, cell, a.plane);
    const double vMin = a.validMin ? a.validMin[cell] : 0.0, vMax = a.validMax ? a.validMax[cell] : 0.0;
    uint32_t* pairCol = a.pair + t * a.nzo * a.plane + cell;
    float* factorCol = a.factor + t * a.nzo * a.plane + cell;

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
            float f = 0.f;
            bool defined = false;
            if (range && first[g] != second[g]) {  // nzi == 0 never gets here: the host refuses it
                const float l0 = in.level(first[g]), l1 = in.level(second[g]);
                defined = entry_factor(a.method, (double)l0, (double)l1, x[g], f);
            }
            // an undefined cell keeps its first level on both sides: the apply still reads the plane its neighbours read
            pairCol[(size_t)(k0 + g) * a.plane] = first[g] | ((defined ? second[g] : first[g]) << 16);
            factorCol[(size_t)(k0 + g) * a.plane] = defined ? f : 0.f;
        }
    }
}

// ---- apply

template <typename T, int NV>
struct ApplyArgs {
    const uint32_t* pair;  // [nt][nzo][plane]
    const float* factor;
    const T* in[NV];       // [nt][nzi][plane]
    T* out[NV];            // [nt][nzo][plane]
    float bad[NV];         // the fill value narrowed to float, as mifi_bad2nanf takes it
    int hasBad[NV];
    int plainFloat[NV];    // T == float without a fill value: an interpolation array, stored as it is
    T fill[NV];
    float clampMin[NV], clampMax[NV];
    size_t plane;
    unsigned nzi, nzo;
    unsigned off;          // elements between a 16-byte boundary and out[v][0], the same for every v of a launch
};

template <typename T, int V>
struct alignas(V * sizeof(T) < 16 ? V * sizeof(T) : 16) Pack {
    T v[V];
};

// the data values of V x-adjacent cells on one side of their pairs (shift 0: first, 16: second); col points at level 0 of the first cell
template <typename T, int V>
__device__ __forceinline__ void gather(const T* col, size_t plane, const uint32_t (&pr)[V], int shift, float bad, bool hasBad, float (&r)[V])
{
    if (V > 1) {
        bool same = true;
#pragma unroll
        for (int c = 1; c < V; ++c) same &= ((pr[c] >> shift) & 0xffffu) == ((pr[0] >> shift) & 0xffffu);
        const T* p = col + (size_t)((pr[0] >> shift) & 0xffffu) * plane;
        if (same && reinterpret_cast<uintptr_t>(p) % sizeof(Pack<T, V>) == 0) {
            const Pack<T, V> x = *reinterpret_cast<const Pack<T, V>*>(p);
#pragma unroll
            for (int c = 0; c < V; ++c) r[c] = as_float_nan<T>(x.v[c], bad, hasBad);
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < V; ++c) r[c] = as_float_nan<T>(col[(size_t)((pr[c] >> shift) & 0xffffu) * plane + c], bad, hasBad);
}

// V x-adjacent cells of one output row, from `cell` on, for every variable of the launch; vec: the entries and the outputs of
// the V cells are one aligned pack each
template <typename T, int V, int NV>
__device__ __forceinline__ void apply_cells(const ApplyArgs<T, NV>& a, size_t t, size_t rowStart, size_t cell, bool vecEntries)
{
    uint32_t pr[V];
    float f[V];
    const size_t e = rowStart + cell;
    if (V > 1 && vecEntries) {
        const Pack<uint32_t, V> p = *reinterpret_cast<const Pack<uint32_t, V>*>(a.pair + e);
        const Pack<float, V> q = *reinterpret_cast<const Pack<float, V>*>(a.factor + e);
#pragma unroll
        for (int c = 0; c < V; ++c) { pr[c] = p.v[c]; f[c] = q.v[c]; }
    } else {
#pragma unroll
        for (int c = 0; c < V; ++c) { pr[c] = a.pair[e + c]; f[c] = a.factor[e + c]; }
    }
    const size_t col = t * a.nzi * a.plane + cell;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        float A[V], B[V];
        gather<T, V>(a.in[v] + col, a.plane, pr, 0, a.bad[v], a.hasBad[v] != 0, A);
        gather<T, V>(a.in[v] + col, a.plane, pr, 16, a.bad[v], a.hasBad[v] != 0, B);
        Pack<T, V> o;
#pragma unroll
        for (int c = 0; c < V; ++c) {
            float y = FA_BM_VALUE_OF_FOLDED(f[c], A[c], B[c]);  // blend_math.hpp
            if ((pr[c] & 0xffffu) == (pr[c] >> 16)) y = undefined_f();
            // src/CDMVerticalInterpolator.cc:494-504 (a NaN bound compares false, as the reference's isnan() test skips it)
            if (y < a.clampMin[v]) y = a.clampMin[v];
            if (y > a.clampMax[v]) y = a.clampMax[v];
            if (std::is_same<T, float>::value && a.plainFloat[v]) o.v[c] = (T)y;
            else o.v[c] = from_float_fill<T>(y, a.fill[v]);
        }
        *reinterpret_cast<Pack<T, V>*>(a.out[v] + e) = o;
    }
}

template <typename T, int NV>
__global__ void __launch_bounds__(kBlock) plan_apply_kernel(const ApplyArgs<T, NV> a)
{
    constexpr int V = 16 / sizeof(T);
    const size_t t = blockIdx.y;
    const size_t lane = (size_t)blockIdx.x * kBlock + threadIdx.x;
    for (unsigned k = 0; k < a.nzo; ++k) {
        const size_t rowStart = (t * a.nzo + k) * a.plane;
        // cells of this row in front of the first 16-byte group of the outputs
        size_t head = (V - (rowStart + a.off) % V) % V;
        if (head > a.plane) head = a.plane;
        const size_t groups = (a.plane - head) / V, tail0 = head + groups * V, singles = head + (a.plane - tail0);
        if (lane < groups) apply_cells<T, V, NV>(a, t, rowStart, head + (size_t)V * lane, a.off == 0);
        if (lane < singles) apply_cells<T, 1, NV>(a, t, rowStart, lane < head ? lane : tail0 + (lane - head), false);
    }
}

template <typename T, int NV>
void launch_apply(const fimex_amd_vertical_plan& plan, const VerticalPlanVar* const* vars, unsigned off, hipStream_t stream)
{
    constexpr size_t V = 16 / sizeof(T);
    ApplyArgs<T, NV> a{};
    a.pair = plan.pair.get();
    a.factor = plan.factor.get();
    for (int v = 0; v < NV; ++v) {
        const VerticalPlanVar& var = *vars[v];
        a.in[v] = static_cast<const T*>(var.in);
        a.out[v] = static_cast<T*>(var.out);
        a.bad[v] = (float)var.badValue;  // the double fill value narrows to mifi_bad2nanf's float parameter (CDMInterpolator.cc:117)
        a.hasBad[v] = !(a.bad[v] != a.bad[v]);
        a.plainFloat[v] = std::is_same<T, float>::value && var.badValue != var.badValue;
        a.fill[v] = a.plainFloat[v] ? T(0) : static_cast<T>(var.badValue);  // ScaleValue's newFill_ (Utils.h:456)
        a.clampMin[v] = var.clampMin;
        a.clampMax[v] = var.clampMax;
    }
    a.plane = plan.info.nx * plan.info.ny;
    a.nzi = (unsigned)plan.info.nzi;
    a.nzo = (unsigned)plan.info.nzo;
    a.off = off;
    // a row holds at most plane / V whole groups and 2 (V - 1) single cells
    const size_t lanes = std::max(a.plane / V + 1, 2 * (V - 1));
    FA_REQUIRE(plan.info.nt <= 65535, "at most 65535 unlimited-dimension positions per plan");
    FA_REQUIRE(ceil_div(lanes, kBlock) <= 0x7fffffffu, "horizontal plane too large");
    const dim3 grid((unsigned)ceil_div(lanes, kBlock), (unsigned)plan.info.nt, 1);
    plan_apply_kernel<T, NV><<<grid, kBlock, 0, stream>>>(a);
    FA_HIP(hipGetLastError());
}

}  // namespace

// every argument has been checked (capi_vertical_plan.hip); the pointers in the two descriptions are device pointers except the coefficients
void build_vertical_plan(fimex_amd_vertical_plan& plan, const fimex_amd_vertical_levels& inLevels, const fimex_amd_vertical_levels* outLevels,
                         const double* h_level1, const double* d_validMin, const double* d_validMax, hipStream_t stream)
{
    const size_t plane = plan.info.nx * plan.info.ny, nt = plan.info.nt, nzo = plan.info.nzo;
    if (plane * nt > 0) {
        const dim3 grid = column_grid(plane, nt);
        StreamScratch scratch(search_scratch_doubles(inLevels, outLevels, nzo), stream);
        PlanArgs a{};
        fill_search_args(a, plan.info.method, inLevels, outLevels, h_level1, nzo, d_validMin, d_validMax, plane, scratch, stream);
        a.pair = plan.pair.get();
        a.factor = plan.factor.get();
        for_search_group([&](auto group) { plan_build_kernel<decltype(group)::value><<<grid, kBlock, 0, stream>>>(a); });
        FA_HIP(hipGetLastError());
    }
    FA_HIP(hipEventRecord(plan.built.e, stream));
}

// every argument has been checked: nvar >= 1, the pointers are aligned to the element size
void launch_vertical_plan_apply(const fimex_amd_vertical_plan& plan, const VerticalPlanVar* vars, size_t nvar, int cdmType, hipStream_t stream)
{
    if (plan.pair.size() == 0) return;
    for_cdm_type(cdmType, [&](auto tag) {
        using T = decltype(tag);
        // a launch takes variables whose outputs lie alike to a 16-byte boundary: they share the head of every row
        std::vector<const VerticalPlanVar*> byOff[16 / sizeof(T)];
        for (size_t i = 0; i < nvar; ++i) byOff[(reinterpret_cast<uintptr_t>(vars[i].out) % 16) / sizeof(T)].push_back(&vars[i]);
        for (unsigned off = 0; off < 16 / sizeof(T); ++off) {
            const std::vector<const VerticalPlanVar*>& g = byOff[off];
            size_t i = 0;
            for (; i + 4 <= g.size(); i += 4) launch_apply<T, 4>(plan, &g[i], off, stream);
            if (i + 2 <= g.size()) { launch_apply<T, 2>(plan, &g[i], off, stream); i += 2; }
            if (i < g.size()) launch_apply<T, 1>(plan, &g[i], off, stream);
        }
    });
}

}  // namespace fimex_amd
