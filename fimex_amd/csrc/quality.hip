// Quality masking: CDMQualityExtractor::getDataSlice (src/CDMQualityExtractor.cc:239-391), in place.  A cell of the
// data gets the fill value where the status of its position inside the status slice fails the rule; the status repeats along the
// slow dimensions of the data (:377-385) and is read as Data::asDouble().
//
// One streaming pass over (data type, status type).  A lane evaluates the rule once for the status cells under one 16-byte group
// of data and then walks the repeats: nothing masked means no access to the data at all, everything masked one
// 16-byte store per repeat, anything between load, merge, store.  The groups start `head` cells into a repeat, where the data is
// 16-byte aligned; the cells in front and behind the last whole group go one by one, and so does everything where the repeats
// start at different alignments.
// A lane reads the status of a group before it writes the group, and groups are disjoint, so the status may be the data itself.
// Value lists of up to kByValue entries are kernel arguments, longer ones go through stream-ordered scratch and a binary search.
// HIGHEST and LOWEST first reduce the defined status values in two stages into that scratch; nothing returns to the host.
#include "vertical_common.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <type_traits>
#include <vector>

namespace fimex_amd {

namespace {

constexpr int kByValue = 8;
constexpr unsigned kMaxPartials = 1024;

template <typename T, int N>
struct alignas(16) Group {
    T v[N];
};

struct Rule {
    int mode;
    double limit, validMin, validMax, statusFill;  // NaN: no such bound (every comparison with it is false)
    const double* extreme;                         // HIGHEST / LOWEST: the extreme of the defined status values, NaN where none is
    const double* list;                            // VALUES with more than kByValue entries: sorted, on the device
    unsigned nList;
    double v[kByValue];  // a shorter list: padded with its first entry

    // :304-330, the status that survives valid_min / valid_max / _FillValue
    __device__ __forceinline__ bool defined(double s) const { return !(s != s) && !(s < validMin) && !(s > validMax) && !(s == statusFill); }

    __device__ __forceinline__ bool listed(double s) const
    {
        if (!list) {
            bool hit = false;
#pragma unroll
            for (int k = 0; k < kByValue; ++k) hit |= (s == v[k]);
            return hit;
        }
        unsigned lo = 0, hi = nList;  // std::binary_search, :370
        while (lo < hi) {
            const unsigned mid = lo + (hi - lo) / 2;
            if (list[mid] < s) lo = mid + 1;
            else hi = mid;
        }
        return lo < nList && list[lo] == s;
    }

    // the cell gets the fill value (:380): a NaN status in every mode
    __device__ __forceinline__ bool masked(double s, double ext) const
    {
        if (s != s) return true;
        if (mode == FIMEX_AMD_QUALITY_VALUES) return !listed(s);
        if (!defined(s)) return true;
        switch (mode) {
        case FIMEX_AMD_QUALITY_MAX: return s > limit;  // :339
        case FIMEX_AMD_QUALITY_MIN: return s < limit;  // :349
        case FIMEX_AMD_QUALITY_HIGHEST:
        case FIMEX_AMD_QUALITY_LOWEST: return !(s == ext);  // include/fimex/CDMQualityExtractor.h; divergence D8
        default: return false;                              // ALL
        }
    }
};

__device__ __forceinline__ double pick(double a, double b, bool highest)
{
    if (a != a) return b;
    if (b != b) return a;
    return highest ? (b > a ? b : a) : (b < a ? b : a);
}

__device__ __forceinline__ double block_pick(double best, bool highest)
{
    __shared__ double sh[kBlock];
    sh[threadIdx.x] = best;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w /= 2) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] = pick(sh[threadIdx.x], sh[threadIdx.x + w], highest);
        __syncthreads();
    }
    return sh[0];
}

template <typename S>
__global__ void __launch_bounds__(kBlock) extreme_partial_kernel(const S* __restrict__ status, size_t n, const Rule r, bool highest,
                                                                 double* __restrict__ partial)
{
    const size_t stride = (size_t)gridDim.x * kBlock;
    double best = __builtin_nan("");
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double s = (double)status[i];
        if (r.defined(s)) best = pick(best, s, highest);
    }
    best = block_pick(best, highest);
    if (threadIdx.x == 0) partial[blockIdx.x] = best;
}

__global__ void __launch_bounds__(kBlock) extreme_final_kernel(const double* __restrict__ partial, unsigned count, bool highest,
                                                               double* __restrict__ extreme)
{
    double best = __builtin_nan("");
    for (unsigned i = threadIdx.x; i < count; i += kBlock) best = pick(best, partial[i], highest);
    best = block_pick(best, highest);
    if (threadIdx.x == 0) *extreme = best;
}

template <typename C, typename S>
__global__ void __launch_bounds__(kBlock) mask_kernel(C* data, const S* status, size_t nStatus, size_t repeats, size_t head, const Rule r,
                                                      const C fill)
{
    constexpr int kPer = 16 / sizeof(C);
    constexpr unsigned kAll = (1u << kPer) - 1;
    const double ext = r.extreme ? *r.extreme : 0.0;
    const size_t stride = (size_t)gridDim.x * kBlock, lane = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t groups = (nStatus - head) / kPer;
    for (size_t g = lane; g < groups; g += stride) {
        const size_t i0 = head + g * kPer;
        unsigned m = 0;
#pragma unroll
        for (int e = 0; e < kPer; ++e) m |= (r.masked((double)status[i0 + e], ext) ? 1u : 0u) << e;
        if (!m) continue;
        for (size_t rep = 0; rep < repeats; ++rep) {
            Group<C, kPer>* p = reinterpret_cast<Group<C, kPer>*>(data + rep * nStatus + i0);
            Group<C, kPer> x;
            if (m != kAll) x = *p;
#pragma unroll
            for (int e = 0; e < kPer; ++e)
                if ((m >> e) & 1u) x.v[e] = fill;
            *p = x;
        }
    }
    const size_t tail0 = head + groups * kPer, single = head + (nStatus - tail0);
    for (size_t j = lane; j < single; j += stride) {
        const size_t i = j < head ? j : tail0 + (j - head);
        if (!r.masked((double)status[i], ext)) continue;
        for (size_t rep = 0; rep < repeats; ++rep) data[rep * nStatus + i] = fill;
    }
}

// data_caster<C, double> (include/fimex/Utils.h:85-115): through MetNoFimex::round, an int, for an integer C
template <typename C>
C cast_fill(double v)
{
    if (std::is_integral<C>::value) return static_cast<C>(static_cast<int>(std::lround(v)));
    return static_cast<C>(v);
}

template <typename C>
bool fill_representable(double v)
{
    if (std::is_same<C, float>::value) return !std::isfinite(v) || std::fabs(v) <= (double)std::numeric_limits<float>::max();
    if (std::is_floating_point<C>::value) return true;
    if (!(std::fabs(v) < 9223372036854775808.0)) return false;  // NaN, or lround is unspecified
    return (double)cast_fill<C>(v) == std::round(v);
}

// cells in front of the first 16-byte group of a repeat; nStatus where the repeats do not all start at the alignment of the first
template <typename C>
size_t head_cells(const C* data, size_t nStatus, size_t repeats)
{
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(data);
    if (d0 % sizeof(C) || (repeats > 1 && (nStatus * sizeof(C)) % 16)) return nStatus;
    return std::min<size_t>(((16 - d0 % 16) % 16) / sizeof(C), nStatus);
}

template <typename C, typename S>
void launch_mask(C* data, size_t nData, const S* status, size_t nStatus, const QualityRule& q, double fillValue, hipStream_t stream)
{
    Rule r{};
    r.mode = q.mode;
    r.limit = q.limit;
    r.validMin = q.validMin;
    r.validMax = q.validMax;
    r.statusFill = q.statusFill;
    const bool byExtreme = q.mode == FIMEX_AMD_QUALITY_HIGHEST || q.mode == FIMEX_AMD_QUALITY_LOWEST;
    const bool longList = q.mode == FIMEX_AMD_QUALITY_VALUES && q.nValues > (size_t)kByValue;
    FA_REQUIRE(q.nValues <= std::numeric_limits<unsigned>::max(), "more status values than 32 bits count");
    const unsigned partials = byExtreme ? (unsigned)std::min<size_t>(ceil_div(nStatus, kBlock), kMaxPartials) : 0;
    StreamScratch scratch(byExtreme ? partials + 1 : (longList ? q.nValues : 0), stream);  // freed on the stream, behind the mask kernel
    if (byExtreme) {
        const bool highest = q.mode == FIMEX_AMD_QUALITY_HIGHEST;
        double* partial = scratch.take(partials);
        double* extreme = scratch.take(1);
        extreme_partial_kernel<S><<<partials, kBlock, 0, stream>>>(status, nStatus, r, highest, partial);
        FA_HIP(hipGetLastError());
        extreme_final_kernel<<<1, kBlock, 0, stream>>>(partial, partials, highest, extreme);
        FA_HIP(hipGetLastError());
        r.extreme = extreme;
    } else if (longList) {
        double* list = scratch.take(q.nValues);
        upload(list, q.h_values, q.nValues, stream);
        r.list = list;
        r.nList = (unsigned)q.nValues;
    } else if (q.mode == FIMEX_AMD_QUALITY_VALUES) {
        for (int k = 0; k < kByValue; ++k) r.v[k] = q.h_values[(size_t)k < q.nValues ? k : 0];
    }
    constexpr size_t kPer = 16 / sizeof(C);
    const size_t repeats = nData / nStatus, head = head_cells(data, nStatus, repeats);
    const size_t groups = (nStatus - head) / kPer, single = nStatus - groups * kPer;
    const size_t want = ceil_div(groups > single ? groups : single, kBlock);
    const size_t cap = std::max(1, tuning("QUALITY_MAX_BLOCKS", 256 * 8));
    mask_kernel<C, S><<<(unsigned)(want < cap ? want : cap), kBlock, 0, stream>>>(data, status, nStatus, repeats, head, r, cast_fill<C>(fillValue));
    FA_HIP(hipGetLastError());
}

}  // namespace

bool quality_mode_known(int mode) { return mode >= FIMEX_AMD_QUALITY_VALUES && mode <= FIMEX_AMD_QUALITY_LOWEST; }

bool quality_fill_representable(int cdmType, double fill)
{
    bool r = false;
    for_cdm_type(cdmType, [&](auto t) { r = fill_representable<decltype(t)>(fill); });
    return r;
}

// every argument has been checked (capi_time_quality.hip): nStatus > 0 divides nData > 0, the fill is representable, the value list
// of VALUES is sorted, not empty and holds no NaN
void launch_quality_mask(void* d_data, int dataType, size_t nData, const void* d_status, int statusType, size_t nStatus, const QualityRule& rule,
                         double fillValue, hipStream_t stream)
{
    for_cdm_type(dataType, [&](auto c) {
        for_cdm_type(statusType, [&](auto s) {
            using C = decltype(c);
            using S = decltype(s);
            launch_mask<C, S>(static_cast<C*>(d_data), nData, static_cast<const S*>(d_status), nStatus, rule, fillValue, stream);
        });
    });
}

}  // namespace fimex_amd
