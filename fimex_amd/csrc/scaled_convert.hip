// Scaled conversion between stored types: DataImpl<IN>::convertDataType -> ScaleValue<IN, OUT>
// (include/fimex/Utils.h:443-464, src/DataImpl.h:316-349) for every pair of the ten numeric CDM types, the step behind
// getScaledDataSliceInUnit on the way in and behind the writers' packing on the way out.
//
// One streaming kernel over (IN, OUT).  A lane converts groups of kPer = 16 / min(sizeof(IN), sizeof(OUT)) elements: the narrower
// side moves as one 16-byte access per lane, the wider side as several, every one of them 16 bytes.  The groups start `head`
// elements into the arrays, where both pointers are 16-byte aligned; the elements in front of them and behind the last whole group
// go one by one.  Where no such start exists (pointers whose misalignments differ) head = n and everything goes one by one.  A lane
// reads all of a group before it writes any of it and groups are disjoint, so out may be in itself when the sizes agree.  No LDS,
// no scratch; the grid is capped and strides.
#include "merge_math.hpp"
#include "plan.hpp"
#include "typed_convert.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <type_traits>

namespace fimex_amd {

namespace {

template <typename T, int N>
struct alignas(16) Group {
    T v[N];
};

// Utils.h:443-464, stated once in merge_math.hpp for the conversions and the merge on stored types.  A derived struct of this
// file's own and not a using-declaration on purpose: the kernels below take it by value, so its name is part of their mangled
// symbols, and those stay what they were before the arithmetic moved (the device assembly is unchanged but for the id symbol).
template <typename IN, typename OUT>
struct ScaleValue : merge_math::ScaleValue<IN, OUT> {};

template <typename IN, typename OUT>
__global__ void __launch_bounds__(kBlock) scaled_kernel(const IN* in, OUT* out, size_t n, size_t head, const ScaleValue<IN, OUT> sv)
{
    constexpr int kPer = 16 / (sizeof(IN) < sizeof(OUT) ? sizeof(IN) : sizeof(OUT));
    const size_t stride = (size_t)gridDim.x * kBlock, lane = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t groups = (n - head) / kPer;
    const Group<IN, kPer>* gin = reinterpret_cast<const Group<IN, kPer>*>(in + head);
    Group<OUT, kPer>* gout = reinterpret_cast<Group<OUT, kPer>*>(out + head);
    for (size_t g = lane; g < groups; g += stride) {
        const Group<IN, kPer> x = gin[g];
        Group<OUT, kPer> y;
#pragma unroll
        for (int e = 0; e < kPer; ++e) y.v[e] = sv(x.v[e]);
        gout[g] = y;
    }
    const size_t tail0 = head + groups * kPer, single = head + (n - tail0);
    for (size_t j = lane; j < single; j += stride) {
        const size_t i = j < head ? j : tail0 + (j - head);
        out[i] = sv(in[i]);
    }
}

using merge_math::representable;

// elements in front of the first group, or n where the two pointers never reach a 16-byte boundary together
template <typename IN, typename OUT>
size_t head_elements(const IN* in, const OUT* out, size_t n)
{
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), o0 = reinterpret_cast<uintptr_t>(out);
    for (size_t h = 0; h < 16 && h < n; ++h)
        if ((i0 + h * sizeof(IN)) % 16 == 0 && (o0 + h * sizeof(OUT)) % 16 == 0) return h;
    return n;
}

template <typename IN, typename OUT>
void launch_scaled(const void* d_in, size_t n, double oldFill, double a, double b, double newFill, void* d_out, hipStream_t stream)
{
    const IN* in = static_cast<const IN*>(d_in);
    OUT* out = static_cast<OUT*>(d_out);
    ScaleValue<IN, OUT> sv{};
    sv.hasFill = representable<IN>(oldFill);
    sv.oldFill = sv.hasFill ? static_cast<IN>(oldFill) : IN(0);
    sv.a = a;
    sv.b = b;
    sv.newFill = static_cast<OUT>(newFill);
    constexpr size_t kPer = 16 / (sizeof(IN) < sizeof(OUT) ? sizeof(IN) : sizeof(OUT));
    const size_t head = head_elements(in, out, n), groups = (n - head) / kPer, single = n - groups * kPer;
    const size_t want = ceil_div(groups > single ? groups : single, kBlock);
    const size_t cap = std::max(1, tuning("SCALED_MAX_BLOCKS", 256 * 8));
    scaled_kernel<IN, OUT><<<(unsigned)(want < cap ? want : cap), kBlock, 0, stream>>>(in, out, n, head, sv);
    FA_HIP(hipGetLastError());
}

}  // namespace

bool scaled_fill_representable(int cdmType, double fill)
{
    bool r = false;
    for_cdm_type(cdmType, [&](auto t) { r = representable<decltype(t)>(fill); });
    return r;
}

// every argument has been checked (capi_derived.hip); n > 0
void launch_convert_scaled(const void* d_in, int inType, size_t n, double oldFill, double oldScale, double oldOffset, int outType, double newFill,
                           double newScale, double newOffset, void* d_out, hipStream_t stream)
{
    const double a = oldScale / newScale, b = (oldOffset - newOffset) / newScale;  // Utils.h:453-454
    for_cdm_type(inType, [&](auto i) {
        for_cdm_type(outType, [&](auto o) { launch_scaled<decltype(i), decltype(o)>(d_in, n, oldFill, a, b, newFill, d_out, stream); });
    });
}

}  // namespace fimex_amd
