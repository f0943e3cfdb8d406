// accumulate / deAccumulate of CDMProcessor::getDataSlice (src/CDMProcessor.cc:470-491, :534-578) over a batch of nt positions of the
// unlimited dimension starting at firstPos.  The input is read as Data::asDouble(): a static_cast per element, no fill
// value handling, as in the reference.
//
// One lane per cell walks t, so every sum has the reference's operands in the reference's order and the result is bit for bit; the
// loads of a cell do not depend on its sums, so the levels of the unrolled loop are in flight together.  Consecutive lanes own
// adjacent cells: every load and store is coalesced.  The grid is capped and strides.
#include "plan.hpp"

#include <algorithm>

namespace fimex_amd {

namespace {

// replaceNanWith0 (:470-473): applied to position 0 only, and only where it is the addend / subtrahend
__device__ __forceinline__ double nan0(double v) { return v != v ? 0.0 : v; }

// acc[0] = in[0]; acc[1] = in[1] + nan0(in[0]); acc[t] = in[t] + acc[t-1]: what a writer pulling positions 0, 1, 2, ... gets from
// the slice cache of :537-557
template <typename T>
__global__ void __launch_bounds__(kBlock) accumulate_kernel(const T* __restrict__ in, size_t n, size_t nt, size_t firstPos,
                                                            const double* __restrict__ prev, double* __restrict__ out)
{
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        size_t t = 0;
        double acc;
        if (firstPos == 0) {
            acc = (double)in[i];
            out[i] = acc;  // not accumulated, its NaN kept
            acc = nan0(acc);
            t = 1;
        } else {
            acc = firstPos == 1 ? nan0(prev[i]) : prev[i];
        }
#pragma unroll 4
        for (; t < nt; ++t) {
            acc = (double)in[t * n + i] + acc;  // std::plus(d, dp), :486
            out[t * n + i] = acc;
        }
    }
}

// out[0] = in[0]; out[t] = in[t] - in[t-1], nan0 on in[0] as the subtrahend (:561-578)
template <typename T>
__global__ void __launch_bounds__(kBlock) deaccumulate_kernel(const T* __restrict__ in, size_t n, size_t nt, size_t firstPos,
                                                              const T* __restrict__ prev, double* __restrict__ out)
{
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        size_t t = 0;
        double before;
        if (firstPos == 0) {
            before = (double)in[i];
            out[i] = before;
            before = nan0(before);
            t = 1;
        } else {
            before = firstPos == 1 ? nan0((double)prev[i]) : (double)prev[i];
        }
#pragma unroll 4
        for (; t < nt; ++t) {
            const double cur = (double)in[t * n + i];
            out[t * n + i] = cur - before;  // std::minus(d, dp), :574
            before = cur;
        }
    }
}

unsigned cell_blocks(size_t n)
{
    const size_t want = ceil_div(n, kBlock), cap = std::max(1, tuning("ACCUMULATE_MAX_BLOCKS", 256 * 8));
    return (unsigned)(want < cap ? want : cap);
}

}  // namespace

// every argument has been checked (capi_derived.hip); n > 0 and nt > 0
void launch_accumulate(const void* d_in, int cdmType, size_t n, size_t nt, size_t firstPos, const double* d_prev, double* d_out, hipStream_t stream)
{
    for_cdm_type(cdmType, [&](auto v) {
        using T = decltype(v);
        accumulate_kernel<T><<<cell_blocks(n), kBlock, 0, stream>>>(static_cast<const T*>(d_in), n, nt, firstPos, d_prev, d_out);
    });
    FA_HIP(hipGetLastError());
}

void launch_deaccumulate(const void* d_in, int cdmType, size_t n, size_t nt, size_t firstPos, const void* d_prev, double* d_out,
                         hipStream_t stream)
{
    for_cdm_type(cdmType, [&](auto v) {
        using T = decltype(v);
        deaccumulate_kernel<T><<<cell_blocks(n), kBlock, 0, stream>>>(static_cast<const T*>(d_in), n, nt, firstPos, static_cast<const T*>(d_prev),
                                                                      d_out);
    });
    FA_HIP(hipGetLastError());
}

}  // namespace fimex_amd
