// Forward-mapping regrid, plan creation: the reference's scatter (src/CachedForwardInterpolation.cc:38-131 push_back()s every source
// value into a std::vector per target cell) is inverted once into a CSR list of source cells per target cell, kept in source scan
// order, so that the apply kernels (forward.hip, forward_median.hip, forward_tiled.hip) gather without atomics or allocation and
// add in exactly the reference's order.
#include <cstring>  // before rocprim: its texture iterator calls memset

#include "forward_math.hpp"

#include <rocprim/rocprim.hpp>

namespace fimex_amd {

namespace {

// target cell of every source cell (forward_math.hpp: forward_target)
__global__ void __launch_bounds__(kBlock) forward_targets(const double* __restrict__ px, const double* __restrict__ py,
                                                          uint32_t nIn, int64_t outX, int64_t outY, uint32_t* __restrict__ tgt)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nIn) return;
    tgt[i] = forward_target(px[i], py[i], outX, outY);
}

__global__ void __launch_bounds__(kBlock) iota_kernel(uint32_t* __restrict__ idx, uint32_t n)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) idx[i] = i;
}

// offsets[t] = first position in the sorted keys that is >= t (t = 0 .. nOut): lower bound by binary search
__global__ void __launch_bounds__(kBlock) csr_offsets_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t nOut, uint32_t* __restrict__ offsets)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t > nOut) return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    offsets[t] = lo;
}

__global__ void __launch_bounds__(kBlock) csr_stats_kernel(const uint32_t* __restrict__ offsets, uint32_t nOut, unsigned long long* __restrict__ stats)
{
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    uint32_t len = 0;
    bool empty = false;
    if (t < nOut) {
        len = offsets[t + 1] - offsets[t];
        empty = len == 0;
        if (t == nOut - 1) stats[0] = offsets[nOut];  // mapped source cells
    }
    const unsigned long long e = __popcll(__ballot(empty));
    uint32_t m = len;
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (e) atomicAdd(&stats[2], e);
        if (m) atomicMax(&stats[1], (unsigned long long)m);
    }
}

}  // namespace

void build_forward_plan(fimex_amd_regrid_plan& plan, const double* d_px, const double* d_py, hipStream_t stream)
{
    const size_t nIn = plan.inX * plan.inY, nOut = plan.outX * plan.outY;
    FA_REQUIRE(nIn > 0 && nIn <= kMaxSliceCells, "input grid must have between 1 and 2^30-1 cells per slice");
    FA_REQUIRE(nOut > 0 && nOut <= 0x7FFFFFFFu, "output grid must have between 1 and 2^31-1 cells");
    DeviceArray<uint32_t> d_tgt(nIn);
    forward_targets<<<dim3((uint32_t)ceil_div(nIn, kBlock)), kBlock, 0, stream>>>(
        d_px, d_py, (uint32_t)nIn, (int64_t)plan.outX, (int64_t)plan.outY, d_tgt.get());
    FA_HIP(hipGetLastError());
    // CSR by a stable radix sort of (target, source index): buckets keep the source scan order, which is the
    // reference's push_back order (src/CachedForwardInterpolation.cc:103-112); unmapped cells (key ~0) sort to the end
    DeviceArray<uint32_t> d_idx(nIn), d_keysSorted(nIn), d_idxSorted(nIn);
    iota_kernel<<<dim3((uint32_t)ceil_div(nIn, kBlock)), kBlock, 0, stream>>>(d_idx.get(), (uint32_t)nIn);
    FA_HIP(hipGetLastError());
    size_t tmpBytes = 0;
    FA_HIP(rocprim::radix_sort_pairs(nullptr, tmpBytes, d_tgt.get(), d_keysSorted.get(), d_idx.get(), d_idxSorted.get(), nIn, 0, 32, stream));
    DeviceArray<unsigned char> tmp(tmpBytes ? tmpBytes : 1);
    FA_HIP(rocprim::radix_sort_pairs(tmp.get(), tmpBytes, d_tgt.get(), d_keysSorted.get(), d_idx.get(), d_idxSorted.get(), nIn, 0, 32, stream));
    plan.offsets.allocate(nOut + 1);
    DeviceArray<unsigned long long> d_stats(3);  // mapped, maxBucket, empty
    FA_HIP(hipMemsetAsync(d_stats.get(), 0, 3 * sizeof(unsigned long long), stream));
    csr_offsets_kernel<<<dim3((uint32_t)ceil_div(nOut + 1, kBlock)), kBlock, 0, stream>>>(d_keysSorted.get(), (uint32_t)nIn, (uint32_t)nOut,
                                                                                          plan.offsets.get());
    FA_HIP(hipGetLastError());
    csr_stats_kernel<<<dim3((uint32_t)ceil_div(nOut, kBlock)), kBlock, 0, stream>>>(plan.offsets.get(), (uint32_t)nOut, d_stats.get());
    FA_HIP(hipGetLastError());
    unsigned long long h_stats[3] = {0, 0, 0};
    FA_HIP(hipMemcpyAsync(h_stats, d_stats.get(), sizeof(h_stats), hipMemcpyDeviceToHost, stream));
    FA_HIP(hipStreamSynchronize(stream));
    const size_t mapped = (size_t)h_stats[0], maxBucket = (size_t)h_stats[1], empty = (size_t)h_stats[2];
    plan.src.allocate(mapped ? mapped : 1);
    if (mapped) FA_HIP(hipMemcpyAsync(plan.src.get(), d_idxSorted.get(), mapped * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    FA_HIP(hipStreamSynchronize(stream));  // temporaries are released on return
    plan.info.planBytes = (nOut + 1) * sizeof(uint32_t) + mapped * sizeof(uint32_t);
    plan.info.undefinedCells = empty;
    plan.info.maxBucket = maxBucket;
    plan.info.mappedSourceCells = mapped;
    build_forward_tiles(plan, stream);  // dense mappings: the LDS-staged form (forward_tiled.hip)
}

}  // namespace fimex_amd
