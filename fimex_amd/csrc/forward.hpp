// What the forward apply kernels of forward.hip and forward_median.hip share: their arguments and the start of a wave-per-target
// kernel.  The aggregation rules themselves are forward_math.hpp's.
#pragma once

#include "forward_math.hpp"

namespace fimex_amd {

struct FwdArgs {
    const float* in;
    float* out;
    const uint32_t* offsets;
    const uint32_t* src;
    uint32_t nOut;
    size_t inLayer;
    uint32_t nz;
    uint32_t zPerBlock;
    uint32_t rankAll;  // tuning build (FWD_MEDIAN_SHORT=0): the median of every bucket by rank counting
};

// one wave per target cell, 4 targets per workgroup: the wave's lane, target, slices z0 .. z1 and bucket (b, len)
struct WaveTarget {
    uint32_t lane, t, z0, z1, b, len;
};
// false: nothing is left to do -- no such target, or an empty bucket, whose slices are undefined (stored here)
__device__ __forceinline__ bool wave_target(const FwdArgs& a, WaveTarget& w)
{
    w.lane = threadIdx.x & (kWave - 1);
    w.t = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (w.t >= a.nOut) return false;  // wave-uniform
    w.z0 = blockIdx.y * a.zPerBlock;
    w.z1 = min(a.nz, w.z0 + a.zPerBlock);
    w.b = a.offsets[w.t];
    w.len = a.offsets[w.t + 1] - w.b;
    if (w.len != 0) return true;
    if (w.lane == 0)
        for (uint32_t z = w.z0; z < w.z1; ++z) a.out[(size_t)z * a.nOut + w.t] = undefined_f();
    return false;
}
// forward_median.hip: the median of medium buckets, one wave per target cell
void launch_forward_median_wave(const FwdArgs& a, size_t maxBucket, bool undef, uint32_t chunks, hipStream_t stream);

inline dim3 wave_grid(const FwdArgs& a, uint32_t chunks) { return dim3((uint32_t)ceil_div(a.nOut, kBlock / kWave), chunks, 1); }

}  // namespace fimex_amd
