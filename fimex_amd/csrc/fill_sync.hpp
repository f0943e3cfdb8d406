// How the waves and workgroups of the systolic fill kernels (fill.hip, creepfill.hip) wait for each other: LDS flags, lane
// moves, the words of several workgroups per slice, bounded waits, the hand-off between bands.
#pragma once

#include "common.hpp"

namespace fimex_amd {

namespace {

// Flags of the LDS hand-off.  The LDS executes one wave's operations in issue order and is coherent within the CU, so a
// flag written after the data (and read before it) needs no fence -- and must not get one: a release / acquire at
// workgroup scope makes the compiler wait for ALL outstanding vector-memory operations (s_waitcnt vmcnt(0)), i.e. for the
// chunk prefetch that was issued a moment ago, once per event.  Compiler barriers keep the program order.
__device__ __forceinline__ void lds_publish(unsigned int* flag, unsigned int value)
{
    asm volatile("" ::: "memory");
    __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ unsigned int lds_observe(const unsigned int* flag)
{
    asm volatile("" ::: "memory");
    const unsigned int v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    asm volatile("" ::: "memory");
    return v;
}

// value of lane l-1 (lane 0 keeps its own): one DPP move, "wave_shr:1" (0x138), no LDS round trip
__device__ __forceinline__ float lane_from_above(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
// the same with lane 0 (which has no lane above) receiving `first`: the DPP move leaves lanes without a source at the
// old value of the destination, so the separate select for lane 0 is not needed
__device__ __forceinline__ float lane_from_above_or(float v, float first)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(first), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
// value held by lane `idx` (wave-uniform index) broadcast through an SGPR
__device__ __forceinline__ float lane_value(float v, int idx)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), idx));
}

// ---- several workgroups per slice (small batches): the bands of one slice are dealt to G workgroups, W = waves per workgroup
// at a time (bands 0 .. W-1 to workgroup 0, W .. 2W-1 to workgroup 1, ...), so that a batch of 16 slices uses 96 CUs instead of
// 16.  Inside a workgroup nothing changes; the hand-off of every W-th band boundary, which already went through global memory,
// now crosses workgroups: the producer's stores of that band are write-through (sc0 sc1), it publishes its progress in a
// global word after s_waitcnt vmcnt(0) (relaxed agent-scope store = sc1), the consumer polls that word and reads the row
// above with sc0 sc1 loads (MI355X_MICROARCH.md, inter-workgroup visibility: every store and every load of the handed-off
// bytes bypasses the non-coherent caches).  The sweeps of the workgroups of a slice are separated by a barrier on a global
// counter with agent-scope release / acquire, which makes everything else (the row below a band, the border columns) visible.
// Every wait is bounded: a spin that exceeds its cap sets the launch's error word, every other wait then falls through, the
// kernel ends and the host call fails with a message -- a wrong counter cannot hang the GPU.
struct MultiWg {
    uint32_t g, G;            // this workgroup and the number of workgroups of its slice (1: the single-workgroup kernels)
    uint32_t experiment = 0;  // tuning build: 1 = the producer does not wait for its stores (timing experiment, results invalid)
    unsigned int* flags;      // [bands] progress of the bands whose hand-off crosses workgroups: columns final + 1
    unsigned int* error;      // one word per launch
    unsigned long long* prof = nullptr;  // tuning build, experiment 4: cycles summed over bands: [0] events, [1] steps, [2] bands
};
// A wait gives up after kSpinCapTicks of WALL time (s_memrealtime, the 100 MHz constant clock): long enough that workgroups
// kept off their CUs by other work on the device -- a concurrent one-workgroup-per-slice fill of a long batch, another process --
// still arrive (they are queued behind that work, not lost), short enough that a wrong counter ends the call instead of hanging
// the GPU.  The clock is read only every 4096th (256th) poll, for the first time after that many polls: a wait that ends
// quickly never reads it.
constexpr unsigned long long kSpinCapTicks = 30ull * 100000000ull;  // 30 s
__device__ __forceinline__ bool spin_expired(unsigned long long& t0)
{
    const unsigned long long now = __builtin_amdgcn_s_memrealtime();
    if (t0 == 0) { t0 = now | 1ull; return false; }
    return now - t0 > kSpinCapTicks;
}

__device__ __forceinline__ bool launch_failed(const unsigned int* error)
{
    return __hip_atomic_load(error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}
__device__ __forceinline__ void fail_launch(unsigned int* error, unsigned int code)
{
    __hip_atomic_store(error, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// waits until the LDS word reaches `need`; false: gave up (cap or another wave's failure)
__device__ __forceinline__ bool wait_lds_at_least(const unsigned int* flag, unsigned int need, unsigned int* error)
{
    unsigned long long t0 = 0;
    for (unsigned int it = 0;; ++it) {
        asm volatile("" ::: "memory");
        if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= need) { asm volatile("" ::: "memory"); return true; }
        __builtin_amdgcn_s_sleep(1);
        if ((it & 0xFFF) == 0xFFF && (spin_expired(t0) || launch_failed(error))) { fail_launch(error, 1); return false; }
    }
}
__device__ __forceinline__ bool wait_global_at_least(const unsigned int* flag, unsigned int need, unsigned int* error)
{
    unsigned long long t0 = 0;
    for (unsigned int it = 0;; ++it) {
        if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need) { asm volatile("" ::: "memory"); return true; }
        __builtin_amdgcn_s_sleep(2);
        if ((it & 0xFF) == 0xFF && (spin_expired(t0) || launch_failed(error))) { fail_launch(error, 2); return false; }
    }
}
// barrier of the G workgroups of one slice on a monotone global counter (instance k waits for k * G arrivals)
__device__ __forceinline__ void slice_barrier(unsigned int* counter, unsigned int target, unsigned int* error)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        wait_global_at_least(counter, target, error);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
}

constexpr int kHandW = 192;  // columns of a band's last row kept in LDS for the band below

// LDS hand-off between consecutive bands: the wave of band b publishes its last row's new values in
// hand[b % 16][(b / 16) & 1][x % 192] and a counter "band, columns finished"; the wave of band b + 1 reads them 64
// columns at a time and publishes how far it has read, which bounds how far the producer may run ahead.
struct Handoff {
    float* data;             // [16][2][kHandW]
    unsigned int* produced;  // [16][2]  (band + 1) << 19 | columns of the last row that are final
    unsigned int* consumed;  // [16][2]  (band + 1) << 19 | columns the band below has taken over
};
__device__ __forceinline__ unsigned int hand_tag(uint32_t band, uint32_t cols) { return ((band + 1) << 19) | cols; }

}  // namespace

}  // namespace fimex_amd
