// The shell of the second staged form's kernels (staged2.hip: float slices, staged2_typed.hip: stored 1- and 2-byte types): which
// tile and z chunk a workgroup owns, the per-lane staging list, the ring of LDS slots that slice z + 1 .. z + DEPTH - 1 stream
// into by LDS-DMA while slice z is interpolated, and the choice of the loop copy.  The kernels keep what differs: element size,
// per-lane plan layout, stencil reads and conversions, result stores.
#pragma once

#include "staged2.hpp"
#include "staged_common.hpp"

#include <type_traits>

namespace fimex_amd {
namespace {

// workgroup -> tile and slices [z0, z1) of its z chunk; false: the workgroup has no tile
__device__ __forceinline__ bool decode_workgroup(const Staged2Args& a, StagedTile& T, uint32_t& z0, uint32_t& z1)
{
    uint32_t slot0 = blockIdx.x, zc = blockIdx.y;
    if (a.nZChunks != 0) {  // workgroup s runs on XCD s % 8; the k-th workgroup of an XCD is z chunk k % n of the XCD's tile k / n
        const uint32_t k = blockIdx.x / kXcds;
        zc = k % a.nZChunks;
        slot0 = (k / a.nZChunks) * kXcds + blockIdx.x % kXcds;
    }
    const uint32_t tile = a.order[slot0];
    if (tile == 0xFFFFFFFFu) return false;
    T = a.tiles[tile];
    z0 = a.zStart[zc];
    z1 = a.zStart[zc + 1];
    return true;
}

// (slice pointers are wave-uniform; said explicitly, or the compiler loops over the lanes' descriptors)
__device__ __forceinline__ const char* uniform(const char* ptr)
{
    const uint64_t v = reinterpret_cast<uint64_t>(ptr);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<const char*>(((uint64_t)hi << 32) | lo);
}

// a where the mask is all ones, b where it is all zeros
__device__ __forceinline__ float pick(uint32_t mask, float a, float b)
{
    return __uint_as_float((__float_as_uint(a) & mask) | (__float_as_uint(b) & ~mask));
}

// One copy of the slice loop per number of DMA instructions a lane issues per slice (1 .. KMAX, chosen per tile: no instruction
// is issued for chunks a tile does not have and every wait keeps an immediate count) and per kind of wave:
// body(integral_constant<int, UN>, bool_constant<PLAIN>).  The plan never gives a tile more than KMAX * NT chunks.
template <int KMAX, int UN = 1, class Body>
__device__ __forceinline__ void dispatch_un(uint32_t un, bool plainWave, Body&& body)
{
    static_assert(KMAX <= 8, "one copy of the loop per DMA count");
    if (un == UN) {
        if (plainWave) body(std::integral_constant<int, UN>(), std::true_type());
        else body(std::integral_constant<int, UN>(), std::false_type());
    } else if constexpr (UN < KMAX) {
        dispatch_un<KMAX, UN + 1>(un, plainWave, body);
    }
}

// The slice ring of one workgroup of NT threads, in its dynamic LDS: DEPTH slots, each holds the largest tile of the plan, then 1 KiB that is never
// read.  Construction loads the lane's staging list and issues the DMAs of the first DEPTH - 1 slices, so it comes before
// everything else in a kernel: the per-output plan loads while they fly.
template <int NT, int KMAX, int DEPTH>
struct SliceRing {
    const char* inBase;
    char* outBase;
    uint32_t inBytes, outBytes;      // one source / result slice
    uint32_t inRecords, outRecords;  // the same as buffer sizes; tuning build: 0 switches the loads / stores off
    uint32_t z0, z1;
    uint32_t un;          // DMA instructions per lane and slice
    uint32_t gOff[KMAX];  // chunk c = threadIdx.x + j * NT of the tile's list: byte offset of its 16 bytes inside a source slice
    uint32_t slotChunks, slotFloats, waveChunk;

    __device__ __forceinline__ SliceRing(const Staged2Args& a, const StagedTile& T, uint32_t z0_, uint32_t z1_, uint32_t elemBytes)
        : inBase(reinterpret_cast<const char*>(a.in)), outBase(reinterpret_cast<char*>(a.out)), inBytes(a.inBytes),
          outBytes(a.nOut * elemBytes), inRecords((kTuningBuild && (a.flags & 1)) ? 0u : a.inBytes),
          outRecords((kTuningBuild && (a.flags & 2)) ? 0u : a.nOut * elemBytes), z0(z0_), z1(z1_), un((T.nChunks + NT - 1) / NT),
          slotChunks(a.slotChunks), slotFloats(a.slotChunks * 4u), waveChunk((threadIdx.x / kWave) * kWave)
    {
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            const uint32_t c = threadIdx.x + j * NT;
            gOff[j] = (c < T.nChunks) ? a.chunkOff[T.chunkBase + c] * elemBytes : 0xFFFFFFFFu;  // ~0u: dropped by the bounds check (zeros)
        }
        for (uint32_t i = 0; i + 1 < (uint32_t)DEPTH && i < z1 - z0; ++i) {
            const rsrc_t rs = in(z0 + i);
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
                if ((uint32_t)j < un) dma16(rs, dma_dst(i, j), gOff[j]);
        }
    }

    __device__ __forceinline__ rsrc_t in(uint32_t z) const { return make_rsrc(inBase + (size_t)z * inBytes, inRecords); }
    __device__ __forceinline__ rsrc_t out(uint32_t z) const { return make_rsrc(outBase + (size_t)z * outBytes, outRecords); }
    // for the loops that do not go through the ring (gather tiles)
    __device__ __forceinline__ rsrc_t in_uniform(uint32_t z) const { return make_rsrc(uniform(inBase + (size_t)z * inBytes), inRecords); }
    __device__ __forceinline__ rsrc_t out_uniform(uint32_t z) const { return make_rsrc(uniform(outBase + (size_t)z * outBytes), outRecords); }

    // A lane without a chunk carries an offset beyond the slice and the DMA writes ZEROS for it (scripts/calib/dma_oob.hip):
    // inside the slot that is unused space, but a slot is not a whole number of NT chunks, and the last wave instructions of a
    // full tile would run past its end into the next slot -- the slice being interpolated.  Such an instruction (whole: slots
    // are multiples of 64 chunks) is pointed at the spare KiB instead of being left out, so every wave issues the same number.
    __device__ __forceinline__ float* dma_dst(uint32_t sl, int j) const
    {
        extern __shared__ __attribute__((aligned(16))) float smem[];
        const uint32_t c = waveChunk + (uint32_t)j * NT;
        return c < slotChunks ? smem + sl * slotFloats + c * 4u : smem + DEPTH * slotFloats;
    }

    // the first DEPTH - 1 slices have arrived (a workgroup's first wait only; run() follows)
    __device__ __forceinline__ void wait_first() const
    {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }

    // The loop over the z chunk's slices with UN as a compile-time constant, so that every wait is an immediate: results come
    // back in issue order, and behind the DMA of slice i + 1 the DMAs of the slices i + 2 .. i + DEPTH - 1 and the stores of the
    // last DEPTH - 1 iterations may stay in flight.  sliceBody(z, slot) interpolates slice z out of the bytes at `slot` and
    // issues exactly STORES store instructions (and no other memory instruction that counts in vmcnt).
    template <int UN, int STORES, class SliceBody>
    __device__ __forceinline__ void run(SliceBody&& sliceBody) const
    {
        extern __shared__ __attribute__((aligned(16))) float smem[];
        const uint32_t nzl = z1 - z0;
        uint32_t slot = 0;
        for (uint32_t i = 0; i < nzl; ++i) {
            const uint32_t z = z0 + i;
            const bool more = i + DEPTH - 1 < nzl;
            if (more) {  // into the slot slice i - 1 has left
                const uint32_t sl = (slot + DEPTH - 1 >= (uint32_t)DEPTH) ? slot - 1 : slot + DEPTH - 1;
                const rsrc_t rs = in(z + DEPTH - 1);
#pragma unroll
                for (int j = 0; j < UN; ++j) dma16(rs, dma_dst(sl, j), gOff[j]);
            }
            sliceBody(z, reinterpret_cast<const char*>(smem + slot * slotFloats));
            if (more) wait_vmcnt<(DEPTH - 2) * UN + (DEPTH - 1) * STORES>();
            else wait_vmcnt<STORES>();  // the tail of the z chunk: everything but this slice's stores
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            slot = (slot + 1 == (uint32_t)DEPTH) ? 0 : slot + 1;
        }
    }
};

}  // namespace
}  // namespace fimex_amd
