// The shell of the second staged form's kernels (staged2.hip: float slices, staged2_typed.hip: stored 1- and 2-byte types,
// staged2_vector.hip, staged2_vector_typed.hip: pairs of vector components, regridded and rotated): which
// tile and z chunk a workgroup owns, the per-lane staging list, the ring of LDS slots that slice z + 1 .. z + DEPTH - 1 stream
// into by LDS-DMA while slice z is interpolated, and the choice of the loop copy.  The kernels keep what differs: element size,
// per-lane plan layout, stencil reads and conversions, result stores.
#pragma once

#include "staged2.hpp"
#include "staged_common.hpp"

#include "slice_list.hpp"  // (behind the HIP headers: its functions are host and device functions here)

#include <type_traits>

namespace fimex_amd {
namespace {

// workgroup -> tile and slices [z0, z1) of its z chunk; false: the workgroup has no tile
__device__ __forceinline__ bool decode_workgroup(const Staged2Args& a, StagedTile& T, uint32_t& z0, uint32_t& z1)
{
    uint32_t slot0 = blockIdx.x, zc = blockIdx.y;
    if (a.nZChunks != 0) flat_grid_workgroup(blockIdx.x, a.nZChunks, a.chunkPerXcd, slot0, zc);
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

// ---- which memory a slice of the launch is: the ring's policy

// The array form, the default: slice z of the launch is slice z of one source array and of one result array, base + z * bytes.
// No state and no code of its own.
struct ArraySlices {
    static constexpr bool kList = false;
};

// what a list launch (staged2_list.hip, staged2_list_typed.hip) knows of its variables, in the kernel arguments
struct SliceListArgs {
    SliceEnds e;
    uint64_t exactMask;  // bit k: variable k is computed in the reference's arithmetic (see SliceRing::exact_slice)
    const char* in[kSliceListMaxVars];
    char* out[kSliceListMaxVars];
};

// The list form: logical slice l of the launch is a level of one of up to kSliceListMaxVars variables, each an array of its own
// (slice_list.hpp).  The ring fetches slice z + DEPTH - 1 while slice z is interpolated and stored, so a workgroup holds two
// cursors: `src`, the next slice to fetch, runs ahead; `cur` is the slice in work -- its result, and its source for the loops that
// read memory directly.  Both are seeded at the chunk's z0 and moved one slice at a time: `src` by every fetch, `cur` by
// slice_done().  Scalar and wave-uniform, said explicitly as uniform() does for the pointers.
struct ListSlices {
    static constexpr bool kList = true;
    const SliceListArgs* list;
    mutable SliceCursor src, cur;  // (moved by the const ring's loop)

    __device__ __forceinline__ static void make_uniform(SliceCursor& c)
    {
        c.var = __builtin_amdgcn_readfirstlane(c.var);
        c.level = __builtin_amdgcn_readfirstlane(c.level);
        c.left = __builtin_amdgcn_readfirstlane(c.left);
    }
    __device__ __forceinline__ void seed(const SliceListArgs* l, uint32_t z0)
    {
        list = l;
        cur = slice_seek(l->e.ends, l->e.nvar, z0);
        make_uniform(cur);
        src = cur;
    }
    __device__ __forceinline__ static void step(const SliceListArgs* l, SliceCursor& c)
    {
        slice_advance(l->e.ends, l->e.nvar, c);
        make_uniform(c);
    }
    __device__ __forceinline__ const char* fetch(uint32_t inBytes) const
    {
        const char* p = uniform(list->in[src.var] + (size_t)src.level * inBytes);
        step(list, src);
        return p;
    }
    __device__ __forceinline__ const char* in_cur(uint32_t inBytes) const { return uniform(list->in[cur.var] + (size_t)cur.level * inBytes); }
    __device__ __forceinline__ char* out_cur(uint32_t outBytes) const
    {
        return const_cast<char*>(uniform(list->out[cur.var] + (size_t)cur.level * outBytes));
    }
};

// The slice ring of one workgroup of NT threads, in its dynamic LDS: DEPTH slots, each holds the largest tile of the plan, then 1 KiB that is never
// read.  Construction loads the lane's staging list and issues the DMAs of the first DEPTH - 1 slices, so it comes before
// everything else in a kernel: the per-output plan loads while they fly.
// Slices: where slice z lies.  Array form: in(z) / out(z).  List form: the ring asks for the slices of its chunk in order, each
// once -- source(z) moves the source cursor, and whoever walks the slices says slice_done() after each (run() does; the kernels'
// loops that do not go through the ring do it themselves); z only counts.
template <int NT, int KMAX, int DEPTH, class Slices = ArraySlices>
struct SliceRing : Slices {
    const char* inBase;
    char* outBase;
    uint32_t inBytes, outBytes;      // one source / result slice
    uint32_t inRecords, outRecords;  // the same as buffer sizes; tuning build: 0 switches the loads / stores off
    uint32_t z0, z1;
    uint32_t un;          // DMA instructions per lane and slice
    uint32_t gOff[KMAX];  // chunk c = threadIdx.x + j * NT of the tile's list: byte offset of its 16 bytes inside a source slice
    uint32_t slotChunks, slotFloats, waveChunk;
    const char* inBaseV = nullptr;  // pairs only (run_pairs): the second component's source

    // The ring of a component pair (staged2_vector.hip: float slices; staged2_vector_typed.hip: slices of elemBytes-byte elements,
    // both components in one type): [z0, z1) counts pairs, and the ring walks the 2 * (z1 - z0)
    // logical slices u(z0), v(z0), u(z0 + 1), ... -- logical slice l is slice z0 + l / 2 of `a.in` (l even) or of `inV` (l odd).
    __device__ __forceinline__ SliceRing(const Staged2Args& a, const StagedTile& T, uint32_t z0_, uint32_t z1_, const void* inV, uint32_t elemBytes)
        : inBase(reinterpret_cast<const char*>(a.in)), outBase(reinterpret_cast<char*>(a.out)), inBytes(a.inBytes),
          outBytes(a.nOut * elemBytes), inRecords((kTuningBuild && (a.flags & 1)) ? 0u : a.inBytes),
          outRecords((kTuningBuild && (a.flags & 2)) ? 0u : a.nOut * elemBytes), z0(z0_), z1(z1_), un((T.nChunks + NT - 1) / NT),
          slotChunks(a.slotChunks), slotFloats(a.slotChunks * 4u), waveChunk((threadIdx.x / kWave) * kWave),
          inBaseV(reinterpret_cast<const char*>(inV))
    {
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            const uint32_t c = threadIdx.x + j * NT;
            gOff[j] = (c < T.nChunks) ? a.chunkOff[T.chunkBase + c] * elemBytes : 0xFFFFFFFFu;
        }
        for (uint32_t l = 0; l + 1 < (uint32_t)DEPTH && l < 2 * (z1 - z0); ++l) {
            const rsrc_t rs = in_pair(l);
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
                if ((uint32_t)j < un) dma16(rs, dma_dst(l, j), gOff[j]);
        }
    }

    __device__ __forceinline__ SliceRing(const Staged2Args& a, const StagedTile& T, uint32_t z0_, uint32_t z1_, uint32_t elemBytes,
                                         const SliceListArgs* list = nullptr)
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
        if constexpr (Slices::kList) this->seed(list, z0);
        for (uint32_t i = 0; i + 1 < (uint32_t)DEPTH && i < z1 - z0; ++i) {
            const rsrc_t rs = source(z0 + i);
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
                if ((uint32_t)j < un) dma16(rs, dma_dst(i, j), gOff[j]);
        }
    }

    __device__ __forceinline__ rsrc_t in(uint32_t z) const
    {
        static_assert(!Slices::kList, "a list has no slice z of one array: source(z), in_uniform(z)");
        return make_rsrc(inBase + (size_t)z * inBytes, inRecords);
    }
    // the source of the next slice to fetch, z: every buffer resource is one slice, with the slice's own size
    __device__ __forceinline__ rsrc_t source(uint32_t z) const
    {
        if constexpr (Slices::kList) return make_rsrc(this->fetch(inBytes), inRecords);
        else return in(z);
    }
    __device__ __forceinline__ rsrc_t out(uint32_t z) const
    {
        if constexpr (Slices::kList) return make_rsrc(this->out_cur(outBytes), outRecords);
        else return make_rsrc(outBase + (size_t)z * outBytes, outRecords);
    }
    // the slice in work is finished, the next one follows
    __device__ __forceinline__ void slice_done() const
    {
        if constexpr (Slices::kList) Slices::step(this->list, this->cur);
    }
    // List form, FIMEX_AMD_BICUBIC_FAST plans: whether the slice in work is computed in the reference's arithmetic after all.  A
    // variable of fewer than STAGED_MIN_NZ slices, called on its own, runs the gather kernel, which knows no other arithmetic;
    // in a list it gets the same bytes.
    __device__ __forceinline__ bool exact_slice() const
    {
        if constexpr (Slices::kList) return ((this->list->exactMask >> this->cur.var) & 1u) != 0;
        else return false;
    }
    // list form: the variable of the slice in work (stored types: its fill value)
    __device__ __forceinline__ uint32_t variable() const
    {
        if constexpr (Slices::kList) return this->cur.var;
        else return 0u;
    }
    // logical slice l of a pair ring
    __device__ __forceinline__ rsrc_t in_pair(uint32_t l) const
    {
        return make_rsrc(((l & 1u) ? inBaseV : inBase) + (size_t)(z0 + l / 2u) * inBytes, inRecords);
    }
    // for the loops that do not go through the ring (gather tiles)
    __device__ __forceinline__ rsrc_t in_uniform(uint32_t z) const
    {
        if constexpr (Slices::kList) return make_rsrc(this->in_cur(inBytes), inRecords);
        else return make_rsrc(uniform(inBase + (size_t)z * inBytes), inRecords);
    }
    __device__ __forceinline__ rsrc_t out_uniform(uint32_t z) const
    {
        if constexpr (Slices::kList) return out(z);
        else return make_rsrc(uniform(outBase + (size_t)z * outBytes), outRecords);
    }

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
                const rsrc_t rs = source(z + DEPTH - 1);
#pragma unroll
                for (int j = 0; j < UN; ++j) dma16(rs, dma_dst(sl, j), gOff[j]);
            }
            sliceBody(z, reinterpret_cast<const char*>(smem + slot * slotFloats));
            slice_done();
            if (more) wait_vmcnt<(DEPTH - 2) * UN + (DEPTH - 1) * STORES>();
            else wait_vmcnt<STORES>();  // the tail of the z chunk: everything but this slice's stores
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            slot = (slot + 1 == (uint32_t)DEPTH) ? 0 : slot + 1;
        }
    }

    // s_waitcnt vmcnt(N) lgkmcnt(0): a u step keeps what it read from LDS in registers and stores nothing, so nothing else makes
    // sure that its LDS reads have returned before the barrier that releases the slot to the next DMA
    template <int N>
    __device__ __forceinline__ static void wait_vmcnt_and_lds()
    {
        static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
        __builtin_amdgcn_s_waitcnt((N & 0xF) | ((N >> 4) << 14) | (0x7 << 4));
        asm volatile("" ::: "memory");
    }

    // run() for a pair ring (see the pair constructor), one trip per pair with its u step and its v step written out, so that
    // every wait keeps an immediate.  uBody(slot) interpolates the u slice into registers and issues no memory instruction that
    // counts in vmcnt; vBody(z, slot) interpolates the v slice, rotates and issues exactly STORES store instructions (2 * PER in
    // the float kernel; 2 * NST on stored types, NST = 2 with pair stores and 4 without).  Logical slice l lies in
    // slot l % DEPTH.  With S(l) the stores of logical step l (0 on a u step, STORES on a v step), this was issued behind the DMA
    // of logical slice l + 1 when step l ends and may stay in flight, by run()'s own argument:
    //   DEPTH 2  that DMA is issued in step l itself, ahead of the step's stores: S(l), 0 after a u step, STORES after a v step;
    //   DEPTH 3  it is issued in step l - 1, then come S(l - 1), the DMA of slice l + 2 (UN instructions) and S(l); one of two
    //            consecutive steps is a v step: UN + STORES after either;
    //   tail     the steps that fetch nothing more (DEPTH 3: both steps of the last pair; DEPTH 2: its v step -- the u step still
    //            fetches the pair's own v slice) leave only their own stores outstanding, 0 and STORES.
    template <int UN, int STORES, class UBody, class VBody>
    __device__ __forceinline__ void run_pairs(UBody&& uBody, VBody&& vBody) const
    {
        static_assert(DEPTH == 2 || DEPTH == 3, "the slots of a pair's steps are written out for these depths");
        extern __shared__ __attribute__((aligned(16))) float smem[];
        auto fetch = [&](uint32_t l, uint32_t sl) __attribute__((always_inline)) {
            const rsrc_t rs = in_pair(l);
#pragma unroll
            for (int j = 0; j < UN; ++j) dma16(rs, dma_dst(sl, j), gOff[j]);
        };
        auto next = [](uint32_t sl) { return sl + 1 == (uint32_t)DEPTH ? 0u : sl + 1; };
        const uint32_t n = z1 - z0;
        uint32_t slotU = 0;
        for (uint32_t p = 0; p < n; ++p) {
            const bool more = p + 1 < n;
            const uint32_t slotV = next(slotU), slotN = next(slotV);  // DEPTH 2: slotN is slotU
            // u step, logical slice 2p
            if (DEPTH == 2) fetch(2 * p + 1, slotV);    // into the slot the v slice of pair p - 1 has left
            else if (more) fetch(2 * p + 2, slotN);
            uBody(reinterpret_cast<const char*>(smem + slotU * slotFloats));
            if (DEPTH == 3 && more) wait_vmcnt_and_lds<UN + STORES>();
            else wait_vmcnt_and_lds<0>();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            // v step, logical slice 2p + 1
            if (more) fetch(2 * p + DEPTH, slotU);  // into the slot the u slice has just left
            vBody(z0 + p, reinterpret_cast<const char*>(smem + slotV * slotFloats));
            if (more) wait_vmcnt<(DEPTH - 2) * UN + STORES>();
            else wait_vmcnt<STORES>();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            slotU = DEPTH == 2 ? slotU : slotN;
        }
    }
};

}  // namespace
}  // namespace fimex_amd
