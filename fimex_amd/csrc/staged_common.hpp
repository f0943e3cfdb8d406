// Device helpers shared by the LDS-staged regrid kernels (staged.hip: one 256-thread workgroup per uniform tile;
// staged2*.hip: larger workgroups, tiles of varying width, slice ring of varying depth, see staged2_ring.hpp).
#pragma once

#include "plan.hpp"
#include "stencil_math.hpp"

namespace fimex_amd {
namespace {

constexpr int kMaxRows = 160;  // source rows one tile may span

// The source cells a tile of output cells needs, for one workgroup of kBlock threads that holds it in LDS (__shared__): per
// source row one segment of 16-byte chunks, and the place of every segment in the tile's LDS image.  Both staged forms build
// their plans on it (build_tiles in staged.hip, tile_scan in staged2_plan.hip); each keeps its tile geometry -- `cells(f)` calls
// f(cell, need) for every cell of the tile the calling thread owns -- and what it writes out.  Every thread of the workgroup
// calls scan() and segments(); a tile that does not fit ends there.
struct TileFootprint {
    int rmin, rmax, fail;
    int rowMin[kMaxRows], rowMax[kMaxRows];  // per source row rmin + i: first and last column needed; after segments(): rowMin = the segment's first column
    uint32_t rowChunk[kMaxRows + 1];         // first chunk of row i's segment in the tile's image; [nr] = all chunks

    // the rows and per row the columns that the tile's cells read; returns the number of rows, -1: more than kMaxRows
    template <class Cells>
    __device__ int scan(Cells&& cells)
    {
        if (threadIdx.x == 0) { rmin = 0x7FFFFFFF; rmax = -1; fail = 0; }
        __syncthreads();
        cells([&](size_t, const CellNeed& c) {
            if (c.valid) { atomicMin(&rmin, (int)c.ya); atomicMax(&rmax, (int)c.yb); }
        });
        __syncthreads();
        const int r0 = rmin;
        const int nr = (rmax >= r0) ? rmax - r0 + 1 : 0;
        if (nr > kMaxRows) return -1;
        for (int i = threadIdx.x; i < nr; i += kBlock) { rowMin[i] = 0x7FFFFFFF; rowMax[i] = -0x7FFFFFFF; }
        __syncthreads();
        cells([&](size_t, const CellNeed& c) {
            if (c.valid)
                for (int64_t r = c.ya; r <= c.yb; ++r) {
                    atomicMin(&rowMin[r - r0], (int)c.xa);
                    atomicMax(&rowMax[r - r0], (int)c.xb);
                }
        });
        __syncthreads();
        return nr;
    }

    __device__ bool has_row(int i) const { return rowMax[i] >= rowMin[i]; }  // some cell of the tile reads source row rmin + i

    // Segments of chunks of cpc source cells (16 bytes) in a slice of ix x iy, and their prefix sum.  false: more than capChunks.
    __device__ bool segments(int nr, int64_t ix, int64_t iy, uint32_t cpc, uint32_t capChunks)
    {
        if (threadIdx.x == 0) {
            const int64_t layer = ix * iy;
            uint32_t acc = 0;
            for (int i = 0; i < nr; ++i) {
                rowChunk[i] = acc;
                if (has_row(i)) {
                    // the segment starts on a 16-byte boundary of the SLICE (the DMA moves 16 bytes per lane; aligned pieces stay
                    // inside one line): it may begin up to cpc - 1 cells before the first cell needed, in the row above for x < 0
                    const int64_t first = (int64_t)(rmin + i) * ix + rowMin[i];
                    int64_t start = first & ~(int64_t)(cpc - 1);
                    const uint32_t nch = (uint32_t)((first - start + (rowMax[i] - rowMin[i])) / cpc + 1);
                    // a last chunk that would cross the end of the slice is moved back instead (unaligned, still whole; slices of
                    // stored types hold a multiple of 4 bytes, so the chunk still starts on a 4-byte boundary)
                    if (start + cpc * (int64_t)nch > layer) start = layer - cpc * (int64_t)nch;
                    if (start < 0) fail = 1;
                    rowMin[i] = (int)(start - (int64_t)(rmin + i) * ix);  // column of the segment's first cell, may be negative
                    acc += nch;
                }
            }
            rowChunk[nr] = acc;
            if (acc > capChunks) fail = 1;
        }
        __syncthreads();
        return fail == 0;
    }

    // global cell offset of the first cell of row i's segment
    __device__ int64_t segment_start(int i, int64_t ix) const { return (int64_t)(rmin + i) * ix + rowMin[i]; }

    // the plan entry of one cell: LDS offsets (16 bits each, in elements) of its stencil rows 0 | 1 << 16 and 2 | 3 << 16
    __device__ void offsets(const CellNeed& c, uint32_t cpc, uint32_t& a, uint32_t& b) const
    {
        a = b = kInvalidPos;
        if (!c.valid) return;
        uint32_t off[4];
        for (int r = 0; r < 4; ++r) {
            const int64_t row = (c.ya + r <= c.yb) ? c.ya + r : c.yb;  // missing rows repeat the last one
            const int i = (int)(row - rmin);
            off[r] = rowChunk[i] * cpc + (uint32_t)(c.xa - rowMin[i]);
        }
        a = off[0] | (off[1] << 16);
        b = off[2] | (off[3] << 16);
    }
};

// One LDS-DMA wave instruction: 64 lanes x 16 bytes from per-lane buffer offsets to ldsBase + lane * 16.
// (The builtin exists only in the device pass; the host pass of hipcc parses kernel bodies too.)
__device__ __forceinline__ void dma16(rsrc_t rs, float* ldsBase, uint32_t voff, uint32_t aux = 0)
{
#if defined(__HIP_DEVICE_COMPILE__)
    using lds_ptr = __attribute__((address_space(3))) void*;
    switch (aux) {  // cache policy, wave-uniform (tuning knob LOAD_AUX; the default policy measured best)
    case 1: __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)ldsBase, 16, voff, 0, 0, 1); break;
    case 16: __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)ldsBase, 16, voff, 0, 0, 16); break;
    case 17: __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)ldsBase, 16, voff, 0, 0, 17); break;
    case 2: __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)ldsBase, 16, voff, 0, 0, 2); break;
    default: __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)ldsBase, 16, voff, 0, 0, 0); break;
    }
#else
    (void)rs; (void)ldsBase; (void)voff; (void)aux;
#endif
}

// s_waitcnt on vmcnt only (gfx9 encoding: vmcnt in bits 3:0 and 15:14, expcnt 6:4 and lgkmcnt 11:8 left at "no wait")
template <int N>
__device__ __forceinline__ void wait_vmcnt()
{
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    __builtin_amdgcn_s_waitcnt((N & 0xF) | ((N >> 4) << 14) | (0x7 << 4) | (0xF << 8));
    asm volatile("" ::: "memory");
}

}  // namespace
}  // namespace fimex_amd
