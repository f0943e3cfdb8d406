// Device helpers shared by the LDS-staged regrid kernels (staged.hip: one 256-thread workgroup per uniform tile;
// staged2*.hip: larger workgroups, tiles of varying width, slice ring of varying depth, see staged2_ring.hpp).
#pragma once

#include "plan.hpp"
#include "stencil_math.hpp"

namespace fimex_amd {
namespace {

constexpr int kMaxRows = 160;  // source rows one tile may span

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
