// What the float kernels of the second LDS-staged regrid form share beside their text (staged2_apply_kernel.hpp): staged2.hip
// (slices of one array) and staged2_list.hip (slices of a list of variables).
#pragma once

#include "staged2_ring.hpp"

namespace fimex_amd {
namespace {

// Result stores of the slice loop: non-temporal and written through (sc1 nt): 0.4-1 % faster than nt alone in six placements of the
// output out of six (profiles/calib/r02_store_policy.jsonl), plain stores 2-6 % slower.  Tuning build: flags 8 plain, 16 nt, 32 sc0 nt.
__device__ __forceinline__ void store_result(uint32_t bits, rsrc_t ro, uint32_t off, uint32_t flags)
{
    if (kTuningBuild && (flags & 56u)) {
        if (flags & 8u) __builtin_amdgcn_raw_buffer_store_b32(bits, ro, off, 0, 0);
        else if (flags & 16u) __builtin_amdgcn_raw_buffer_store_b32(bits, ro, off, 0, 2);
        else __builtin_amdgcn_raw_buffer_store_b32(bits, ro, off, 0, 3);
        return;
    }
    __builtin_amdgcn_raw_buffer_store_b32(bits, ro, off, 0, 18);
}

// the store policy of a float launch into the kernels' flags: STAGE2_STORE 1 plain, 2 nt, 4 sc0 nt (default: sc1 nt)
inline void set_store_policy(Staged2Args& a) { a.flags |= (uint32_t)tuning("STAGE2_STORE", 0) << 3; }

}  // namespace
}  // namespace fimex_amd
