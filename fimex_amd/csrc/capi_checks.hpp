// Argument checks shared by the capi_*.hip files: buffers that must not overlap.  They compare addresses, so they always run on
// the caller's own pointers, host or device.
#pragma once

#include "common.hpp"

#include <initializer_list>
#include <string>

#pragma GCC visibility push(hidden)  // inline code of the capi_*.hip files
namespace fimex_amd {

struct Span {
    const void* p;
    size_t bytes;
    const char* name;
};

// the output buffer against every buffer the call reads
inline void require_no_overlap(const void* out, size_t outBytes, std::initializer_list<Span> inputs)
{
    const char* o0 = static_cast<const char*>(out);
    for (const Span& s : inputs) {
        if (!s.p || !s.bytes) continue;
        const char* i0 = static_cast<const char*>(s.p);
        FA_REQUIRE(o0 + outBytes <= i0 || i0 + s.bytes <= o0, std::string("the output buffer overlaps ") + s.name);
    }
}

// the 2-D / 3-D members of a level description as inputs of require_no_overlap
inline void require_no_overlap_with_levels(const void* out, size_t outBytes, const fimex_amd_vertical_levels& l, size_t cells)
{
    const bool field = l.kind == FIMEX_AMD_VLEVEL_FIELD, ps = !field && l.kind != FIMEX_AMD_VLEVEL_AXIS;
    require_no_overlap(out, outBytes, {{field ? l.field : nullptr, cells * l.nz * sizeof(float), "the level field"},
                                       {ps ? l.ps : nullptr, cells * sizeof(float), "ps"}});
}

// out may be one of the two inputs itself (every cell is read before it is written), but must not overlap either otherwise
inline void require_same_or_apart(const float* out, const float* in, size_t n, const char* name)
{
    if (out != in) require_no_overlap(out, n * sizeof(float), {{in, n * sizeof(float), name}});
}

}  // namespace fimex_amd
#pragma GCC visibility pop
