// What the vertical files share -- vertical.hip and vertical_plan.hip (interpolation; through
// vertical_search.hpp), vertical_levels.hip (the level converters, n6) and vertical_velocity.hip: the device-side form of
// fimex_amd_vertical_levels with the levels of one column, the upload of host coefficient arrays as kernel arguments into
// stream-ordered scratch, and the launch grid of a lane per column.  Everything has internal linkage: every file that includes
// it compiles its own copy of the upload kernel and the host helpers.  Column also compiles for the host (vertical_search.hpp).
#pragma once
#include "plan.hpp"

#include <algorithm>
#include <cstddef>
#include <type_traits>

namespace fimex_amd {

namespace {

constexpr int kUploadChunk = 128;  // doubles per upload launch (1 KiB of kernel arguments)

// device-side form of fimex_amd_vertical_levels: the coefficient arrays live in device memory
struct Levels {
    int kind;
    unsigned nz;
    const double* c0;  // axis | sigma | a | ap
    const double* c1;  // b
    double p0, ptop;
    const float* ps;     // [nt][plane]
    const float* field;  // [nt][nz][plane]
};

// the levels of one column: level(k) is what iVerticalValues[...] holds in the reference (double formula -> asFloat())
struct Column {
    const Levels& L;
    const float* fieldCol;  // FIELD: &field[t][0][cell]
    size_t plane;
    double ps, pDiff;
    __host__ __device__ Column(const Levels& L, size_t t, size_t cell, size_t plane) : L(L), fieldCol(nullptr), plane(plane), ps(0), pDiff(0)
    {
        if (L.kind == FIMEX_AMD_VLEVEL_FIELD) fieldCol = L.field + t * L.nz * plane + cell;
        else if (L.kind != FIMEX_AMD_VLEVEL_AXIS) {
            ps = (double)L.ps[t * plane + cell];
            pDiff = ps - L.ptop;  // vertical_coordinate_transformations.c:39
        }
    }
    __host__ __device__ float level(unsigned k) const
    {
        switch (L.kind) {
        case FIMEX_AMD_VLEVEL_FIELD: return fieldCol[(size_t)k * plane];
        case FIMEX_AMD_VLEVEL_AXIS: return (float)L.c0[k];
        case FIMEX_AMD_VLEVEL_SIGMA: return (float)(L.ptop + L.c0[k] * pDiff);          // :41
        case FIMEX_AMD_VLEVEL_HYBRID_SIGMA: return (float)((L.c0[k] * L.p0) + (L.c1[k] * ps));  // :60
        default: return (float)(L.c0[k] + (L.c1[k] * ps));                              // :68 (HYBRID_SIGMA_AP)
        }
    }
};

struct UploadChunk {
    double v[kUploadChunk];
};

// host doubles reach the device as kernel arguments: nothing waits for the stream and the caller's array is free on return
__global__ void __launch_bounds__(kUploadChunk) upload_kernel(double* __restrict__ dst, const UploadChunk chunk, unsigned n)
{
    if (threadIdx.x < n) dst[threadIdx.x] = chunk.v[threadIdx.x];
}

void upload(double* d_dst, const double* h_src, size_t n, hipStream_t stream)
{
    for (size_t off = 0; off < n; off += kUploadChunk) {
        UploadChunk c{};
        const size_t len = std::min<size_t>(kUploadChunk, n - off);
        for (size_t i = 0; i < len; ++i) c.v[i] = h_src[off + i];
        upload_kernel<<<1, kUploadChunk, 0, stream>>>(d_dst + off, c, (unsigned)len);
        FA_HIP(hipGetLastError());
    }
}

// stream-ordered scratch for the coefficient arrays of one call: freed on the stream, after the kernels that read it
class StreamScratch {
public:
    StreamScratch(size_t doubles, hipStream_t stream) : stream_(stream)
    {
        if (doubles) FA_HIP(hipMallocAsync(reinterpret_cast<void**>(&p_), doubles * sizeof(double), stream));
    }
    ~StreamScratch() { if (p_) (void)hipFreeAsync(p_, stream_); }
    StreamScratch(const StreamScratch&) = delete;
    StreamScratch& operator=(const StreamScratch&) = delete;
    double* take(size_t n) { double* r = p_ + used_; used_ += n; return r; }

private:
    double* p_ = nullptr;
    size_t used_ = 0;
    hipStream_t stream_;
};

size_t coefficient_count(const fimex_amd_vertical_levels& l)
{
    switch (l.kind) {
    case FIMEX_AMD_VLEVEL_FIELD: return 0;
    case FIMEX_AMD_VLEVEL_AXIS: case FIMEX_AMD_VLEVEL_SIGMA: return l.nz;
    default: return 2 * l.nz;
    }
}

Levels device_levels(const fimex_amd_vertical_levels& l, StreamScratch& scratch, hipStream_t stream)
{
    Levels d{};
    d.kind = l.kind;
    d.nz = (unsigned)l.nz;
    d.p0 = l.p0;
    d.ptop = l.ptop;
    d.ps = l.ps;
    d.field = l.field;
    const double* h0 = l.kind == FIMEX_AMD_VLEVEL_AXIS ? l.axis : l.kind == FIMEX_AMD_VLEVEL_SIGMA ? l.sigma
                     : l.kind == FIMEX_AMD_VLEVEL_HYBRID_SIGMA ? l.a : l.kind == FIMEX_AMD_VLEVEL_HYBRID_SIGMA_AP ? l.ap : nullptr;
    const bool two = l.kind == FIMEX_AMD_VLEVEL_HYBRID_SIGMA || l.kind == FIMEX_AMD_VLEVEL_HYBRID_SIGMA_AP;
    if (h0 && l.nz) {
        double* c0 = scratch.take(l.nz);
        upload(c0, h0, l.nz, stream);
        d.c0 = c0;
    }
    if (two && l.nz) {
        double* c1 = scratch.take(l.nz);
        upload(c1, l.b, l.nz, stream);
        d.c1 = c1;
    }
    return d;
}

// kind is a compile-time constant in the kernels that take it as a template argument: f(std::integral_constant<int, kind>)
template <class F>
void for_level_kind(int kind, F&& f)
{
    switch (kind) {
    case FIMEX_AMD_VLEVEL_FIELD: f(std::integral_constant<int, FIMEX_AMD_VLEVEL_FIELD>{}); break;
    case FIMEX_AMD_VLEVEL_AXIS: f(std::integral_constant<int, FIMEX_AMD_VLEVEL_AXIS>{}); break;
    case FIMEX_AMD_VLEVEL_SIGMA: f(std::integral_constant<int, FIMEX_AMD_VLEVEL_SIGMA>{}); break;
    case FIMEX_AMD_VLEVEL_HYBRID_SIGMA: f(std::integral_constant<int, FIMEX_AMD_VLEVEL_HYBRID_SIGMA>{}); break;
    default: f(std::integral_constant<int, FIMEX_AMD_VLEVEL_HYBRID_SIGMA_AP>{}); break;
    }
}

dim3 column_grid(size_t plane, size_t nt)
{
    FA_REQUIRE(nt <= 65535, "at most 65535 unlimited-dimension positions per call");
    FA_REQUIRE(ceil_div(plane, kBlock) <= 0x7fffffffu, "horizontal plane too large");
    return dim3((unsigned)ceil_div(plane, kBlock), (unsigned)nt, 1);
}

}  // namespace

}  // namespace fimex_amd
