// Extraction: what extract.hip, projection.hip and capi_extract.hip share.
#pragma once

#include "plan.hpp"

#include <vector>

namespace fimex_amd {

constexpr int kExtractMaxSlow = FIMEX_AMD_EXTRACT_MAX_DIMS - 1;

// A reduction after normalisation (extract.hip), on the host: rows of `width` elements of the merged fastest dimension, cut into
// runs that are contiguous in the source, and per slower dimension the source offset of every output index.  Offsets count elements.
struct ExtractTables {
    fimex_amd_extract_info info{};
    uint64_t base = 0;                       // the dimensions of output length 1
    uint64_t width = 0;                      // output elements per row
    std::vector<uint64_t> runOut, runSrc;    // run k: output columns [runOut[k], runOut[k + 1]), source offset runSrc[k]
    std::vector<std::vector<uint64_t>> slow;  // fastest first
};

// the kernel's view of the same, tables in device memory
struct ExtractArgs {
    uint64_t base, width, n;  // n: output elements
    uint32_t nSlow, nRuns;
    uint64_t run0;  // runSrc[0]: all a row of one run needs
    const uint64_t* runOut;
    const uint64_t* runSrc;
    uint64_t size[kExtractMaxSlow];
    const uint64_t* off[kExtractMaxSlow];
};

// checks the description (throws with the message of the refusal) and normalises it; touches no device
ExtractTables extract_normalise(const fimex_amd_extract_dim* dims, size_t nDims);
void build_extract_plan(fimex_amd_extract_plan& plan, const ExtractTables& tables);  // uploads to the current device
// the pointers are aligned to elem and the plan holds at least one output element
void launch_extract(const fimex_amd_extract_plan& plan, const void* d_in, size_t elem, void* d_out, hipStream_t stream);

// projection.hip: flags of the mesh columns and rows with a point inside the box; xKeep[nx], yKeep[ny] on the host.  Synchronises.
void run_bounding_box(const char* projIn, const char* projLonLat, const double* h_xAxis, size_t nx, const double* h_yAxis, size_t ny,
                      bool axesInDegree, double south, double north, double west, double east, unsigned char* h_xKeep, unsigned char* h_yKeep,
                      hipStream_t stream);

}  // namespace fimex_amd

struct fimex_amd_extract_plan {
    int device = 0;
    fimex_amd_extract_info info{};
    fimex_amd::ExtractArgs args{};
    fimex_amd::DeviceArray<uint64_t> tables;
};
