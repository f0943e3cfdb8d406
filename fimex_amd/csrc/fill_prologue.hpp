// What the fill sources share on the host: the prologue of the systolic kernels (statistics, first guess, masks), the launch of a
// batch of slices on them, and the sweeps over whole slices that the fills by rectangles (fill_rects.hip) drive.
#pragma once

#include "fill_sum.hpp"

namespace fimex_amd {

constexpr int kMaxBands = 4096;

struct FillStatsArgs {
    const float* field;
    SliceStats* stats;
    size_t total;
    int wantDeviation;   // fill2d: second pass for the convergence criterion (:1284-1302)
    int useDefault;      // creepfillval2d: the caller's value is the first guess, only the undefined cells are counted
    float defaultVal;
    float relaxCrit;
    int sumAlgo;
    const double* defaults;  // per slice, instead of defaultVal (the rectangles of a decomposed creep fill: the whole slice's average)
    const unsigned long long* bounds;  // per slice, with defaults: SliceStats::sweepBound
    const double* devs;                // per slice, with defaults: SliceStats::meanAbsDev (fill2d by rectangles: the whole field's criterion)
};

// fill_prologue.hip
void launch_fill_stats(const FillStatsArgs& s, size_t nz, hipStream_t stream);  // fill_stats_kernel, one workgroup per slice
void launch_fill_prologue(bool creep, float* d_field, SliceStats* d_stats, size_t nx, size_t ny, size_t nz, uint32_t* mask, uint32_t mws,
                          unsigned char* mbRows, unsigned char* mbCols, bool wantDeviation, bool useDefault, float defaultVal, float relaxCrit,
                          hipStream_t stream, const double* d_defaults = nullptr, const unsigned long long* d_bounds = nullptr,
                          const double* d_devs = nullptr);
int device_cus();
bool launch_resident(const void* kernel, dim3 grid, dim3 block, void** params, size_t ldsBytes, hipStream_t stream);
void collect_stats(const DeviceArray<SliceStats>& d_stats, size_t nz, size_t* h_nChanged, hipStream_t stream, const char* what);

// ---- the systolic launch of a batch [nz][ny][nx], shared by run_fill2d_whole and run_creepfill_whole
inline size_t fill_bands(size_t ny) { return ny > 2 ? (ny - 2 + kWave - 1) / kWave : 0; }  // bands of 64 interior rows
inline uint32_t fill_mask_words(size_t nx) { return (uint32_t)((nx + kWave + 31) / 32 + 2); }  // skewed columns 0 .. nx + 62, plus prefetch slack
bool systolic_fits(size_t nx, size_t ny);
size_t groups_per_slice(size_t nBands, size_t wavesPerWg, size_t nz);
DeviceArray<unsigned int> cleared_words(size_t n, hipStream_t stream);
bool launch_multi(const void* kernel, size_t groups, size_t nz, int threads, void* args, size_t ldsBytes, hipStream_t stream);
void launch_single(const void* kernel, size_t nz, int threads, void* args, size_t ldsBytes, hipStream_t stream);
void finish_systolic(const DeviceArray<unsigned int>& error, const DeviceArray<SliceStats>& stats, size_t nz, size_t* h_nChanged,
                     hipStream_t stream, const char* what);

// the per-slice words of the multi-workgroup kernels ([0] barrier counter, [1..3] the fill's own, [4 .. 4 + bands) progress words of
// the hand-offs that cross workgroups), zeroed, and the fields of the kernel's arguments that describe them
template <typename Args>
DeviceArray<unsigned int> multi_sync_words(Args& a, size_t nBands, size_t groups, size_t nz, hipStream_t stream)
{
    a.syncStride = (uint32_t)(4 + nBands);
    a.groups = (uint32_t)groups;
    a.nz = (uint32_t)nz;
    DeviceArray<unsigned int> sync = cleared_words(nz * a.syncStride, stream);
    a.sync = sync.get();
    return sync;
}

// fill.hip, creepfill.hip: the sweeps over whole slices [nz][ny][nx].  d_defaults / d_devs / d_bounds (device, per slice): first
// guess, convergence criterion and sweep bound given instead of computed; couple > 0: slices i, i + couple, ... end their sweeps
// together (fill2d by rectangles, see run_fill2d) -- false where that cannot be launched (nothing has been touched then).
bool run_fill2d_whole(size_t nx, size_t ny, size_t nz, float* d_field, float relaxCrit, float corrEff, size_t maxLoop,
                      size_t* h_nChanged, hipStream_t stream, const double* d_defaults, const double* d_devs, uint32_t couple);
void run_creepfill_whole(size_t nx, size_t ny, size_t nz, float* d_field, bool useDefault, float defaultVal,
                         unsigned short repeat, char setWeight, size_t* h_nChanged, hipStream_t stream, const double* d_defaults,
                         const unsigned long long* d_bounds = nullptr);

}  // namespace fimex_amd
