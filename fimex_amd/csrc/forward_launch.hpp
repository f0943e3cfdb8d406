// Which kernel a forward apply launches and how it cuts the batch (launch_forward_apply, forward.hip): pure C++, no device code --
// tests/forward_launch_host.cc compiles it on its own, tests/test_forward_launch.py checks the rule and its invariants on the
// CPU, and the GPU tests of the slice loops ask it which kernel, how many z chunks and how many passes per chunk a case runs.
#pragma once

#include <cstddef>
#include <cstdint>

namespace fimex_amd {
namespace forward_launch {

constexpr uint32_t kBlock = 256;          // target cells per workgroup of the lane kernels
constexpr uint32_t kXcds = 8;             // the lane kernels' grid is a multiple of this
constexpr uint32_t kMaxChunks = 65535;    // gridDim.y
constexpr int kLaneZc = 8;                // slices a lane reduces together (gathers in flight per lane)
constexpr int kAggregateMedian = 2;       // Aggregate::Median (plan.hpp)

enum class Family : int {
    Tiled = 0,        // the LDS-staged kernel of forward_tiled.hip, which keeps its own z schedule
    Lane = 1,         // forward_apply_lane<A, UNDEF, zc, rank, ahead>
    Wave = 2,         // forward_apply_wave<A, UNDEF>: one slice at a time
    MedianWave = 3,   // the wave kernels of forward_median.hip
    MedianAsMax = 4,  // the median of single cells: forward_apply_lane<Max, UNDEF, zc>
};

// The switches of the tuning build as launch_forward_apply reads them; -1: not set (the product build: all of them).
struct Tuning {
    int tiled = -1;          // FWD_TILED: 0 = never the tiled kernel
    int zpb = -1;            // FWD_ZPB: slices per z chunk before the chunks are made equal
    int wave = -1;           // FWD_WAVE: 0 = never, any other value = always the wave kernel (sums and extrema)
    int medianShort = -1;    // FWD_MEDIAN_SHORT: 0 = the median of every bucket by rank counting
    int medianWaveMin = -1;  // FWD_MEDIAN_WAVE_MIN: mean bucket length from which the median takes a wave per target
    int medianWave = -1;     // FWD_MEDIAN_WAVE: 0 = never the wave median
    int medianZc = -1;       // FWD_MEDIAN_ZC: 4 = the median of at most two cells four slices at a time
};

struct Launch {
    Family family;
    int zc;              // slices per pass of the lane kernel's loop (wave kernels: 1)
    int ahead;           // source cells requested before the first is added (1: none ahead)
    bool rank;           // median only: the rank-counting path is compiled in
    bool rankAll;        // FWD_MEDIAN_SHORT=0: every bucket takes it
    uint32_t zPerBlock;  // slices per z chunk, the same for every chunk but the last
    uint64_t chunks;     // z chunks; more than kMaxChunks cannot be launched (chunksFit)
    uint32_t laneGridX;  // workgroups per z chunk of the lane kernels
    double meanBucket;   // source cells per non-empty target
    bool chunksFit() const { return chunks <= kMaxChunks; }
};

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// slices per pass of the lane kernels that look no cell ahead: one slice per call is the reference's own call pattern, so short
// batches do not run eight-slice passes that read their last slice again and again
inline int short_batch_zc(uint64_t nz) { return nz == 1 ? 1 : nz <= 2 ? 2 : nz <= 4 ? 4 : kLaneZc; }

// nOut target cells (at least one), nz slices (at least one); mappedSourceCells, undefinedCells (empty targets) and maxBucket as
// the plan's info reports them; aggregate: Aggregate's value; tilesValid: the plan holds a tiled form.
inline Launch forward_launch(uint64_t nOut, uint64_t nz, uint64_t mappedSourceCells, uint64_t undefinedCells, uint64_t maxBucket, int aggregate,
                             bool tilesValid, const Tuning& t)
{
    Launch l{};
    const bool median = aggregate == kAggregateMedian;
    l.zc = 1;
    l.ahead = 1;
    l.rankAll = t.medianShort == 0;
    // z chunks: a workgroup reads its CSR entries once per chunk, so chunks are long; several chunks only where the target grid
    // alone would not fill the chip
    const uint64_t blocks = ceil_div(nOut, kBlock);
    uint64_t zpb = t.zpb > 0 ? (uint64_t)t.zpb : (blocks >= 4096 ? 64u : 16u);
    if (zpb > nz) zpb = nz;
    l.chunks = ceil_div(nz, zpb);
    zpb = ceil_div(nz, l.chunks);  // chunks of one size
    l.zPerBlock = (uint32_t)zpb;
    l.chunks = ceil_div(nz, zpb);
    l.laneGridX = (uint32_t)(ceil_div(blocks, kXcds) * kXcds);
    const uint64_t nonEmpty = nOut - undefinedCells;
    l.meanBucket = nonEmpty ? (double)mappedSourceCells / (double)nonEmpty : 0.0;
    if (tilesValid && !median && t.tiled != 0) {  // dense mappings, all aggregates but the median
        l.family = Family::Tiled;
        return l;
    }
    if (!median) {
        // wave per bucket only where the buckets are long and the targets too few to fill the chip with lanes (fewer than 64 K
        // (target, z chunk) lanes)
        const bool wave = t.wave < 0 ? (l.meanBucket >= 32.0 && nOut * l.chunks < 65536) : t.wave != 0;
        if (wave) {
            l.family = Family::Wave;
        } else if (l.meanBucket > 4.0) {  // the lane kernels with eight cells of look-ahead
            l.family = Family::Lane;
            l.zc = kLaneZc;
            l.ahead = 8;
        } else {
            l.family = Family::Lane;
            l.zc = short_batch_zc(nz);
        }
        return l;
    }
    if (maxBucket <= 1 && !l.rankAll) {
        // no bucket holds more than one cell: the median of one value is the value, which is what the max kernel returns for it
        l.family = Family::MedianAsMax;
        l.zc = short_batch_zc(nz);
        return l;
    }
    const int waveMin = t.medianWaveMin >= 0 ? t.medianWaveMin : 12;
    if (!l.rankAll && maxBucket > 2 && maxBucket <= 256 && l.meanBucket >= (double)waveMin && t.medianWave != 0) {
        l.family = Family::MedianWave;  // medium buckets throughout: one wave per target, the median by selection on keys
        return l;
    }
    // buckets of at most two cells: eight (or four) slices in flight, no rank counting; longer ones are ranked slice by slice by
    // the same kernel
    l.family = Family::Lane;
    l.rank = maxBucket > 2 || l.rankAll;
    l.zc = (!l.rank && t.medianZc == 4) ? 4 : kLaneZc;
    return l;
}

}  // namespace forward_launch
}  // namespace fimex_amd
