// Forward-mapping regrid (bucket reductions) for gfx950: the apply kernels that gather straight from memory.
//
// Replaces CachedForwardInterpolation (src/CachedForwardInterpolation.cc:38-131): the reference
// scans the source slice and push_back()s every value into a std::vector per target cell, then
// aggregates each vector (sum / mean / median / max / min).  With the scatter inverted at plan creation
// (forward_plan.hip) the apply kernel is a gather with no atomics and no allocation, and sums add in exactly the
// reference's order (bit-identical results).  The aggregation rules are forward_math.hpp's.
//
// Two apply paths, chosen per plan from its largest bucket:
//  * lane-per-target: one lane walks its bucket; ZC slices are reduced together so that the CSR
//    entries are read once per ZC slices;
//  * wave-per-target (large buckets): the 64 lanes load 64 bucket entries at a time (coalesced
//    index reads), a ballot drops undefined values, and the reduction is finished across the wave
//    (shuffle reduction for max / min, ordered lane scan for sum / mean so that the reference's
//    left-to-right float additions are kept).
// Dense mappings take the LDS-staged kernel of forward_tiled.hip, their medians the wave kernels of forward_median.hip.
#include "forward.hpp"
#include "forward_launch.hpp"

namespace fimex_amd {

namespace {

// One bucket, ZC slices at a time: sum / mean / max / min by ordered_step and, for Aggregate::Median, the median of buckets of at
// most two source cells (median_of_two_step; longer buckets: median_by_rank in the kernel below).
// i0: the bucket's first source cell, loaded once per lane outside the slice loop (most buckets hold one cell: no dependent
// index load per slice group is left).
// AHEAD: source cells whose values are requested before the first of them is added (1: none ahead -- plans whose buckets are short)
template <Aggregate A, bool UNDEF, int ZC, int AHEAD>
__device__ __forceinline__ void reduce_bucket(const FwdArgs& a, uint32_t b, uint32_t e, uint32_t i0, const float* src, const size_t (&koff)[ZC], float (&r)[ZC])
{
    float acc[ZC];
    uint32_t cnt[ZC];
    bool anyNan[ZC];
#pragma unroll
    for (int k = 0; k < ZC; ++k) { acc[k] = 0.f; cnt[k] = 0; anyNan[k] = false; }
    auto take = [&](const float (&v)[ZC]) __attribute__((always_inline)) {  // one source cell of the bucket, all ZC slices, in scan order
#pragma unroll
        for (int k = 0; k < ZC; ++k) {
            if constexpr (A == Aggregate::Median) median_of_two_step<UNDEF>(v[k], acc[k], cnt[k], anyNan[k]);
            else ordered_step<A, UNDEF>(v[k], acc[k], cnt[k]);
        }
    };
    uint32_t j = b;
    // long buckets (a source finer than the target): the values of AHEAD cells are requested before the first is added -- the
    // additions stay in scan order, but a lane no longer waits a memory round trip per cell (0.1-degree global -> 1-degree global,
    // 100 cells per bucket, 100 slices: 3.87 ms without, 1.74 ms with 4, 1.38 ms with 8 cells ahead; the registers this takes cost
    // the sparse plans of configs[3] 13 %, hence the variant without)
    if constexpr (AHEAD > 1)
    for (; j + AHEAD <= e; j += AHEAD) {
        uint32_t i[AHEAD];
#pragma unroll
        for (int q = 0; q < AHEAD; ++q) i[q] = (q == 0 && j == b) ? i0 : a.src[j + q];
        float v[AHEAD][ZC];
#pragma unroll
        for (int q = 0; q < AHEAD; ++q)
#pragma unroll
            for (int k = 0; k < ZC; ++k) v[q][k] = src[koff[k] + i[q]];
#pragma unroll
        for (int q = 0; q < AHEAD; ++q) take(v[q]);
    }
    for (; j < e; ++j) {
        const uint32_t i = (j == b) ? i0 : a.src[j];
        float v[ZC];
#pragma unroll
        for (int k = 0; k < ZC; ++k) v[k] = src[koff[k] + i];
        take(v);
    }
#pragma unroll
    for (int k = 0; k < ZC; ++k) {
        if constexpr (A == Aggregate::Median) r[k] = median_of_two_finish<UNDEF>(acc[k], cnt[k], anyNan[k]);
        else r[k] = finish<A, UNDEF>(acc[k], cnt[k], cnt[k], false);
    }
}

// one lane per target cell.  Workgroups are dealt round-robin over the 8 XCDs; XCD x takes the x-th eighth of the target
// cells (blocks of 256 consecutive cells), so that a source line -- whose cells map to neighbouring targets in several target
// rows -- is fetched into ONE L2 instead of into all eight (configs[3]: 1.85 GB -> about 1.1 GB of fabric traffic per 100 slices).
// RANK (median only): some bucket of the plan holds more than two cells; without it the rank-counting path is not compiled in
template <Aggregate A, bool UNDEF, int ZC, bool RANK = false, int AHEAD = 1>
__global__ void __launch_bounds__(kBlock) forward_apply_lane(FwdArgs a)
{
    const uint32_t perXcd = gridDim.x / kXcds;  // the grid holds 8 * perXcd workgroups per z chunk
    const uint32_t blk = (blockIdx.x % kXcds) * perXcd + blockIdx.x / kXcds;
    const uint32_t t = blk * kBlock + threadIdx.x;
    if (t >= a.nOut) return;
    const uint32_t z0 = blockIdx.y * a.zPerBlock;
    const uint32_t z1 = min(a.nz, z0 + a.zPerBlock);
    const uint32_t b = a.offsets[t], e = a.offsets[t + 1];
    const uint32_t i0 = (e > b) ? a.src[b] : 0u;
    if (A == Aggregate::Median && RANK && (e - b > 2 || (kTuningBuild && a.rankAll != 0))) {
        // median of a bucket of three or more source cells: value of rank size()/2 (std::nth_element, :49-53) by rank counting, slice
        // by slice -- no scratch memory, any bucket size; the other lanes of the wave (buckets of at most two cells, by far the
        // most in practice: DESIGN.md gives the occupancy histogram) take the batched path below
        for (uint32_t z = z0; z < z1; ++z) {
            const float* src = a.in + (size_t)z * a.inLayer;
            __builtin_nontemporal_store(median_by_rank<UNDEF>(e - b, [&](uint32_t j) { return src[a.src[b + j]]; }), a.out + (size_t)z * a.nOut + t);
        }
        return;
    }
    for (uint32_t z = z0; z < z1; z += ZC) {
        const float* src = a.in + (size_t)z * a.inLayer;
        // slices past the end of the chunk re-read the last one (results dropped): no branch in the gather loop
        size_t koff[ZC];
#pragma unroll
        for (int k = 0; k < ZC; ++k) koff[k] = (size_t)min((uint32_t)k, z1 - 1 - z) * a.inLayer;
        float r[ZC];
        reduce_bucket<A, UNDEF, ZC, AHEAD>(a, b, e, i0, src, koff, r);
#pragma unroll
        for (int k = 0; k < ZC; ++k)
            if (z + k < z1) __builtin_nontemporal_store(r[k], a.out + (size_t)(z + k) * a.nOut + t);
    }
}

// ---- wave-per-target path -------------------------------------------------------------------
template <Aggregate A>
__device__ __forceinline__ float wave_extremum(float v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const float o = __shfl_xor(v, d, kWave); v = beats<A>(o, v) ? o : v; }
    return v;
}

// one wave per target cell; 4 targets per workgroup
template <Aggregate A, bool UNDEF>
__global__ void __launch_bounds__(kBlock) forward_apply_wave(FwdArgs a)
{
    WaveTarget w;
    if (!wave_target(a, w)) return;
    const uint32_t lane = w.lane, b = w.b, e = w.b + w.len;
    for (uint32_t z = w.z0; z < w.z1; ++z) {
        const float* src = a.in + (size_t)z * a.inLayer;
        float acc = 0.f;       // running result, identical in every lane
        uint32_t cnt = 0;
        bool firstNan = false;  // max/min with UNDEF: a NaN in first position sticks (std::max_element)
        for (uint32_t base = b; base < e; base += kWave) {
            const uint32_t j = base + lane;
            const bool inRange = j < e;
            const float v = inRange ? src[a.src[j]] : 0.f;
            const bool valid = inRange && keep<UNDEF>(v);
            const unsigned long long mask = __ballot(valid);
            if (mask == 0) continue;
            if (is_sum(A)) {
                // ordered sum: fold the surviving lanes left to right, as std::accumulate does
                unsigned long long m = mask;
                while (m) {
                    const int l = __ffsll((long long)m) - 1;
                    acc = acc + __shfl(v, l, kWave);
                    m &= m - 1;
                }
            } else {
                if (UNDEF && cnt == 0) {
                    const int l0 = __ffsll((long long)mask) - 1;
                    firstNan = isnan(__shfl(v, l0, kWave));
                }
                // NaNs after the first position never win a "<" comparison: neutralise them
                const bool usableV = valid && !isnan(v);
                // std::max_element / min_element return the FIRST of the elements that compare equal to the extremum: of +0.0 and
                // -0.0 the one that comes first in the bucket.  The shuffle reduction finds the value, the lowest lane that holds it
                // supplies the bits.
                const float m = wave_extremum<A>(usableV ? v : start_value<A, UNDEF>());
                const unsigned long long at = __ballot(usableV && v == m);
                if (at) {
                    const float first = __shfl(v, __ffsll((long long)at) - 1, kWave);
                    acc = (cnt == 0 || beats<A>(first, acc)) ? first : acc;
                }
            }
            cnt += (uint32_t)__popcll(mask);
        }
        if (lane == 0) a.out[(size_t)z * a.nOut + w.t] = finish<A, UNDEF>(acc, cnt, cnt, firstNan);  // every kept value was counted
    }
}

using forward_launch::Family;
constexpr int kLaneZc = forward_launch::kLaneZc;
static_assert((int)Aggregate::Median == forward_launch::kAggregateMedian && (uint32_t)kBlock == forward_launch::kBlock && (uint32_t)kXcds == forward_launch::kXcds,
              "forward_launch.hpp restates the constants of plan.hpp and common.hpp");

// sums and extrema (and the median of single cells as a maximum): the kernel forward_launch.hpp names
template <Aggregate A, bool UNDEF>
void launch_kind(const FwdArgs& a, const forward_launch::Launch& l, dim3 grid, hipStream_t stream)
{
    if (l.family == Family::Wave) {
        forward_apply_wave<A, UNDEF><<<wave_grid(a, grid.y), kBlock, 0, stream>>>(a);
    } else if (l.ahead == 8) {
        forward_apply_lane<A, UNDEF, kLaneZc, false, 8><<<grid, kBlock, 0, stream>>>(a);
    } else if (l.zc == 1) {
        // one slice per call is the reference's own call pattern (src/CDMInterpolator.cc:251-259): no eight-slice passes that read
        // the one slice eight times (configs[3], one slice: see DESIGN.md 6)
        forward_apply_lane<A, UNDEF, 1><<<grid, kBlock, 0, stream>>>(a);
    } else if (l.zc == 2) {
        forward_apply_lane<A, UNDEF, 2><<<grid, kBlock, 0, stream>>>(a);
    } else if (l.zc == 4) {
        forward_apply_lane<A, UNDEF, 4><<<grid, kBlock, 0, stream>>>(a);
    } else {
        forward_apply_lane<A, UNDEF, kLaneZc><<<grid, kBlock, 0, stream>>>(a);
    }
}

// -1: not set
forward_launch::Tuning read_tuning()
{
    forward_launch::Tuning t;
    t.tiled = tuning("FWD_TILED", -1);
    t.zpb = tuning("FWD_ZPB", -1);
    t.wave = tuning("FWD_WAVE", -1);
    t.medianShort = tuning("FWD_MEDIAN_SHORT", -1);
    t.medianWaveMin = tuning("FWD_MEDIAN_WAVE_MIN", -1);
    t.medianWave = tuning("FWD_MEDIAN_WAVE", -1);
    t.medianZc = tuning("FWD_MEDIAN_ZC", -1);
    return t;
}

}  // namespace

// The choice of kernel and the z chunks are forward_launch.hpp's (the measurements behind its thresholds: DESIGN.md 6):
//  * z chunks: a workgroup reads its CSR entries once per chunk, so chunks are long (the CSR of configs[3] is 10 MB, a slice's
//    must-move bytes about the same); several chunks only where the target grid alone would not fill the chip;
//  * wave per bucket only where the targets are too few to fill the chip with lanes: a dense mapping with many targets runs
//    1.7-1.8 ms through the lane kernels against 6.5 (mean: the ordered fold) and 2.0 ms (max) through the wave kernels (0.1-degree
//    global -> 1-degree global, 100 cells per bucket, 100 slices);
//  * the median of medium buckets throughout (a source finer than the target) by one wave per target: its cost does not depend on
//    the bucket's length (25 ms per 100 slices of a million targets), the lane kernel's rank counting grows with its square (6.3 ms
//    at 4-9 cells, about 32 at 25): a wave per target from a mean length of twelve;
//  * the median of buckets of at most two cells: eight slices in flight, no rank counting (four targets per lane with 16-byte stores
//    were measured as well: 8 % slower on configs[3], the gathers lose parallelism).
void launch_forward_apply(const fimex_amd_regrid_plan& plan, const float* d_in, size_t nz, float* d_out, hipStream_t stream)
{
    if (nz == 0) return;
    FA_REQUIRE(nz <= 0xFFFFFFFFu, "too many slices");
    const size_t nOut = plan.outX * plan.outY;
    const forward_launch::Launch l = forward_launch::forward_launch(nOut, nz, plan.info.mappedSourceCells, plan.info.undefinedCells, plan.info.maxBucket,
                                                                    (int)plan.aggregate, plan.fwdTiles.valid, read_tuning());
    if (l.family == Family::Tiled && launch_forward_tiled(plan, d_in, nz, d_out, stream)) return;
    FA_REQUIRE(l.family != Family::Tiled, "the tiled forward kernel refused a plan that holds its tiles");
    FwdArgs a{};
    a.in = d_in;
    a.out = d_out;
    a.offsets = plan.offsets.get();
    a.src = plan.src.get();
    a.nOut = (uint32_t)nOut;
    a.inLayer = plan.inX * plan.inY;
    a.nz = (uint32_t)nz;
    a.rankAll = l.rankAll ? 1u : 0u;
    a.zPerBlock = l.zPerBlock;
    FA_REQUIRE(l.chunksFit(), "too many z chunks for one launch");
    // the lane kernels map workgroup -> block of targets through the XCD it runs on: their grid is a multiple of 8
    const dim3 gridLane(l.laneGridX, (uint32_t)l.chunks, 1);
    const bool u = plan.undefAggr;
    switch (l.family) {
    case Family::MedianAsMax:
        with_aggregate(Aggregate::Max, u, [&](auto A, auto U) { launch_kind<A(), U()>(a, l, gridLane, stream); });
        break;
    case Family::MedianWave:
        launch_forward_median_wave(a, plan.info.maxBucket, u, gridLane.y, stream);
        break;
    case Family::Lane:
        if (plan.aggregate == Aggregate::Median) {
            with_undef(u, [&](auto U) {
                if (l.rank) forward_apply_lane<Aggregate::Median, U(), kLaneZc, true><<<gridLane, kBlock, 0, stream>>>(a);
                else if (l.zc == 4) forward_apply_lane<Aggregate::Median, U(), 4><<<gridLane, kBlock, 0, stream>>>(a);
                else forward_apply_lane<Aggregate::Median, U(), kLaneZc><<<gridLane, kBlock, 0, stream>>>(a);
            });
            break;
        }
        [[fallthrough]];
    default:  // Family::Wave, and the lanes of sums and extrema
        with_aggregate(plan.aggregate, u, [&](auto A, auto U) { launch_kind<A(), U()>(a, l, gridLane, stream); });
        break;
    }
    FA_HIP(hipGetLastError());
}

}  // namespace fimex_amd
