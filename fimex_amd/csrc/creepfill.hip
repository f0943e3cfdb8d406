// Creep fills (mifi_creepfill2d_f / mifi_creepfillval2d_f, src/interpolation.c:1378-1537) over whole slices; the order of
// the sweeps and the systolic scheme are those of fill.hip.
#include "fill_prologue.hpp"
#include "fill_sync.hpp"

#include <algorithm>

namespace fimex_amd {

namespace {

// ------------------------------------------------------------------------------- creep fill
struct CreepArgs {
    float* field;
    signed char* w;     // workspace, one byte per cell (:1389)
    unsigned short* r;  // workspace, one ushort per cell (:1394)
    SliceStats* stats;
    uint32_t nx, ny;
    int useDefault;
    float defaultVal;
    unsigned short repeat;
    signed char setWeight;
    int sumAlgo;
    const double* defaults;  // per slice, see FillStatsArgs
    const unsigned long long* bounds;
};

__global__ void __launch_bounds__(kFillBlock) creepfill_kernel(CreepArgs a)
{
    __shared__ __align__(16) double lds[2 * kSumTile];
    __shared__ unsigned long long shUndef;
    __shared__ float shDefault;
    __shared__ unsigned int shChanged;
    const uint32_t nx = a.nx, ny = a.ny;
    const size_t total = (size_t)nx * ny;
    float* f = a.field + (size_t)blockIdx.x * total;
    signed char* w = a.w + (size_t)blockIdx.x * total;
    unsigned short* r = a.r + (size_t)blockIdx.x * total;
    SliceStats* st = a.stats + blockIdx.x;

    unsigned long long nUndef = 0;
    const double sum = scan_order_sum(f, total, a.useDefault ? 2 : 0, 0., lds, &nUndef, a.sumAlgo);  // a default value needs no average
    if (threadIdx.x == 0) {
        shUndef = nUndef;
        const unsigned long long nDef = total - nUndef;
        shDefault = a.defaults ? (float)a.defaults[blockIdx.x] : (a.useDefault ? a.defaultVal : ((nDef != 0) ? (float)(sum / (double)nDef) : 0.f));  // :1516
        st->nUndef = nUndef;
        st->status = 1;
    }
    __syncthreads();
    nUndef = shUndef;
    const unsigned long long nDef = total - nUndef;
    if (nDef == 0 || nUndef == 0) return;  // :1384-1386, :1515
    if (nx < 2 || ny < 2) { if (threadIdx.x == 0) st->status = -1; return; }
    const float defaultVal = shDefault;
    const unsigned short repeat = a.repeat;

    for (size_t i = threadIdx.x; i < total; i += kFillBlock) {  // :1408-1421
        if (isnan(f[i])) { w[i] = 0; r[i] = 0; f[i] = defaultVal; }
        else { w[i] = a.setWeight; r[i] = repeat; }
    }
    __syncthreads();

    const uint32_t nxm1 = nx - 1, nym1 = ny - 1;
    const bool hasInterior = nx > 2 && ny > 2;
    unsigned long long l = 0;
    unsigned int changedInLoop = 1;
    const unsigned long long bound = a.bounds ? a.bounds[blockIdx.x] : nDef;
    while (changedInLoop > 0 && l < bound) {  // :1430
        l++;
        if (threadIdx.x == 0) shChanged = 0;
        __syncthreads();
        unsigned int mine = 0;
        if (hasInterior) {
            const uint32_t dLast = (nx - 2) + (ny - 2);
            for (uint32_t d = 2; d <= dLast; ++d) {
                const uint32_t xlo = (d > (ny - 2)) ? d - (ny - 2) : 1;
                const uint32_t xhi = (d - 1 < nx - 2) ? d - 1 : nx - 2;
                for (uint32_t x = xlo + threadIdx.x; x <= xhi; x += kFillBlock) {
                    const size_t p = (size_t)(d - x) * nx + x;
                    if (r[p] < repeat) {  // :1443
                        const int wr = w[p + 1], wl = w[p - 1], wd = w[p + nx], wu = w[p - nx];
                        const size_t wsum = (size_t)(wr + wl + wd + wu);  // :1445
                        if (wsum != 0) {
                            float v = f[p];
                            v += wr * f[p + 1] + wl * f[p - 1] + wd * f[p + nx] + wu * f[p - nx];  // :1451
                            v /= (float)(1 + wsum);                                                // :1452
                            f[p] = v;
                            w[p] = 1;
                            r[p] = r[p] + 1;
                            mine++;
                        }
                    }
                }
                __syncthreads();
            }
        }
        if (mine) atomicAdd(&shChanged, mine);
        __syncthreads();
        changedInLoop = shChanged;
        __syncthreads();
    }
    for (unsigned int k = 0; k < repeat; ++k) {  // :1464-1489
        for (uint32_t y = 1 + threadIdx.x; y < nym1; y += kFillBlock) {
            const size_t row = (size_t)y * nx;
            if (r[row] < repeat) {
                f[row] += f[row + 1] * w[row + 1];
                f[row] /= (float)(1 + w[row + 1]);
                w[row] = 1;
            }
            if (r[row + nxm1] < repeat) {
                f[row + nxm1] += f[row + nx - 2] * w[row + nx - 2];
                f[row + nxm1] /= (float)(1 + w[row + nx - 2]);
                w[row + nxm1] = 1;
            }
        }
        __syncthreads();
        for (uint32_t x = threadIdx.x; x < nx; x += kFillBlock) {
            const size_t b = (size_t)nym1 * nx + x;
            if (r[x] < repeat) {
                f[x] += f[nx + x] * w[nx + x];
                f[x] /= (float)(1 + w[nx + x]);
                w[x] = 1;
            }
            if (r[b] < repeat) {
                f[b] += f[b - nx] * w[b - nx];
                f[b] /= (float)(1 + w[b - nx]);
                w[b] = 1;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ creep fill, systolic version
// Same row-band pipeline as fill2d_kernel_v2 (lane = row, skewed columns, LDS ring, LDS hand-off between bands).
// The reference's per-cell state (:1389-1421) is folded into bit masks in the same skewed layout as the rings:
//   D  cell was defined on entry                      w = setWeight, r = repeat, never updated
//   U  cell has been updated at least once            w = 1
// A cell that starts being updated in sweep s is updated in every sweep s .. s + repeat - 1 (its neighbours never
// lose their weight), so "r[p] < repeat" in sweep l is "p is not in U as of sweep l - repeat": U is kept for the
// last repeat + 1 sweeps instead of a counter per cell.  Weights travel as floats (0, 1, setWeight: all exact).
constexpr int kCreepWaves = 8;    // 8 waves x 256 registers: the creep step keeps more state than the 128 registers of a 16-wave workgroup hold
constexpr int kCreepThreads = kCreepWaves * kWave;
constexpr int kCreepCh = 32;                        // 128-byte row pieces per chunk: whole lines, one memory event per 32 columns
constexpr int kCreepRingW = 2 * kCreepCh;
constexpr int kCreepPitch = kCreepRingW + 1;
constexpr int kCreepRowsPerIt = kWave / kCreepCh;
constexpr int kCreepChunksPerWord = 32 / kCreepCh;
constexpr int kHandWC = 128;  // hand-off window of the creep kernel: values and weight codes share the LDS left

struct CreepV2Args {
    float* field;
    uint32_t* maskD;   // [nz][ny][mws]           interior rows skewed by (y - 1) & 63, rows 0 and ny - 1 unskewed
    uint32_t* maskU;   // [nz][gens][ny][mws]     zero on entry
    SliceStats* stats;
    uint32_t nx, ny, mws, gens;
    int useDefault;
    float defaultVal;
    uint32_t repeat;
    int setWeight;     // >= 0
    int sumAlgo;
    int skipIdle;
    unsigned int* error;  // one word per launch: set by a wait that gave up (see MultiWg)
    // several workgroups per slice (creepfill_kernel_v3): per slice [0] barrier counter, [1..3] "something changed" by sweep
    // mod 3, [4 .. 4 + bands) progress words of the hand-offs that cross workgroups
    unsigned int* sync;
    uint32_t syncStride, groups, nz;
};

struct HandoffC {
    float* data;             // [16][2][kHandWC]
    unsigned char* wcode;    // [16][2][kHandWC]  0, 1, 2 = setWeight
    unsigned int* produced;  // [16][2]
    unsigned int* consumed;  // [16][2]
};

// value of lane l+1 (lane 63 keeps its own): "wave_shl:1" (0x130)
__device__ __forceinline__ uint32_t lane_from_below(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x130, 0xf, 0xf, false);
}

template <bool MULTI>
__device__ void creep_band(float* __restrict__ f, const uint32_t* __restrict__ maskD, const uint32_t* __restrict__ uOld,
                           const uint32_t* __restrict__ uHist, uint32_t* __restrict__ uNew, float* ring, HandoffC hand, uint32_t b,
                           uint32_t nx, uint32_t ny, uint32_t mws, float swf, bool skipIdle, int& changed, MultiWg mg)
{
    unsigned int* const error = mg.error;
    using rsrc_t = __amdgpu_buffer_rsrc_t;
    b = __builtin_amdgcn_readfirstlane(b);  // wave-uniform, see fill2d_band
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t y0 = 1 + kWave * b;
    const uint32_t nrow = min((uint32_t)kWave, (ny - 1) - y0);
    const uint32_t L = nrow - 1;
    const bool rowValid = lane < nrow;
    const uint32_t y = y0 + min(lane, L);
    const uint32_t C = nx - 2;
    const uint32_t xpEnd = C + L;
    float* ringRow = ring + lane * kCreepPitch;
    const float* ringBelow = ring + min(lane + 1, (uint32_t)kWave - 1) * kCreepPitch;
    const float left0 = f[(size_t)y * nx];
    const uint32_t* drow = maskD + (size_t)y * mws;
    const uint32_t* urow = uOld + (size_t)y * mws;
    const uint32_t* hrow = uHist ? uHist + (size_t)y * mws : nullptr;
    uint32_t* nrowU = uNew + (size_t)y * mws;
    const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(f + (size_t)(y0 - 1) * nx, 0, (nrow + 2) * nx * 4u, 0x00020000);
    const bool hasBelow = y0 + nrow < ny - 1;
    const bool outGlobal = hasBelow && (b % kCreepWaves) == kCreepWaves - 1;
    const bool inGlobal = b > 0 && (b % kCreepWaves) == 0;
    const bool writeThrough = MULTI && outGlobal;  // several workgroups per slice: the band below runs on another CU (fill2d_band)
    const uint32_t kOob = 0xFFFFFFFFu;
    // weight of border column 0 of my row: skewed column = lane
    const float wLeft0 = ((drow[lane >> 5] >> (lane & 31)) & 1u) ? swf : 0.f;

    const uint32_t crow = lane / kCreepCh, ccol = lane % kCreepCh;
    float stage[kCreepCh];
    auto chunk_off = [&](uint32_t c, uint32_t it, bool store) -> uint32_t {
        const uint32_t row = kCreepRowsPerIt * it + crow;
        const int64_t x = (int64_t)c * kCreepCh + ccol - row;
        const bool ok = row < nrow && (store ? (x >= 1 && x <= (int64_t)C) : (x >= 0 && x <= (int64_t)nx - 1));
        return ok ? (uint32_t)(((row + 1) * nx + x) * 4u) : kOob;
    };
    // interior chunks: lean addressing, see fill2d_band
    auto interior = [&](uint32_t c) -> bool { return nrow == (uint32_t)kWave && c * kCreepCh >= (uint32_t)kWave && c * kCreepCh + kCreepCh - 1 <= C; };
    const uint32_t voffLane = ((crow + 1) * nx + ccol - crow) * 4u;           // row crow, chunk 0, column ccol - crow
    const uint32_t rowStep = (uint32_t)kCreepRowsPerIt * (nx - 1) * 4u;            // next row group: kCreepRowsPerIt rows down, as many columns back
    float* ringLane = ring + crow * kCreepPitch + ccol;
    auto load_chunk = [&](uint32_t c) {
        if (interior(c)) {
            const uint32_t s0 = c * kCreepCh * 4u;
#pragma unroll
            for (uint32_t it = 0; it < (uint32_t)kCreepCh; ++it)
                stage[it] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voffLane, s0 + it * rowStep, 0));
            return;
        }
#pragma unroll
        for (uint32_t it = 0; it < (uint32_t)kCreepCh; ++it)
            stage[it] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, chunk_off(c, it, false), 0, 0));
    };
    auto commit_chunk = [&](uint32_t c) {
        float* dst = ringLane + ((c * kCreepCh) & kCreepCh);
#pragma unroll
        for (uint32_t it = 0; it < (uint32_t)kCreepCh; ++it) dst[kCreepRowsPerIt * it * kCreepPitch] = stage[it];
    };
    // ring -> registers before the slot is refilled, registers -> global behind the event's loads (see fill2d_band)
    float v[kCreepCh];
    auto flush_read = [&](uint32_t c) {
        const float* src = ringLane + ((c * kCreepCh) & kCreepCh);
#pragma unroll
        for (uint32_t it = 0; it < (uint32_t)kCreepCh; ++it) v[it] = src[kCreepRowsPerIt * it * kCreepPitch];
    };
    auto flush_store = [&](uint32_t c) {
        if (interior(c)) {
            const uint32_t s0 = c * kCreepCh * 4u;
#pragma unroll
            for (uint32_t it = 0; it < (uint32_t)kCreepCh; ++it) {
                if (writeThrough) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[it]), rs, voffLane, s0 + it * rowStep, 17);
                else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[it]), rs, voffLane, s0 + it * rowStep, 0);
            }
            return;
        }
#pragma unroll
        for (uint32_t it = 0; it < (uint32_t)kCreepCh; ++it) {
            if (writeThrough) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[it]), rs, chunk_off(c, it, true), 0, 17);
            else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[it]), rs, chunk_off(c, it, true), 0, 0);
        }
    };
    // this sweep's U word of my row: the band below reads the last row's words (weights of its "up" cells)
    auto store_u = [&](uint32_t word, uint32_t value) {
        if (writeThrough) __hip_atomic_store(&nrowU[word], value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else nrowU[word] = value;
    };
    auto load_block = [&](uint32_t rowInBuf, uint32_t k) {
        const uint32_t col = 64 * k + lane;
        const uint32_t off = col <= nx - 1 ? (rowInBuf * nx + col) * 4u : kOob;
        if (MULTI && inGlobal && rowInBuf == 0) return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 17));  // see fill2d_band
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
    };
    // weights of 64 columns of an unskewed row (row 0, the first row of the band below, row ny - 1)
    auto load_wblock = [&](uint32_t yRow, uint32_t k) -> float {
        const uint32_t col = min(64 * k + lane, nx - 1);
        const uint32_t d = maskD[(size_t)yRow * mws + (col >> 5)], u = uOld[(size_t)yRow * mws + (col >> 5)];
        return ((d >> (col & 31)) & 1u) ? swf : (float)((u >> (col & 31)) & 1u);
    };

    const uint32_t round = kCreepWaves * (MULTI ? mg.G : 1u);
    const uint32_t slotOut = (b % kCreepWaves) * 2 + ((b / round) & 1);
    const uint32_t slotIn = ((b - 1) % kCreepWaves) * 2 + (((b - 1) / round) & 1);
    float* handOut = hand.data + slotOut * kHandWC;
    unsigned char* handOutW = hand.wcode + slotOut * kHandWC;
    const float* handIn = hand.data + slotIn * kHandWC;
    const unsigned char* handInW = hand.wcode + slotIn * kHandWC;
    if (lane == 0) {
        __hip_atomic_store(&hand.produced[slotOut], hand_tag(b, 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(&hand.consumed[slotOut], hand_tag(b, 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // every 16th boundary goes through global memory (see fill2d_band): values from the flushed row, weights from the
    // D mask and this sweep's U words of that row (skew 63), which the producing band stores at every event
    auto wait_above = [&](uint32_t cols) {  // chunk by chunk, see fill2d_band
        cols = min(cols, C + 1);
        if (MULTI) { wait_global_at_least(&mg.flags[b - 1], cols + 1, error); return; }
        wait_lds_at_least(&hand.produced[slotIn], hand_tag(b - 1, cols), error);
    };
    auto load_wblock_above = [&](uint32_t k) -> float {
        const uint32_t xs = min(64 * k + lane, nx - 1) + (kWave - 1);
        const uint32_t d = maskD[(size_t)(y0 - 1) * mws + (xs >> 5)];
        const uint32_t u = MULTI ? __hip_atomic_load(&uNew[(size_t)(y0 - 1) * mws + (xs >> 5)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                 : uNew[(size_t)(y0 - 1) * mws + (xs >> 5)];
        return ((d >> (xs & 31)) & 1u) ? swf : (float)((u >> (xs & 31)) & 1u);
    };
    // columns [xpc, xpc + kCreepCh) of the row above (values and weights) into lanes (column % 64)
    auto take_above = [&](uint32_t xpc, float& fv, float& wv) {
        wait_lds_at_least(&hand.produced[slotIn], hand_tag(b - 1, min(xpc + kCreepCh, C + 1)), error);
        const uint32_t col = (xpc & ~63u) + lane;
        const float v = handIn[col % kHandWC];
        const unsigned int code = handInW[col % kHandWC];
        if (lane - (xpc & 63u) < (uint32_t)kCreepCh) { fv = v; wv = (code == 2u) ? swf : (float)code; }
        if (lane == 0)
            lds_publish(&hand.consumed[slotIn], hand_tag(b - 1, xpc + kCreepCh));
    };

    load_chunk(0);
    commit_chunk(0);
    load_chunk(1);
    commit_chunk(1);
    load_chunk(2);
    float upCur = 0.f, upWCur = 0.f, upLd = 0.f, upWLd = 0.f;
    const bool fromGlobal = b == 0 || inGlobal;
    if (fromGlobal) {  // see fill2d_band: the chunk in work in lanes (column % 64), the next chunk's block one event ahead
        if (inGlobal) wait_above(kCreepCh);
        upCur = load_block(0, 0);
        upWCur = inGlobal ? load_wblock_above(0) : load_wblock(0, 0);
        if (inGlobal) wait_above(2 * kCreepCh);
        upLd = load_block(0, kCreepCh >> 6);
        upWLd = inGlobal ? load_wblock_above(kCreepCh >> 6) : load_wblock(0, kCreepCh >> 6);
    } else take_above(0, upCur, upWCur);
    const uint32_t yBelow = y0 + nrow;
    float downA = load_block(nrow + 1, 0), downB = downA, downLd = 0.f;
    float downWA = load_wblock(yBelow, 0), downWB = downWA, downWLd = 0.f;
    uint32_t downIssued = 0;
    bool downLdValid = false;
    const uint32_t wLast = mws - 1;
    uint32_t dw = drow[0], dwN = drow[1], dwLd = drow[min(2u, wLast)];
    uint32_t uw = urow[0], uwN = urow[1], uwLd = urow[min(2u, wLast)];
    uint32_t hw = hrow ? hrow[0] : 0u, hwN = hrow ? hrow[1] : 0u, hwLd = hrow ? hrow[min(2u, wLast)] : 0u;
    uint32_t ddw = lane_from_below(dw), ddwN = lane_from_below(dwN), duw = lane_from_below(uw), duwN = lane_from_below(uwN);
    uint32_t un = 0;
    float prevRes = 0.f, prevW = 0.f;
    float prevRight = ringRow[1];

    const uint32_t nChunks = xpEnd / kCreepCh + 1;
    for (uint32_t c = 0; c < nChunks; ++c) {
        const uint32_t xpc = c * kCreepCh;
        if (c > 0) {
            if (outGlobal) {
                if (xpc > L) {  // stores of the previous event have landed: columns < 16 (c - 1) - L of the last row, values and U bits
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (lane == 0 && xpc - kCreepCh > L) {
                        if (MULTI) __hip_atomic_store(&mg.flags[b], xpc - kCreepCh - L + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        else lds_publish(&hand.produced[slotOut], hand_tag(b, xpc - kCreepCh - L));
                    }
                }
                if (rowValid) store_u((c - 1) / kCreepChunksPerWord, un);  // the (partial) word of the chunk just finished
            }
            // small loads first, the chunk prefetch last (see fill2d_band)
            if ((c % kCreepChunksPerWord) == 0) {  // x' is a multiple of 32: the finished U word goes out, every lane switches words
                if (rowValid) store_u(c / kCreepChunksPerWord - 1, un);
                un = 0;
                const uint32_t nxt = min(c / kCreepChunksPerWord + 2, wLast);
                dw = dwN; dwN = dwLd; dwLd = drow[nxt];
                uw = uwN; uwN = uwLd; uwLd = urow[nxt];
                hw = hwN; hwN = hwLd; hwLd = hrow ? hrow[nxt] : 0u;
                ddw = ddwN; ddwN = lane_from_below(dwN);
                duw = duwN; duwN = lane_from_below(uwN);
            }
            if (downLdValid) { downB = downLd; downWB = downWLd; downLdValid = false; }
            if (xpc + 2 * kCreepCh > L && ((xpc + 2 * kCreepCh - L) >> 6) > downIssued) {  // block j + 1 is requested two chunks before the last lane
                // reaches it and lands in downB at the next event: after block j has moved on to downA, never skipping one
                ++downIssued;
                downLd = load_block(nrow + 1, downIssued);
                downWLd = load_wblock(yBelow, downIssued);
                downLdValid = true;
            }
            if (fromGlobal) {
                if (lane - (xpc & 63u) < (uint32_t)kCreepCh) { upCur = upLd; upWCur = upWLd; }  // this chunk's columns, requested one event ago
                const uint32_t k = (xpc + kCreepCh) >> 6;
                if (inGlobal) wait_above(xpc + 2 * kCreepCh);
                upLd = load_block(0, k);
                upWLd = inGlobal ? load_wblock_above(k) : load_wblock(0, k);
            }
            flush_read(c - 1);
            commit_chunk(c + 1);
            load_chunk(c + 2);  // as soon as its registers are free, before the waits on the neighbouring bands (see fill2d_band)
            if (xpc > L && !outGlobal) {
                if (lane == 0)
                    lds_publish(&hand.produced[slotOut], hand_tag(b, xpc - L));
                if (hasBelow) {
                    const unsigned int limit = xpc + kCreepCh - L;
                    unsigned long long tSpin = 0;
                    for (unsigned int it = 0;; ++it) {
                        const unsigned int cns = lds_observe(&hand.consumed[slotOut]);
                        if (limit <= (cns & 0x7FFFFu) + kHandWC) break;
                        __builtin_amdgcn_s_sleep(1);
                        if ((it & 0xFFF) == 0xFFF && (spin_expired(tSpin) || launch_failed(error))) { fail_launch(error, 3); break; }
                    }
                }
            }
            if (!fromGlobal) take_above(xpc, upCur, upWCur);
            flush_store(c - 1);
        }
        const uint32_t xp0 = max(xpc, 1u), xp1 = min(xpc + kCreepCh - 1, xpEnd);
        // A chunk in which no row has a cell that may still change (undefined on entry and not yet updated `repeat` times:
        // neither D nor H) is passed over: nothing is computed, the state the next chunk and the band below need is taken
        // from the ring and the masks.  After the first sweeps that is most of the field.
        const uint32_t chunkBits = ((xp1 - xp0 + 1 >= 32) ? 0xFFFFFFFFu : ((1u << (xp1 - xp0 + 1)) - 1u)) << (xp0 & 31);
        if (skipIdle && !__any(rowValid && ((~dw & ~hw & chunkBits) != 0u))) {
            for (uint32_t xp = xp0; xp <= xp1; ++xp)
                if (xp > L && ((xp - L) & 63) == 0) { downA = downB; downWA = downWB; }
            un |= uw & chunkBits;  // U is carried over unchanged
            {   // the band below still needs this stretch of the last row: lanes 0..15 copy one column each
                const uint32_t dL = (uint32_t)__builtin_amdgcn_readlane((int)dw, (int)L), uL = (uint32_t)__builtin_amdgcn_readlane((int)uw, (int)L);
                const uint32_t xpk = xp0 + lane;
                const int64_t xk = (int64_t)xpk - L;
                if (xpk <= xp1 && xk >= 1 && xk <= (int64_t)C) {
                    handOut[(uint32_t)xk % kHandWC] = ring[L * kCreepPitch + (xpk & (kCreepRingW - 1))];
                    handOutW[(uint32_t)xk % kHandWC] = ((dL >> (xpk & 31)) & 1u) ? 2 : ((uL >> (xpk & 31)) & 1u);
                }
            }
            prevRes = ringRow[xp1 & (kCreepRingW - 1)];
            prevW = ((dw >> (xp1 & 31)) & 1u) ? swf : (float)((uw >> (xp1 & 31)) & 1u);
            prevRight = ringRow[(xp1 + 1) & (kCreepRingW - 1)];
            continue;
        }
        if (interior(c) && xpc > (uint32_t)kWave) {
            // ---- every lane is at an interior cell with x >= 2: unrolled, no range tests, mask bits as (kCreepCh + 1)-bit windows
            const uint32_t half = xpc & kCreepCh;
            float* rc = ringRow + half;
            const float* rb = ringBelow + half;
            const uint32_t rNext = (half ^ kCreepCh);
            const uint32_t sh0 = xpc & 31, up0 = xpc & 63;
            const uint32_t kSwitch = (L - xpc) & 63;
            const bool switches = kSwitch < (uint32_t)kCreepCh;
            const int dBase = (int)((xpc - L) & 63);
            // bit k: the cell of step k, bit k + 1: its right neighbour (own row) / the cell below (row of lane + 1)
            // (kCreepCh + 1)-bit windows of the word pairs, as 64-bit values: the right neighbour of the chunk's last column is bit kCreepCh
            const uint64_t d17 = (((uint64_t)dwN << 32) | dw) >> sh0, u17 = (((uint64_t)uwN << 32) | uw) >> sh0;
            const uint64_t dd17 = (((uint64_t)ddwN << 32) | ddw) >> sh0, du17 = (((uint64_t)duwN << 32) | duw) >> sh0;
            const uint32_t h16 = hw >> sh0;
            uint32_t newBits = 0;
            // the windows as two 32-bit halves: bit tests at compile-time positions stay 32-bit operations
            const uint32_t dLo = (uint32_t)d17, dHi = (uint32_t)(d17 >> 32), uLo = (uint32_t)u17, uHi = (uint32_t)(u17 >> 32);
            const uint32_t ddLo = (uint32_t)dd17, ddHi = (uint32_t)(dd17 >> 32), duLo = (uint32_t)du17, duHi = (uint32_t)(du17 >> 32);
            auto bit = [](uint32_t lo, uint32_t hi, int i) -> bool { return i < 32 ? ((lo >> i) & 1u) != 0 : ((hi >> (i - 32)) & 1u) != 0; };
#pragma unroll
            for (int k = 0; k < kCreepCh; ++k) {
                const bool cD = bit(dLo, dHi, k), cU = bit(uLo, uHi, k), cH = (h16 >> k) & 1u;
                const float wr = bit(dLo, dHi, k + 1) ? swf : (bit(uLo, uHi, k + 1) ? 1.f : 0.f);
                float wd = bit(ddLo, ddHi, k + 1) ? swf : (bit(duLo, duHi, k + 1) ? 1.f : 0.f);
                const float right = (k < kCreepCh - 1) ? rc[k + 1] : ringRow[rNext];
                float down = (k < kCreepCh - 1) ? rb[k + 1] : ringBelow[rNext];
                const float center = prevRight;
                const float up = lane_from_above_or(prevRes, lane_value(upCur, (int)(up0 + k)));
                const float wu = lane_from_above_or(prevW, lane_value(upWCur, (int)(up0 + k)));
                const bool after = switches && (uint32_t)k >= kSwitch;
                const float dsel = after ? downB : downA, dwsel = after ? downWB : downWA;
                const float downLast = lane_value(dsel, (dBase + k) & 63), wdLast = lane_value(dwsel, (dBase + k) & 63);
                if (lane == L) { down = downLast; wd = wdLast; }
                const float wsum = ((wr + prevW) + wd) + wu;                                        // :1445
                const bool act = !cD && !cH && wsum != 0.f;                                         // :1443, :1446
                float v = center + (((wr * right + prevW * prevRes) + wd * down) + wu * up);        // :1451
                v = v / (1.f + wsum);                                                               // :1452
                const float res = act ? v : center;
                const bool newU = cU || act;
                rc[k] = res;
                if (act) changed = 1;
                newBits |= (newU ? 1u : 0u) << k;
                prevRes = res;
                prevW = cD ? swf : (newU ? 1.f : 0.f);
                prevRight = right;
            }
            if (switches) { downA = downB; downWA = downWB; }
            un |= newBits << sh0;
            {
                const uint32_t dL = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)d17, (int)L), nL = (uint32_t)__builtin_amdgcn_readlane((int)newBits, (int)L);
                if (lane < (uint32_t)kCreepCh) {
                    const uint32_t xk = xpc + lane - L;
                    handOut[xk % kHandWC] = ring[L * kCreepPitch + ((xpc + lane) & (kCreepRingW - 1))];
                    handOutW[xk % kHandWC] = ((dL >> lane) & 1u) ? 2 : ((nL >> lane) & 1u);
                }
            }
            continue;
        }
        for (uint32_t xp = xp0; xp <= xp1; ++xp) {
            if (xp > L && ((xp - L) & 63) == 0) { downA = downB; downWA = downWB; }
            const int64_t x = (int64_t)xp - lane;
            const bool inRange = rowValid && x >= 1 && x <= (int64_t)C;
            const uint32_t sh = xp & 31;
            // bit 0: this cell, bit 1: the cell to the right (own row) / the cell below (row of lane + 1)
            const uint32_t dPair = __builtin_amdgcn_alignbit(dwN, dw, sh), uPair = __builtin_amdgcn_alignbit(uwN, uw, sh);
            const uint32_t ddPair = __builtin_amdgcn_alignbit(ddwN, ddw, sh), duPair = __builtin_amdgcn_alignbit(duwN, duw, sh);
            const bool cD = dPair & 1u, cU = uPair & 1u, cH = (hw >> sh) & 1u;
            const float wr = (dPair & 2u) ? swf : ((uPair & 2u) ? 1.f : 0.f);
            float wd = (ddPair & 2u) ? swf : ((duPair & 2u) ? 1.f : 0.f);
            const uint32_t rp = (xp + 1) & (kCreepRingW - 1);
            const float right = ringRow[rp];
            float down = ringBelow[rp];
            const float center = prevRight;
            const float up = lane_from_above_or(prevRes, lane_value(upCur, (int)(xp & 63)));
            const float wu = lane_from_above_or(prevW, lane_value(upWCur, (int)(xp & 63)));
            const int dIdx = (int)((xp >= L) ? ((xp - L) & 63) : 0);
            const float downLast = lane_value(downA, dIdx), wdLast = lane_value(downWA, dIdx);
            if (lane == L) { down = downLast; wd = wdLast; }
            const float left = (x == 1) ? left0 : prevRes;
            const float wl = (x == 1) ? wLeft0 : prevW;
            const float wsum = ((wr + wl) + wd) + wu;                          // :1445, small integers: exact
            const bool act = inRange && !cD && !cH && wsum != 0.f;             // :1443, :1446
            float v = center + (((wr * right + wl * left) + wd * down) + wu * up);  // :1451
            v = v / (1.f + wsum);                                              // :1452
            const float res = act ? v : center;
            const bool newU = cU || act;
            if (inRange) {
                if (act) { ringRow[xp & (kCreepRingW - 1)] = res; changed = 1; }
                if (lane == L) {
                    handOut[(uint32_t)x % kHandWC] = res;
                    handOutW[(uint32_t)x % kHandWC] = cD ? 2 : (newU ? 1 : 0);
                }
            }
            un |= (newU ? 1u : 0u) << sh;
            prevRes = res;
            prevW = cD ? swf : (newU ? 1.f : 0.f);
            prevRight = right;
        }
    }
    flush_read(nChunks - 1);
    flush_store(nChunks - 1);
    if (rowValid) store_u((nChunks - 1) / kCreepChunksPerWord, un);
    if (outGlobal) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
        if (MULTI && outGlobal) __hip_atomic_store(&mg.flags[b], C + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lds_publish(&hand.produced[slotOut], hand_tag(b, C + 1));
    }
}

// ---- what the two systolic kernels share around creep_band.  The dynamic LDS: the waves' rings [waves][64][pitch] floats, then the
// hand-off's values, weight codes and counters (kCreepLdsBytes is the same sum for the host).  `ring` receives the calling wave's ring.
__device__ __forceinline__ HandoffC creep_carve(float* smem, float*& ring)
{
    HandoffC hand;
    hand.data = smem + kCreepWaves * kWave * kCreepPitch;
    hand.wcode = reinterpret_cast<unsigned char*>(hand.data + kCreepWaves * 2 * kHandWC);
    hand.produced = reinterpret_cast<unsigned int*>(hand.wcode + kCreepWaves * 2 * kHandWC);
    hand.consumed = hand.produced + kCreepWaves * 2;
    ring = smem + (threadIdx.x / kWave) * kWave * kCreepPitch;
    return hand;
}
constexpr size_t kCreepLdsBytes = (size_t)kCreepWaves * kWave * kCreepPitch * sizeof(float) + (size_t)kCreepWaves * 2 * kHandWC * (sizeof(float) + 1) +
                                  (size_t)kCreepWaves * 4 * sizeof(unsigned int);

// one slice of the batch as the sweeps see it; sum, first guess and the D mask were made by fill_stats_kernel / first_guess_kernel
struct CreepSlice {
    float* f;
    const uint32_t* maskD;
    uint32_t* maskU;
    size_t maskWords;
    uint32_t nx, ny, mws, gens, nBands, repeat;
    int setWeight;
    float swf;
    unsigned long long bound;  // the loop's bound (:1430)
    bool skip;                 // :1384-1386, :1515
};
__device__ __forceinline__ CreepSlice creep_slice(const CreepV2Args& a, uint32_t slice)
{
    CreepSlice s;
    s.nx = a.nx;
    s.ny = a.ny;
    s.mws = a.mws;
    s.gens = a.gens;
    s.maskWords = (size_t)a.ny * a.mws;
    s.f = a.field + (size_t)slice * ((size_t)a.nx * a.ny);
    s.maskD = a.maskD + (size_t)slice * s.maskWords;
    s.maskU = a.maskU + (size_t)slice * a.gens * s.maskWords;
    const SliceStats* st = a.stats + slice;
    s.skip = st->skip != 0;
    s.bound = st->sweepBound;
    s.repeat = a.repeat;
    s.setWeight = a.setWeight;
    s.swf = (float)a.setWeight;
    s.nBands = (a.ny - 2 + kWave - 1) / kWave;
    return s;
}

// sweep l over the interior: bands firstBand, firstBand + bandStride, ... by the calling wave
template <bool MULTI>
__device__ __forceinline__ void creep_sweep(const CreepSlice& s, unsigned long long l, float* ring, HandoffC hand, uint32_t firstBand,
                                            uint32_t bandStride, bool skipIdle, int& mine, const MultiWg& mg)
{
    if (threadIdx.x < kCreepWaves * 2) { hand.produced[threadIdx.x] = 0; hand.consumed[threadIdx.x] = 0; }
    __syncthreads();
    const uint32_t* uOld = s.maskU + (size_t)((l - 1) % s.gens) * s.maskWords;
    const uint32_t* uHist = (l > s.repeat) ? s.maskU + (size_t)((l - s.repeat) % s.gens) * s.maskWords : nullptr;
    uint32_t* uNew = s.maskU + (size_t)(l % s.gens) * s.maskWords;
    for (uint32_t b = firstBand; b < s.nBands; b += bandStride)
        creep_band<MULTI>(s.f, s.maskD, uOld, uHist, uNew, ring, hand, b, s.nx, s.ny, s.mws, s.swf, skipIdle, mine, mg);
}

// borders (:1464-1489) after l sweeps, by one workgroup: undefined border cells have r = 0 < repeat in every round, defined ones
// never change
__device__ __forceinline__ void creep_borders(const CreepSlice& s, unsigned long long l)
{
    float* f = s.f;
    const uint32_t* maskD = s.maskD;
    const uint32_t nx = s.nx, mws = s.mws, nxm1 = s.nx - 1, nym1 = s.ny - 1;
    const int setWeight = s.setWeight;
    const uint32_t* uFin = s.maskU + (size_t)(l % s.gens) * s.maskWords;
    auto defined = [&](uint32_t y, uint32_t x) -> bool {
        const uint32_t sk = (y == 0 || y == nym1) ? 0u : ((y - 1) & (kWave - 1));
        return (maskD[(size_t)y * mws + ((x + sk) >> 5)] >> ((x + sk) & 31)) & 1u;
    };
    auto w_interior = [&](uint32_t y, uint32_t x) -> int {  // final weight of an interior cell
        const uint32_t sk = (y - 1) & (kWave - 1);
        if (defined(y, x)) return setWeight;
        return (uFin[(size_t)y * mws + ((x + sk) >> 5)] >> ((x + sk) & 31)) & 1u;
    };
    for (uint32_t k = 0; k < s.repeat; ++k) {
        for (uint32_t y = 1 + threadIdx.x; y < nym1; y += kCreepThreads) {
            const size_t row = (size_t)y * nx;
            if (!defined(y, 0)) {
                const int wn = w_interior(y, 1);
                f[row] += f[row + 1] * wn;
                f[row] /= (float)(1 + wn);
            }
            if (!defined(y, nxm1)) {
                const int wn = w_interior(y, nx - 2);
                f[row + nxm1] += f[row + nx - 2] * wn;
                f[row + nxm1] /= (float)(1 + wn);
            }
        }
        __syncthreads();
        for (uint32_t x = threadIdx.x; x < nx; x += kCreepThreads) {
            const size_t bo = (size_t)nym1 * nx + x;
            const bool edge = (x == 0 || x == nxm1);  // the neighbour is a border cell of the column loop above: w = 1 if it was undefined
            if (!defined(0, x)) {
                const int wn = edge ? (defined(1, x) ? setWeight : 1) : w_interior(1, x);
                f[x] += f[nx + x] * wn;
                f[x] /= (float)(1 + wn);
            }
            if (!defined(nym1, x)) {
                const int wn = edge ? (defined(nym1 - 1, x) ? setWeight : 1) : w_interior(nym1 - 1, x);
                f[bo] += f[bo - nx] * wn;
                f[bo] /= (float)(1 + wn);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kCreepThreads) creepfill_kernel_v2(CreepV2Args a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* ring;
    const HandoffC hand = creep_carve(smem, ring);
    const CreepSlice s = creep_slice(a, blockIdx.x);
    if (s.skip) return;
    unsigned long long l = 0;
    int changedInLoop = 1;
    while (s.repeat > 0 && changedInLoop && l < s.bound) {  // :1430 (nothing has r < repeat when repeat is 0)
        l++;
        int mine = 0;
        creep_sweep<false>(s, l, ring, hand, threadIdx.x / kWave, kCreepWaves, a.skipIdle != 0, mine, MultiWg{0u, 1u, 0u, nullptr, a.error});
        changedInLoop = __syncthreads_or(mine);
    }
    creep_borders(s, l);
}

// The sweeps of creepfill_kernel_v2 with the bands of a slice dealt to a.groups workgroups (MultiWg, fill2d_kernel_v3); the
// border rounds that follow the sweeps are little work and stay with the slice's first workgroup.
__global__ void __launch_bounds__(kCreepThreads) creepfill_kernel_v3(CreepV2Args a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* ring;
    const HandoffC hand = creep_carve(smem, ring);
    const uint32_t G = a.groups;
    const uint32_t slice = (blockIdx.x % kXcds) + kXcds * (blockIdx.x / (kXcds * G));
    const uint32_t g = (blockIdx.x / kXcds) % G;
    if (slice >= a.nz) return;
    const CreepSlice s = creep_slice(a, slice);
    unsigned int* sync = a.sync + (size_t)slice * a.syncStride;
    const MultiWg mg{g, G, 0u, sync + 4, a.error};
    if (s.skip) return;
    unsigned long long l = 0;
    unsigned int barriers = 0;
    int changedInLoop = 1;
    while (s.repeat > 0 && changedInLoop && l < s.bound) {  // :1430
        l++;
        int mine = 0;
        creep_sweep<true>(s, l, ring, hand, g * kCreepWaves + threadIdx.x / kWave, G * kCreepWaves, a.skipIdle != 0, mine, mg);
        unsigned int* changedWord = sync + 1 + (unsigned int)(l % 3);
        if (__syncthreads_or(mine) && threadIdx.x == 0) __hip_atomic_fetch_or(changedWord, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        slice_barrier(sync, ++barriers * G, a.error);
        if (launch_failed(a.error)) return;
        changedInLoop = __hip_atomic_load(changedWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        // the word of the sweep after next (nobody adds to it before the next barrier, which this workgroup has yet to reach),
        // and this workgroup's progress words for the next sweep
        if (g == 0 && threadIdx.x == 0) __hip_atomic_store(sync + 1 + (unsigned int)((l + 2) % 3), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (uint32_t b = g * kCreepWaves + kCreepWaves - 1 + threadIdx.x * G * kCreepWaves; b < s.nBands; b += kCreepThreads * G * kCreepWaves)
            __hip_atomic_store(mg.flags + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // everything the other workgroups wrote is visible behind the last barrier
    if (g == 0) creep_borders(s, l);
}

}  // namespace

// one run of the sweeps over whole slices [nz][ny][nx]; d_defaults (device, per slice) replaces the first guess
void run_creepfill_whole(size_t nx, size_t ny, size_t nz, float* d_field, bool useDefault, float defaultVal,
                         unsigned short repeat, char setWeight, size_t* h_nChanged, hipStream_t stream, const double* d_defaults,
                         const unsigned long long* d_bounds)
{
    if (nx * ny == 0 || nz == 0) return;  // :1380
    FA_REQUIRE(nx <= 0x7FFFFFFFu && ny <= 0x7FFFFFFFu && nz <= 0x7FFFFFFFu, "creepfill: slice too large");
    DeviceArray<SliceStats> stats(nz);
    FA_HIP(hipMemsetAsync(stats.get(), 0, nz * sizeof(SliceStats), stream));
    const char* what = useDefault ? "creepfillval2d" : "creepfill2d";
    const uint32_t mws = fill_mask_words(nx);
    const size_t gens = (size_t)repeat + 1;
    const size_t uWords = nz * gens * ny * mws;
    // the systolic kernel keeps repeat + 1 generations of the "updated" mask; very long repeats take the counter kernel
    if (tuning("CREEP_V2", 1) != 0 && systolic_fits(nx, ny) && setWeight >= 0 && uWords * 4 <= ((size_t)8 << 30)) {
        const size_t nBands = fill_bands(ny);
        DeviceArray<uint32_t> maskD(nz * ny * mws), maskU(uWords);
        FA_HIP(hipMemsetAsync(maskU.get(), 0, uWords * sizeof(uint32_t), stream));
        CreepV2Args a{};
        a.field = d_field;
        a.maskD = maskD.get();
        a.maskU = maskU.get();
        a.stats = stats.get();
        a.nx = (uint32_t)nx;
        a.ny = (uint32_t)ny;
        a.mws = mws;
        a.gens = (uint32_t)gens;
        a.useDefault = useDefault ? 1 : 0;
        a.defaultVal = defaultVal;
        a.repeat = repeat;
        a.setWeight = (int)setWeight;
        a.sumAlgo = tuning("SUM_ALGO", 1);
        a.skipIdle = tuning("CREEP_SKIP", 1);
        launch_fill_prologue(true, d_field, stats.get(), nx, ny, nz, maskD.get(), mws, nullptr, nullptr, false, useDefault, defaultVal, 0.f, stream, d_defaults, d_bounds);
        const DeviceArray<unsigned int> error = cleared_words(1, stream);
        a.error = error.get();
        // small batches: the bands of a slice on several workgroups (groups_per_slice)
        const size_t groups = groups_per_slice(nBands, (size_t)kCreepWaves, nz);
        bool launched = false;
        DeviceArray<unsigned int> sync;
        if (groups > 1) {
            sync = multi_sync_words(a, nBands, groups, nz, stream);
            launched = launch_multi(reinterpret_cast<const void*>(&creepfill_kernel_v3), groups, nz, kCreepThreads, &a, kCreepLdsBytes, stream);
        }
        if (!launched) launch_single(reinterpret_cast<const void*>(&creepfill_kernel_v2), nz, kCreepThreads, &a, kCreepLdsBytes, stream);
        finish_systolic(error, stats, nz, h_nChanged, stream, what);
        return;
    }
    DeviceArray<signed char> w(nx * ny * nz);
    DeviceArray<unsigned short> r(nx * ny * nz);
    CreepArgs a{};
    a.field = d_field;
    a.w = w.get();
    a.r = r.get();
    a.stats = stats.get();
    a.nx = (uint32_t)nx;
    a.ny = (uint32_t)ny;
    a.useDefault = useDefault ? 1 : 0;
    a.defaultVal = defaultVal;
    a.repeat = repeat;
    a.setWeight = (signed char)setWeight;
    a.sumAlgo = tuning("SUM_ALGO", 1);
    a.defaults = d_defaults;
    a.bounds = d_bounds;
    creepfill_kernel<<<dim3((uint32_t)nz), kFillBlock, 0, stream>>>(a);
    FA_HIP(hipGetLastError());
    collect_stats(stats, nz, h_nChanged, stream, what);
}

}  // namespace fimex_amd
