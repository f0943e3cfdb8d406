// In-place 2-D fills (SOR Laplace fill and creep fill) for gfx950.
//
// Replaces mifi_fill2d_f (src/interpolation.c:1246-1376) and mifi_creepfill2d_f /
// mifi_creepfillval2d_f (:1378-1537) as driven slice by slice by processArray_
// (src/CDMInterpolator.cc:136-159).
//
// Both are Gauss-Seidel sweeps in place: cell (x, y) sees the already updated (x-1, y) and
// (x, y-1) and the not yet updated (x+1, y) and (x, y+1).  Any other order changes the result, so
// the sweep is executed as an anti-diagonal wavefront: all cells with x + y = d are independent
// once diagonal d-1 is done.  One workgroup owns one slice (slices are independent, which is where
// the chip-wide parallelism comes from) and steps through the diagonals with a workgroup barrier
// between them.  The sums that feed the first guess (mean, mean absolute deviation) are
// accumulated in the reference's scan order in double, by one wave reading LDS-staged tiles, so
// the first guess is bit-identical too.
//
// This file: the SOR Laplace fill over whole slices; creepfill.hip: the creep fills; fill_rects.hip: both by rectangles.
#include "fill_prologue.hpp"
#include "fill_sync.hpp"

#include <algorithm>
#include <cstdio>

namespace fimex_amd {

namespace {

// ---------------------------------------------------------------------------------- fill2d
struct Fill2dArgs {
    float* field;
    float* w;           // workspace, one float per cell
    SliceStats* stats;  // per slice
    uint32_t nx, ny;
    float relaxCrit, corrEff;
    unsigned long long maxLoop;
    int sumAlgo;
};

__global__ void __launch_bounds__(kFillBlock) fill2d_kernel(Fill2dArgs a)
{
    __shared__ __align__(16) double lds[2 * kSumTile];
    __shared__ double shAverage, shCrit;
    __shared__ unsigned long long shUndef;
    const uint32_t nx = a.nx, ny = a.ny;
    const size_t total = (size_t)nx * ny;
    float* f = a.field + (size_t)blockIdx.x * total;
    float* w = a.w + (size_t)blockIdx.x * total;
    SliceStats* st = a.stats + blockIdx.x;

    unsigned long long nUndef = 0;
    const double sum = scan_order_sum(f, total, 0, 0., lds, &nUndef, a.sumAlgo);
    if (threadIdx.x == 0) {
        shUndef = nUndef;
        const unsigned long long nDef = total - nUndef;
        shAverage = (nDef != 0) ? sum / (double)nDef : 0.;  // :1281
        st->nUndef = nUndef;
        st->status = 1;
    }
    __syncthreads();
    nUndef = shUndef;
    const unsigned long long nDef = total - nUndef;
    if (nDef == 0 || nUndef == 0) return;  // nothing to do, :1266-1268
    if (nx < 2 || ny < 2) { if (threadIdx.x == 0) st->status = -1; return; }  // the reference reads out of bounds here
    const double average = shAverage;

    const double dev = scan_order_sum(f, total, 1, average, lds, nullptr, a.sumAlgo);
    if (threadIdx.x == 0) shCrit = (double)a.relaxCrit * (dev / (double)nDef);  // :1300-1302
    __syncthreads();
    const double crit = shCrit;

    const uint32_t nxm1 = nx - 1, nym1 = ny - 1;
    for (size_t i = threadIdx.x; i < total; i += kFillBlock) {  // :1288-1299 and :1311-1315
        const uint32_t x = (uint32_t)(i % nx), y = (uint32_t)(i / nx);
        float wi = 0.f;
        if (isnan(f[i])) {
            f[i] = (float)average;
            wi = 1.f;
        }
        if (x >= 1 && x < nxm1 && y >= 1 && y < nym1) wi *= a.corrEff;
        w[i] = wi;
    }
    __syncthreads();

    const float crtest = (float)(crit * a.corrEff);  // :1341
    // interior cells 1 <= x <= nx-2, 1 <= y <= ny-2; diagonal d = x + y runs 2 .. nx+ny-4
    const bool hasInterior = nx > 2 && ny > 2;
    for (unsigned long long n = 0; n < a.maxLoop; ++n) {
        const bool check = (n < (a.maxLoop - 5)) && (n % 10 == 0);  // :1339-1340, unsigned like the reference
        int bad = 0;
        if (hasInterior) {
            const uint32_t dLast = (nx - 2) + (ny - 2);
            for (uint32_t d = 2; d <= dLast; ++d) {
                const uint32_t xlo = (d > (ny - 2)) ? d - (ny - 2) : 1;
                const uint32_t xhi = (d - 1 < nx - 2) ? d - 1 : nx - 2;
                for (uint32_t x = xlo + threadIdx.x; x <= xhi; x += kFillBlock) {
                    const size_t p = (size_t)(d - x) * nx + x;
                    const float fc = f[p];
                    const float e = (float)((double)(f[p + 1] + f[p - 1] + f[p + nx] + f[p - nx]) * 0.25 - (double)fc);  // :1332
                    const float wp = w[p];
                    f[p] = fc + e * wp;  // :1333
                    if (check && (fabsf(e * wp) > crtest)) bad = 1;  // :1349
                }
                __syncthreads();
            }
        }
        if (check) {
            if (!__syncthreads_or(bad)) return;  // converged, :1355-1359 (before the border pass)
        }
        for (uint32_t y = 1 + threadIdx.x; y < nym1; y += kFillBlock) {  // :1363-1366
            const size_t r = (size_t)y * nx;
            f[r] += (f[r + 1] - f[r]) * w[r];
            f[r + nxm1] += (f[r + nx - 2] - f[r + nxm1]) * w[r + nxm1];
        }
        __syncthreads();
        for (uint32_t x = threadIdx.x; x < nx; x += kFillBlock) {  // :1367-1370
            const size_t b = (size_t)nym1 * nx + x;
            f[x] += (f[nx + x] - f[x]) * w[x];
            f[b] += (f[b - nx] - f[b]) * w[b];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ fill2d, systolic version
// The anti-diagonal wavefront above pays one workgroup barrier per diagonal (nx + ny of them per sweep).  Here the
// same Gauss-Seidel order is kept with (almost) no barriers: a wave owns a band of 64 consecutive rows, lane l owns
// row y0 + l and walks it left to right, one column per step, l steps behind the lane above it:
//     step s: lane l updates column x = 1 + s - l.
// Then everything a cell needs is one step old in a neighbouring lane or in the lane itself:
//     left  f_new(x-1, y)   own result of the previous step
//     up    f_new(x, y-1)   the previous step's result of lane l-1            (wave shift by one lane)
//     right f_old(x+1, y)   own row, next column                              (LDS ring, see below)
//     down  f_old(x, y+1)   what lane l+1 reads as its "right" in this step   (wave shift by one lane)
// Rows are streamed through a per-wave LDS ring in SKEWED columns x' = x + l, so that all lanes are at the same
// x' = 1 + s: 16-column chunks of all 64 rows are loaded two chunks ahead with coalesced row-segment loads, results
// overwrite the ring in place and finished chunks are flushed with coalesced stores.  The NaN mask that selects the
// weight is kept as bits, one word per 32 skewed columns and row, so every lane switches words in the same step.
// Bands are pipelined over the 16 waves of the workgroup: the first lane of band b needs the last row of band b-1,
// published through an LDS progress counter (release/acquire at workgroup scope; all waves of a workgroup share
// the CU's L1).  One workgroup barrier per sweep remains (border pass, convergence test).
// Two geometries are built: 16 waves on 16-column chunks (more bands in flight, the faster first-guess sums: small
// batches and calls that leave after a few sweeps) and 8 waves on 32-column chunks (whole 128-byte row pieces per
// memory event: large batches, where the chunk traffic of all slices meets in L2).  FILL_GEOMETRY(CH, WAVES) puts the
// derived constants into the scope of a function template.
#define FILL_GEOMETRY(CH, WAVES)                                                                                        \
    constexpr int kCh = (CH);                  /* skewed columns per chunk: one global-memory event per chunk */      \
    constexpr int kV2Waves = (WAVES);                                                                                   \
    constexpr int kV2Threads = kV2Waves * kWave;                                                                        \
    constexpr int kRowsPerIt = kWave / kCh;    /* rows one wave-wide load / store of a chunk covers */                \
    constexpr int kChunksPerWord = 32 / kCh;   /* chunks per 32-column mask word */                                   \
    constexpr int kRingW = 2 * kCh;            /* ring width (two chunks) */                                          \
    constexpr int kPitch = kRingW + 1;         /* conflict-free: bank = (lane + x') mod 32 */                         \
    (void)kV2Threads; (void)kRowsPerIt; (void)kChunksPerWord; (void)kRingW; (void)kPitch

struct Fill2dV2Args {
    float* field;
    uint32_t* maskS;          // [nz][ny][mws] skewed NaN-mask words of the interior rows
    unsigned char* mbRows;    // [nz][2][nx] NaN mask of row 0 and row ny-1
    unsigned char* mbCols;    // [nz][2][ny] NaN mask of column 0 and column nx-1
    SliceStats* stats;
    uint32_t nx, ny, mws;
    float relaxCrit, corrEff;
    unsigned long long maxLoop;
    int sumAlgo;
    unsigned int* error;      // one word per launch: set by a wait that gave up (see MultiWg)
    // several workgroups per slice (fill2d_kernel_v3): per slice [0] barrier counter, [1..2] "not converged" by parity of the
    // check, [4 .. 4 + bands) progress words of the bands whose hand-off crosses workgroups
    unsigned int* sync;
    uint32_t syncStride, groups, nz;
    uint32_t experiment;
    unsigned long long* prof;
    // > 0 (fill2d by rectangles): slices i, i + couple, i + 2 couple, ... are rectangles of ONE field and end their sweeps together,
    // by the criterion over all of them (:1338-1359); word [3] of slice i % couple's sync words is their barrier counter
    uint32_t couple;
};

// e = (f1 + f2 + f3 + f4) * 0.25 - f of interpolation.c:1332: the float sum times the double constant, minus the float
// as double, rounded to float.  One fused multiply-add gives the same bits with a third of the dependent operations: the
// product is exact either way, and the difference of two floats either fits a double exactly (exponents at most 29
// apart: then both paths round the same exact value once) or is dominated by the larger one so completely that both
// round to it; infinities and NaN take the same way through both.  (-ffp-contract=off forbids the compiler to fuse on
// its own; this fusion is deliberate.)  tests/test_gpu_parity.py::test_sor_error_is_the_reference_expression walks the
// exponent gaps.
__device__ __forceinline__ float sor_error(float sum, float center) { return __builtin_fmaf(sum, 0.25f, -center); }

// one band of one sweep, executed by one wave.  Global memory is touched only in the "event" between two 16-step
// chunks: loads issued there are consumed one event later, stores are never waited for (the sweep ends with a
// workgroup barrier); the 16 steps in between run on registers and LDS.
// CHECK: a sweep that also tests convergence (every tenth, :1339-1360); the other nine carry no trace of the test
template <int CH, int WAVES, bool CHECK, bool MULTI = false>
__device__ void fill2d_band(float* __restrict__ f, const uint32_t* __restrict__ maskS, float* ring, Handoff hand, uint32_t b,
                            uint32_t nx, uint32_t ny, uint32_t mws, float wInt, float wZero, float crtest, int& bad, MultiWg mg)
{
    FILL_GEOMETRY(CH, WAVES);
    constexpr bool check = CHECK;
    using rsrc_t = __amdgpu_buffer_rsrc_t;
    // The band is the same for the whole wave, but it derives from threadIdx: said explicitly, the buffer descriptor of the
    // band's rows and every "is this the band that hands over through global memory" test stay in scalar registers.  Left to
    // the compiler, each of the 32 buffer loads and stores of an event sat in a loop over the lanes' (identical) descriptors
    // and each store behind a divergent branch: 7 000 cycles per event against 1 900 for the sixteen steps between two events.
    b = __builtin_amdgcn_readfirstlane(b);
    {   // (where this function is not inlined its arguments arrive in vector registers: the same for the slice's pointers)
        auto uniform = [](auto* ptr) {
            const uint64_t v = reinterpret_cast<uint64_t>(ptr);
            const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
            return reinterpret_cast<decltype(ptr)>(((uint64_t)hi << 32) | lo);
        };
        f = uniform(f);
        maskS = uniform(maskS);
        nx = __builtin_amdgcn_readfirstlane(nx);
        ny = __builtin_amdgcn_readfirstlane(ny);
        mws = __builtin_amdgcn_readfirstlane(mws);
    }
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t y0 = 1 + kWave * b;
    const uint32_t nrow = min((uint32_t)kWave, (ny - 1) - y0);  // rows y0 .. y0 + nrow - 1 <= ny - 2
    const uint32_t L = nrow - 1;                                 // last lane with a row
    const bool rowValid = lane < nrow;
    const uint32_t y = y0 + min(lane, L);
    const uint32_t C = nx - 2;                                   // interior columns 1 .. C
    const uint32_t xpEnd = C + L;                                // last skewed column with work
    float* ringRow = ring + lane * kPitch;
    // the ring's row below lane L (row nrow <= 64) is virtual: the first row of the band below, written chunk by chunk from
    // the 64-column blocks downA / downB, so that the last lane reads its "down" like every other lane
    const float* ringBelow = ring + min(lane + 1, L + 1) * kPitch;
    float* ringVirtual = ring + (L + 1) * kPitch;
    const float left0 = f[(size_t)y * nx];                       // border column 0, not touched by the sweep
    const uint32_t* mrow = maskS + (size_t)y * mws;
    // the band's rows plus the row above and the row below as one buffer: masked lanes use an out-of-range offset
    // (loads return 0, stores are dropped), so every memory instruction is issued unconditionally
    const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(f + (size_t)(y0 - 1) * nx, 0, (nrow + 2) * nx * 4u, 0x00020000);
    const uint32_t kOob = 0xFFFFFFFFu;
    const bool prof = kTuningBuild && mg.experiment == 4 && mg.prof != nullptr;
    const bool earlyPrefetch = !(kTuningBuild && mg.experiment == 5);  // tuning build, FILL_EXPERIMENT=5: the prefetch after the waits (round 2's order)
    unsigned long long tWait = 0, tFlush = 0;
    // Every W-th boundary (band W-1 -> W, 2W-1 -> 2W, ...) goes through global memory: in one workgroup the wave of band b + 1
    // is still busy with band b + 1 - W there (a bounded LDS window would close a cycle of waiting waves on wide grids), with
    // several workgroups per slice (MULTI) band b + 1 belongs to the next workgroup.  The producer's flush already writes the
    // row; it only has to publish how far its stores have completed.
    const bool hasBelow = y0 + nrow < ny - 1;
    const bool outGlobal = hasBelow && (b % kV2Waves) == kV2Waves - 1;
    const bool inGlobal = b > 0 && (b % kV2Waves) == 0;
    const bool writeThrough = MULTI && outGlobal;  // the band below reads these rows on another CU, maybe another XCD

    // chunk c = skewed columns [c*kCh, c*kCh + kCh) of all 64 rows; lane -> (row kRowsPerIt*it + lane/kCh, column lane%kCh)
    const uint32_t crow = lane / kCh, ccol = lane % kCh;
    float stage[kCh];
    auto chunk_off = [&](uint32_t c, uint32_t it, bool store) -> uint32_t {
        const uint32_t row = kRowsPerIt * it + crow;
        const int64_t x = (int64_t)c * kCh + ccol - row;  // unskewed column
        const bool ok = row < nrow && (store ? (x >= 1 && x <= (int64_t)C) : (x >= 0 && x <= (int64_t)nx - 1));
        return ok ? (uint32_t)(((row + 1) * nx + x) * 4u) : kOob;
    };
    // A chunk is "interior" when every one of its 64 x 16 cells is a cell the sweep updates (all rows of the band exist,
    // 1 <= x <= C for all of them): no per-lane conditions are needed then, and since a lone wave issues roughly one
    // instruction per 8-9 clocks, instructions are what the band's time consists of.  Interior chunks address memory as
    // one per-lane offset plus a scalar offset per row group (buffer soffset) and the LDS ring with immediate offsets.
    auto interior = [&](uint32_t c) -> bool { return nrow == (uint32_t)kWave && c * kCh >= (uint32_t)kWave && c * kCh + kCh - 1 <= C; };
    const uint32_t voffLane = ((crow + 1) * nx + ccol - crow) * 4u;           // row crow, chunk 0, column ccol - crow
    const uint32_t rowStep = (uint32_t)kRowsPerIt * (nx - 1) * 4u;            // next row group: kRowsPerIt rows down, as many columns back
    float* ringLane = ring + crow * kPitch + ccol;
    auto load_chunk = [&](uint32_t c) {
        if (kTuningBuild && mg.experiment == 2) return;  // timing experiment: no chunk loads
        if (interior(c)) {
            const uint32_t s0 = c * kCh * 4u;
#pragma unroll
            for (uint32_t it = 0; it < (uint32_t)kCh; ++it)
                stage[it] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voffLane, s0 + it * rowStep, 0));
            return;
        }
#pragma unroll
        for (uint32_t it = 0; it < (uint32_t)kCh; ++it)
            stage[it] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, chunk_off(c, it, false), 0, 0));
    };
    auto commit_chunk = [&](uint32_t c) {
        float* dst = ringLane + ((c * kCh) & kCh);
#pragma unroll
        for (uint32_t it = 0; it < (uint32_t)kCh; ++it) dst[kRowsPerIt * it * kPitch] = stage[it];
    };
    // The results of a finished chunk leave in two steps: out of the ring into registers (before the ring slot is refilled),
    // and to global memory AFTER the event's loads have been issued.  Vector-memory operations complete in issue order: a load
    // that sits behind sixteen stores is not counted as done before they are, so the wait for the next chunk's data was a wait
    // for this chunk's stores -- 3-4 us per event, which set the pace of every band (measured with the tuning build's cycle
    // counters: 8 400 cycles per event against 1 900 for the sixteen steps between two events).
    float v[kCh];
    auto flush_read = [&](uint32_t c) {
        const float* src = ringLane + ((c * kCh) & kCh);
#pragma unroll
        for (uint32_t it = 0; it < (uint32_t)kCh; ++it) v[it] = src[kRowsPerIt * it * kPitch];
    };
    auto flush_store = [&](uint32_t c) {
        if (kTuningBuild && mg.experiment == 3) return;  // timing experiment: no chunk stores
        if (interior(c)) {
            const uint32_t s0 = c * kCh * 4u;
#pragma unroll
            for (uint32_t it = 0; it < (uint32_t)kCh; ++it) {
                if (writeThrough) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[it]), rs, voffLane, s0 + it * rowStep, 17);
                else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[it]), rs, voffLane, s0 + it * rowStep, 0);
            }
            return;
        }
#pragma unroll
        for (uint32_t it = 0; it < (uint32_t)kCh; ++it) {
            if (writeThrough) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[it]), rs, chunk_off(c, it, true), 0, 17);
            else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[it]), rs, chunk_off(c, it, true), 0, 0);
        }
    };
    auto load_block = [&](uint32_t rowInBuf, uint32_t k) {  // 64 columns of the row above (0) / below (nrow + 1)
        const uint32_t col = 64 * k + lane;
        const uint32_t off = col <= nx - 1 ? (rowInBuf * nx + col) * 4u : kOob;
        // the row above a band whose predecessor runs in another workgroup: written during this sweep, read past L1 and L2
        if (MULTI && inGlobal && rowInBuf == 0) return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 17));
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
    };

    // hand-off slots: mine (towards band b + 1) and the one of band b - 1
    const uint32_t round = kV2Waves * (MULTI ? mg.G : 1u);  // bands between two bands of one wave
    const uint32_t slotOut = (b % kV2Waves) * 2 + ((b / round) & 1);
    const uint32_t slotIn = ((b - 1) % kV2Waves) * 2 + (((b - 1) / round) & 1);  // unused for b == 0
    float* handOut = hand.data + slotOut * kHandW;
    const float* handIn = hand.data + slotIn * kHandW;
    if (lane == 0) {
        __hip_atomic_store(&hand.produced[slotOut], hand_tag(b, 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(&hand.consumed[slotOut], hand_tag(b, 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // The hand-off advances chunk by chunk, not in blocks of 64 columns: band b runs behind band b - 1 by the 63 columns of the
    // skew plus one or two chunks, and these lags add up over all bands of a sweep -- the critical path of a small batch.
    auto wait_above = [&](uint32_t cols) {  // the stores of band b - 1 have completed for columns < cols of its last row
        cols = min(cols, C + 1);
        const unsigned long long t0 = prof ? clock64() : 0;
        if (MULTI) wait_global_at_least(&mg.flags[b - 1], cols + 1, mg.error);
        else wait_lds_at_least(&hand.produced[slotIn], hand_tag(b - 1, cols), mg.error);
        if (prof) tWait += clock64() - t0;
    };
    // columns [xpc, xpc + kCh) of the row above from the LDS hand-off of band b - 1, into lanes (column % 64) of upCur
    auto take_above = [&](uint32_t xpc, float& upCur) {
        const unsigned int need = hand_tag(b - 1, min(xpc + kCh, C + 1));
        // a larger band tag means the producer has finished band b - 1 long ago (its data stay in the other parity slot)
        const unsigned long long t0 = prof ? clock64() : 0;
        wait_lds_at_least(&hand.produced[slotIn], need, mg.error);
        if (prof) tWait += clock64() - t0;
        const float v = handIn[((xpc & ~63u) + lane) % kHandW];
        if (lane - (xpc & 63u) < (uint32_t)kCh) upCur = v;
        if (lane == 0)
            lds_publish(&hand.consumed[slotIn], hand_tag(b - 1, xpc + kCh));
    };

    // ---- prologue: chunks 0 and 1 in LDS, chunk 2 in flight; first blocks and mask words.
    // Registers that receive a load at an event (stage[], upLd, downLd, mwLd) are read only at a LATER event.
    load_chunk(0);
    commit_chunk(0);
    load_chunk(1);
    commit_chunk(1);
    load_chunk(2);
    // row above: lanes (column % 64) of upCur hold the chunk in work; from global memory (row 0, or a band whose predecessor
    // hands over through global memory) the next chunk's block is requested one event ahead into upLd
    float upCur = 0.f, upLd = 0.f;
    const bool fromGlobal = b == 0 || inGlobal;
    if (fromGlobal) {
        if (inGlobal) wait_above(kCh);
        upCur = load_block(0, 0);
        if (inGlobal) wait_above(2 * kCh);
        upLd = load_block(0, kCh >> 6);
    } else take_above(0, upCur);
    float downA = load_block(nrow + 1, 0), downB = downA, downLd = 0.f;  // current / next (landed) / in flight
    uint32_t downIssued = 0;
    bool downLdValid = false;
    uint32_t mw = mrow[0], mwN = mrow[1], mwLd = mrow[2];
    float prevRes = 0.f;
    float prevRight = ringRow[1];  // lane 0 is at column 1 in the first step: its centre is skewed column 1

    const uint32_t nChunks = xpEnd / kCh + 1;
    unsigned long long tEvents = 0, tSteps = 0, tMark = prof ? clock64() : 0;
    for (uint32_t c = 0; c < nChunks; ++c) {
        const uint32_t xpc = c * kCh;
        if (prof) { const unsigned long long t = clock64(); tSteps += t - tMark; tMark = t; }
        if (c > 0) {
            // ---- event at the start of chunk c
            if (outGlobal && xpc > L) {  // stores of the previous event (chunk c - 2) have landed: columns < 16 (c - 1) - L of the last row
                if (!(kTuningBuild && mg.experiment == 1)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0 && xpc - kCh > L) {
                    if (MULTI) __hip_atomic_store(&mg.flags[b], xpc - kCh - L + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else lds_publish(&hand.produced[slotOut], hand_tag(b, xpc - kCh - L));
                }
            }
            // Order matters: vector-memory results come back in issue order, so waiting for a load also waits for every
            // load issued before it.  The small loads (mask word, 64-column blocks of the rows above / below) go first,
            // the 16 loads of the chunk prefetch last: whatever the compiler makes of the small ones, it never has to wait
            // for the prefetch before the next event.
            if ((c % kChunksPerWord) == 0) {      // x' is a multiple of 32: every lane switches mask words now
                mw = mwN;
                mwN = mwLd;
                mwLd = mrow[min(c / kChunksPerWord + 2, mws - 1)];
            }
            // row below: the last lane is at column x' - L
            if (downLdValid) { downB = downLd; downLdValid = false; }
            if (xpc + 2 * kCh > L && ((xpc + 2 * kCh - L) >> 6) > downIssued) {  // block j + 1 is requested two chunks before the last lane
                // reaches it and lands in downB at the next event: after block j has moved on to downA, never skipping one
                ++downIssued;
                downLd = load_block(nrow + 1, downIssued);
                downLdValid = true;
            }
            // row above: lane 0 is at column x'
            if (fromGlobal) {
                if (lane - (xpc & 63u) < (uint32_t)kCh) upCur = upLd;  // this chunk's columns, requested one event ago
                if (inGlobal) wait_above(xpc + 2 * kCh);
                upLd = load_block(0, (xpc + kCh) >> 6);
            }
            flush_read(c - 1);       // results of the chunk just finished: ring -> registers
            commit_chunk(c + 1);     // loaded one event ago, into the ring slot the flush has just read
            // The prefetch of chunk c + 2 goes out as soon as its registers are free -- before the waits on the neighbouring bands
            // below, which may take as long as the 16 steps do: the loads are what the next event waits for.
            if (earlyPrefetch) load_chunk(c + 2);
            // publish how far the last row has got, and do not run more than the hand-off window ahead of the band below
            if (xpc > L && !outGlobal) {
                if (lane == 0)
                    lds_publish(&hand.produced[slotOut], hand_tag(b, xpc - L));
                if (hasBelow) {
                    const unsigned int limit = xpc + kCh - L;  // columns < limit are written during this chunk
                    const unsigned long long t0 = prof ? clock64() : 0;
                    unsigned long long tSpin = 0;
                    for (unsigned int it = 0;; ++it) {
                        const unsigned int cns = lds_observe(&hand.consumed[slotOut]);
                        if (limit <= (cns & 0x7FFFFu) + kHandW) break;
                        __builtin_amdgcn_s_sleep(1);
                        if ((it & 0xFFF) == 0xFFF && (spin_expired(tSpin) || launch_failed(mg.error))) { fail_launch(mg.error, 3); break; }
                    }
                    if (prof) tFlush += clock64() - t0;  // (window waits, counted apart)
                }
            }
            if (!fromGlobal) take_above(xpc, upCur);
            if (!earlyPrefetch) load_chunk(c + 2);       // consumed at the next event
            flush_store(c - 1);      // registers -> global, behind the loads (never waited for)
        }
        if (prof) { const unsigned long long t = clock64(); tEvents += t - tMark; tMark = t; }
        const uint32_t xp0 = max(xpc, 1u), xp1 = min(xpc + kCh - 1, xpEnd);
        if (interior(c) && xpc > (uint32_t)kWave) {
            // ---- every lane is at a cell the sweep updates, at x >= 2: no range tests, "left" is the previous result
            const uint32_t half = xpc & kCh;
            float* rc = ringRow + half;
            const float* rb = ringBelow + half;
            const uint32_t rNext = (half ^ kCh);
            const uint32_t sh0 = xpc & 31, up0 = xpc & 63;
            const uint32_t kSwitch = (L - xpc) & 63;
            const bool switches = kSwitch < (uint32_t)kCh;  // xpc + kSwitch > L holds: xpc >= 64 > L - kSwitch
            const int dBase = (int)((xpc - L) & 63);
            {   // the chunk's kCh values of the row below the band into the virtual ring row (lane j: step j)
                const uint32_t j = lane & (kCh - 1);
                const int src = (int)((dBase + j) & 63);   // (the choice of the block is the reading lane's, not the source lane's)
                const float fromA = __shfl(downA, src), fromB = __shfl(downB, src);  // by all lanes: a shuffle under a divergent branch misses its source lanes
                const float vd = (switches && j >= kSwitch) ? fromB : fromA;
                if (lane < (uint32_t)kCh) ringVirtual[(xpc + 1 + j) & (kRingW - 1)] = vd;
            }
            // Everything a group of 16 steps reads from the ring is read first -- a position is read (as "right" / "down" of
            // the step before) strictly before the step that rewrites it, so the values are the ones the interleaved order saw
            // -- and the results are written after the group's last step: the dependent chain of a step (the lane above's
            // previous result -> sum -> error -> result) then runs on registers, DPP and readlane alone, with no LDS latency
            // in it.  The chain is what a band's time consists of, and the bands' lags add up to a sweep's critical path.
            // (Workgroups of 16 waves have 128 registers per lane and four waves per SIMD to cover the latency: interleaved.)
            constexpr bool kPreload = WAVES <= 8;
            constexpr int kGroup = kPreload ? 16 : 1;
#pragma unroll
            for (int g0 = 0; g0 < kCh; g0 += kGroup) {
                float R[kGroup], D[kGroup], out[kGroup];
#pragma unroll
                for (int q = 0; q < kGroup; ++q) {
                    const int k = g0 + q;
                    R[q] = (k < kCh - 1) ? rc[k + 1] : ringRow[rNext];
                    D[q] = (k < kCh - 1) ? rb[k + 1] : ringBelow[rNext];
                }
#pragma unroll
                for (int q = 0; q < kGroup; ++q) {
                    const int k = g0 + q;
                    const float center = prevRight;
                    const float up = lane_from_above_or(prevRes, lane_value(upCur, (int)(up0 + k)));
                    const float wv = ((mw >> (sh0 + k)) & 1u) ? wInt : wZero;
                    const float e = sor_error(((R[q] + prevRes) + D[q]) + up, center);  // interpolation.c:1332
                    const float res = center + e * wv;                                                           // :1333
                    out[q] = res;
                    prevRes = res;
                    if (check && (fabsf(e * wv) > crtest)) bad = 1;                                              // :1349
                    prevRight = R[q];
                }
#pragma unroll
                for (int q = 0; q < kGroup; ++q) rc[g0 + q] = out[q];
            }
            if (switches) downA = downB;
            if (lane < (uint32_t)kCh) handOut[(xpc + lane - L) % kHandW] = ring[L * kPitch + ((xpc + lane) & (kRingW - 1))];
            continue;
        }
        if (xpc >= 1 && xpc + kCh - 1 <= xpEnd) {
            // ---- a whole chunk: 16 steps unrolled, everything that is the same for all lanes in scalar registers, no
            // branches (inactive lanes rewrite the ring slot with its own value), hand-off copied once at the end
            const uint32_t half = xpc & kCh;                                   // ring half this chunk lives in
            float* rc = ringRow + half;
            const float* rb = ringBelow + half;
            const uint32_t rNext = (half ^ kCh);                               // first column of the other half
            const int x0 = (int)xpc - (int)lane;
            const uint32_t sh0 = xpc & 31, up0 = xpc & 63;
            const uint32_t kSwitch = (L - xpc) & 63;                           // step at which the last lane enters the next 64-column block
            const bool switches = kSwitch < (uint32_t)kCh && xpc + kSwitch > L;
            const int dBase = (int)((xpc - L) & 63);                           // column of the last lane within its block (valid when xpc >= L)
            {   // the virtual ring row, as in the interior path (columns before the last lane's first one are never used)
                const uint32_t j = lane & (kCh - 1);
                const int src = (int)((xpc + j >= L) ? ((dBase + j) & 63) : 0);
                const float fromA = __shfl(downA, src), fromB = __shfl(downB, src);  // by all lanes: a shuffle under a divergent branch misses its source lanes
                const float vd = (switches && j >= kSwitch) ? fromB : fromA;
                if (lane < (uint32_t)kCh) ringVirtual[(xpc + 1 + j) & (kRingW - 1)] = vd;
            }
#pragma unroll
            for (int k = 0; k < kCh; ++k) {
                const int x = x0 + k;
                const bool active = rowValid && x >= 1 && x <= (int)C;
                const float right = (k < kCh - 1) ? rc[k + 1] : ringRow[rNext];
                const float down = (k < kCh - 1) ? rb[k + 1] : ringBelow[rNext];
                const float center = prevRight;
                const float up = lane_from_above_or(prevRes, lane_value(upCur, (int)(up0 + k)));
                const float left = (x == 1) ? left0 : prevRes;
                const float wv = ((mw >> (sh0 + k)) & 1u) ? wInt : wZero;
                const float e = sor_error(((right + left) + down) + up, center);  // interpolation.c:1332
                const float res = active ? center + e * wv : center;                                      // :1333
                rc[k] = res;
                prevRes = res;
                if (check && active && (fabsf(e * wv) > crtest)) bad = 1;                                 // :1349
                prevRight = right;
            }
            if (switches) downA = downB;
            {   // the band below reads its "up" values from the hand-off: lanes 0..15 copy one column of the last row each
                const uint32_t xpk = xpc + lane;
                const int xk = (int)xpk - (int)L;
                if (lane < (uint32_t)kCh && xk >= 1 && xk <= (int)C) handOut[(uint32_t)xk % kHandW] = ring[L * kPitch + (xpk & (kRingW - 1))];
            }
            continue;
        }
        for (uint32_t xp = xp0; xp <= xp1; ++xp) {
            if (xp > L && ((xp - L) & 63) == 0) downA = downB;  // the last lane enters block (x' - L) / 64
            const int64_t x = (int64_t)xp - lane;
            const bool active = rowValid && x >= 1 && x <= (int64_t)C;
            const uint32_t rp = (xp + 1) & (kRingW - 1);
            const float right = ringRow[rp];
            float down = ringBelow[rp];  // f_old(x, y+1): row lane+1 holds column x at its skewed column x' + 1
            const float center = prevRight;
            float up = lane_from_above(prevRes);
            const float upFirst = lane_value(upCur, (int)(xp & 63));
            if (lane == 0) up = upFirst;
            const float downLast = lane_value(downA, (int)((xp >= L) ? ((xp - L) & 63) : 0));
            if (lane == L) down = downLast;
            const float left = (x == 1) ? left0 : prevRes;
            const float wv = ((mw >> (xp & 31)) & 1u) ? wInt : wZero;
            const float e = sor_error(((right + left) + down) + up, center);  // interpolation.c:1332
            const float res = center + e * wv;                                                        // :1333
            if (active) {
                ringRow[xp & (kRingW - 1)] = res;
                prevRes = res;
                if (lane == L) handOut[(uint32_t)x % kHandW] = res;  // the band below reads its "up" values here
                if (check && (fabsf(e * wv) > crtest)) bad = 1;     // :1349
            }
            prevRight = right;
        }
    }
    if (prof && lane == 0) {
        atomicAdd(&mg.prof[0], tEvents);
        atomicAdd(&mg.prof[1], tSteps + (clock64() - tMark));
        atomicAdd(&mg.prof[2], 1ull);
        atomicAdd(&mg.prof[3], tWait);
        atomicAdd(&mg.prof[4], tFlush);
        if (b == 0) { atomicAdd(&mg.prof[5], tEvents); atomicAdd(&mg.prof[6], tSteps); atomicAdd(&mg.prof[7], 1ull); }
    }
    flush_read(nChunks - 1);
    flush_store(nChunks - 1);
    if (outGlobal) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
        if (MULTI && outGlobal) __hip_atomic_store(&mg.flags[b], C + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lds_publish(&hand.produced[slotOut], hand_tag(b, C + 1));
    }
}

// ---- what the two systolic kernels share around fill2d_band.  The dynamic LDS holds the waves' rings, [waves][65][pitch] floats
// (every wave's ring has a 65th row: the row below the band), then the hand-off [waves][2][192] floats and its counters;
// fill2d_lds_bytes is the same sum for the host.  `ring` receives the calling wave's ring.
template <int CH, int WAVES>
__device__ __forceinline__ Handoff fill2d_carve(float* smem, float*& ring)
{
    FILL_GEOMETRY(CH, WAVES);
    Handoff hand;
    hand.data = smem + kV2Waves * (kWave + 1) * kPitch;
    hand.produced = reinterpret_cast<unsigned int*>(hand.data + kV2Waves * 2 * kHandW);
    hand.consumed = hand.produced + kV2Waves * 2;
    ring = smem + (threadIdx.x / kWave) * (kWave + 1) * kPitch;
    return hand;
}

// one slice of the batch as the sweeps see it; sums, first guess and masks were made by fill_stats_kernel / first_guess_kernel
struct Fill2dSlice {
    float* f;
    const uint32_t* maskS;
    const unsigned char *mbTop, *mbBot, *mbLeft, *mbRight;
    uint32_t nx, ny, mws, nBands;
    float wInt, wZero, crtest;
    bool skip;  // :1266-1269 (the same for every workgroup of the slice)
};
__device__ __forceinline__ Fill2dSlice fill2d_slice(const Fill2dV2Args& a, uint32_t slice)
{
    Fill2dSlice s;
    s.nx = a.nx;
    s.ny = a.ny;
    s.mws = a.mws;
    s.f = a.field + (size_t)slice * ((size_t)a.nx * a.ny);
    s.maskS = a.maskS + (size_t)slice * a.ny * a.mws;
    s.mbTop = a.mbRows + (size_t)slice * 2 * a.nx;
    s.mbBot = s.mbTop + a.nx;
    s.mbLeft = a.mbCols + (size_t)slice * 2 * a.ny;
    s.mbRight = s.mbLeft + a.ny;
    const SliceStats* st = a.stats + slice;
    s.skip = st->skip != 0;
    s.wInt = 1.f * a.corrEff;  // :1311-1315
    s.wZero = 0.f * a.corrEff;
    s.crtest = (float)(st->meanAbsDev * a.corrEff);
    s.nBands = (a.ny - 2 + kWave - 1) / kWave;
    return s;
}

// the border pass that ends a sweep: cells first, first + stride, ... of the border columns, barrier(), then of the border rows,
// barrier() -- (threadIdx, threads) and __syncthreads for one workgroup per slice, (g threads + threadIdx, G threads) and the
// slice's barrier for several
template <typename Barrier>
__device__ __forceinline__ void fill2d_borders(const Fill2dSlice& s, uint32_t first, uint32_t stride, Barrier barrier)
{
    float* f = s.f;
    const uint32_t nx = s.nx, nxm1 = s.nx - 1, nym1 = s.ny - 1;
    for (uint32_t y = 1 + first; y < nym1; y += stride) {  // :1363-1366
        const size_t r = (size_t)y * nx;
        const float wl = s.mbLeft[y] ? 1.f : 0.f, wr = s.mbRight[y] ? 1.f : 0.f;
        f[r] += (f[r + 1] - f[r]) * wl;
        f[r + nxm1] += (f[r + nx - 2] - f[r + nxm1]) * wr;
    }
    barrier();
    for (uint32_t x = first; x < nx; x += stride) {  // :1367-1370
        const size_t bo = (size_t)nym1 * nx + x;
        const float wt = s.mbTop[x] ? 1.f : 0.f, wb = s.mbBot[x] ? 1.f : 0.f;
        f[x] += (f[nx + x] - f[x]) * wt;
        f[bo] += (f[bo - nx] - f[bo]) * wb;
    }
    barrier();
}

template <int CH, int WAVES>
__global__ void __launch_bounds__(WAVES * kWave) fill2d_kernel_v2(Fill2dV2Args a)
{
    FILL_GEOMETRY(CH, WAVES);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* ring;
    const Handoff hand = fill2d_carve<CH, WAVES>(smem, ring);
    const Fill2dSlice s = fill2d_slice(a, blockIdx.x);
    if (s.skip) return;
    const uint32_t wave = threadIdx.x / kWave;
    const MultiWg single{0u, 1u, 0u, nullptr, a.error};
    for (unsigned long long n = 0; n < a.maxLoop; ++n) {
        const bool check = (n < (a.maxLoop - 5)) && (n % 10 == 0);
        int bad = 0;
        if (threadIdx.x < kV2Waves * 2) { hand.produced[threadIdx.x] = 0; hand.consumed[threadIdx.x] = 0; }
        __syncthreads();
        for (uint32_t b = wave; b < s.nBands; b += kV2Waves)
            if (check) fill2d_band<CH, WAVES, true>(s.f, s.maskS, ring, hand, b, s.nx, s.ny, s.mws, s.wInt, s.wZero, s.crtest, bad, single);
            else fill2d_band<CH, WAVES, false>(s.f, s.maskS, ring, hand, b, s.nx, s.ny, s.mws, s.wInt, s.wZero, s.crtest, bad, single);
        if (check) {
            if (!__syncthreads_or(bad)) return;  // converged (:1355-1359), before the border pass
        } else {
            __syncthreads();
        }
        fill2d_borders(s, threadIdx.x, kV2Threads, [] { __syncthreads(); });
    }
}

// The same sweeps with the bands of a slice dealt to a.groups workgroups (MultiWg, fill_sync.hpp).  Workgroup i serves slice
// (i % 8) + 8 * (i / (8 * groups)) as its member (i / 8) % groups: the workgroups of a slice have the same i % 8, which is how
// workgroups are dealt to the XCDs today (a speed bonus for the hand-off, not a condition: the write-through stores and the
// loads past the caches hold on any placement).  Launched cooperatively: the workgroups of a slice wait for each other.
template <int CH, int WAVES>
__global__ void __launch_bounds__(WAVES * kWave) fill2d_kernel_v3(Fill2dV2Args a)
{
    FILL_GEOMETRY(CH, WAVES);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* ring;
    const Handoff hand = fill2d_carve<CH, WAVES>(smem, ring);
    const uint32_t G = a.groups;
    const uint32_t slice = (blockIdx.x % kXcds) + kXcds * (blockIdx.x / (kXcds * G));
    const uint32_t g = (blockIdx.x / kXcds) % G;
    if (slice >= a.nz) return;
    const Fill2dSlice s = fill2d_slice(a, slice);
    unsigned int* sync = a.sync + (size_t)slice * a.syncStride;
    MultiWg mg{g, G, 0u, sync + 4, a.error};
    mg.experiment = a.experiment;
    mg.prof = a.prof;
    if (s.skip) return;
    const uint32_t wave = threadIdx.x / kWave;
    unsigned int barriers = 0, checks = 0, groupBarriers = 0;
    const uint32_t leader = a.couple ? slice % a.couple : slice;
    const uint32_t members = a.couple ? a.nz / a.couple : 1u;
    unsigned int* lsync = a.sync + (size_t)leader * a.syncStride;
    for (unsigned long long n = 0; n < a.maxLoop; ++n) {
        const bool check = (n < (a.maxLoop - 5)) && (n % 10 == 0);
        int bad = 0;
        if (threadIdx.x < kV2Waves * 2) { hand.produced[threadIdx.x] = 0; hand.consumed[threadIdx.x] = 0; }
        __syncthreads();
        for (uint32_t b = g * kV2Waves + wave; b < s.nBands; b += G * kV2Waves)
            if (check) fill2d_band<CH, WAVES, true, true>(s.f, s.maskS, ring, hand, b, s.nx, s.ny, s.mws, s.wInt, s.wZero, s.crtest, bad, mg);
            else fill2d_band<CH, WAVES, false, true>(s.f, s.maskS, ring, hand, b, s.nx, s.ny, s.mws, s.wInt, s.wZero, s.crtest, bad, mg);
        unsigned int* notConverged = lsync + 1 + (checks & 1);
        if (check) {
            if (__syncthreads_or(bad) && threadIdx.x == 0) __hip_atomic_fetch_or(notConverged, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        slice_barrier(sync, ++barriers * G, a.error);
        if (launch_failed(a.error)) return;
        if (check) {
            if (members > 1) {
                // the rectangles of one field: the word of the NEXT check is cleared before anybody can have passed this barrier
                // (it was read last at the previous check, which everybody has left behind), then all of them meet
                if (slice == leader && g == 0 && threadIdx.x == 0)
                    __hip_atomic_store(lsync + 1 + ((checks + 1) & 1), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                slice_barrier(lsync + 3, ++groupBarriers * members * G, a.error);
                if (launch_failed(a.error)) return;
            }
            if (__hip_atomic_load(notConverged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;  // converged (:1355-1359)
            ++checks;
            if (members == 1 && g == 0 && threadIdx.x == 0)  // the word of the check after next (read last ten sweeps ago)
                __hip_atomic_store(sync + 1 + (checks & 1), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // progress words of this workgroup's outgoing hand-offs: back to "nothing" for the next sweep
        for (uint32_t b = g * kV2Waves + kV2Waves - 1 + threadIdx.x * G * kV2Waves; b < s.nBands; b += kV2Threads * G * kV2Waves)
            __hip_atomic_store(mg.flags + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        fill2d_borders(s, g * kV2Threads + threadIdx.x, G * kV2Threads, [&] { slice_barrier(sync, ++barriers * G, a.error); });
        if (launch_failed(a.error)) return;
    }
}

// dynamic LDS of the systolic kernels (fill2d_carve): rings, hand-off rows, hand-off counters
size_t fill2d_lds_bytes(int waves, int ch)
{
    return (size_t)waves * (kWave + 1) * (2 * ch + 1) * sizeof(float) + (size_t)waves * 2 * kHandW * sizeof(float) + (size_t)waves * 4 * sizeof(unsigned int);
}

// tuning build, FILL_EXPERIMENT=4: the cycle counters of fill2d_band, printed when the call ends
struct Fill2dProfDump {
    DeviceArray<unsigned long long> counters;
    hipStream_t stream;
    uint32_t experiment;
    Fill2dProfDump(uint32_t experiment_, hipStream_t stream_) : counters(8), stream(stream_), experiment(experiment_)
    {
        FA_HIP(hipMemsetAsync(counters.get(), 0, counters.bytes(), stream));
    }
    ~Fill2dProfDump()
    {
        if (experiment != 4) return;
        unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        (void)hipStreamSynchronize(stream);
        (void)hipMemcpy(h, counters.get(), sizeof(h), hipMemcpyDeviceToHost);
        std::fprintf(stderr, "fill2d profile: bands %llu, cycles per band: events %.0f (waiting for the band above %.0f, for the band below %.0f), steps %.0f\n",
                     h[2], h[2] ? (double)h[0] / h[2] : 0.0, h[2] ? (double)h[3] / h[2] : 0.0, h[2] ? (double)h[4] / h[2] : 0.0,
                     h[2] ? (double)h[1] / h[2] : 0.0);
        std::fprintf(stderr, "fill2d profile: band 0 (waits for nobody above): events %.0f, steps %.0f cycles per sweep\n", h[7] ? (double)h[5] / h[7] : 0.0,
                     h[7] ? (double)h[6] / h[7] : 0.0);
    }
};

}  // namespace

bool run_fill2d_whole(size_t nx, size_t ny, size_t nz, float* d_field, float relaxCrit, float corrEff, size_t maxLoop,
                      size_t* h_nChanged, hipStream_t stream, const double* d_defaults, const double* d_devs, uint32_t couple)
{
    if (nx * ny == 0 || nz == 0) return true;  // :1248
    FA_REQUIRE(nx <= 0x7FFFFFFFu && ny <= 0x7FFFFFFFu && nz <= 0x7FFFFFFFu, "fill2d: slice too large");
    DeviceArray<SliceStats> stats(nz);
    FA_HIP(hipMemsetAsync(stats.get(), 0, nz * sizeof(SliceStats), stream));
    if (tuning("FILL_V2", 1) != 0 && systolic_fits(nx, ny)) {
        const size_t nBands = fill_bands(ny);
        const uint32_t mws = fill_mask_words(nx);
        DeviceArray<uint32_t> maskS(nz * ny * mws);
        DeviceArray<unsigned char> mbRows(nz * 2 * nx), mbCols(nz * 2 * ny);
        Fill2dV2Args a{};
        a.field = d_field;
        a.maskS = maskS.get();
        a.mbRows = mbRows.get();
        a.mbCols = mbCols.get();
        a.stats = stats.get();
        a.nx = (uint32_t)nx;
        a.ny = (uint32_t)ny;
        a.mws = mws;
        a.relaxCrit = relaxCrit;
        a.corrEff = corrEff;
        a.maxLoop = maxLoop;
        a.sumAlgo = tuning("SUM_ALGO", 1);
        if (couple > 0 && tuning("FILL_MULTI", 1) == 0) return false;
        launch_fill_prologue(false, d_field, stats.get(), nx, ny, nz, maskS.get(), mws, mbRows.get(), mbCols.get(), d_defaults == nullptr, d_defaults != nullptr, 0.f,
                             relaxCrit, stream, d_defaults, nullptr, d_devs);
        // small batches and short calls: 16 waves x 16 columns; from FILL_WIDE_NZ slices on: 8 waves x 32 columns
        const int geometry = tuning("FILL_GEOMETRY", 0);  // 0: by batch size, 1: 16 x 16, 2: 8 x 32
        const bool wide = geometry == 2 || (geometry == 0 && nz >= (size_t)tuning("FILL_WIDE_NZ", 8));
        const int waves = wide ? 8 : 16, ch = wide ? 32 : 16;
        const DeviceArray<unsigned int> error = cleared_words(1, stream);
        a.error = error.get();
        // several workgroups per slice (groups_per_slice): four waves per workgroup there, one per SIMD: a band's time is the time of
        // its dependent instruction chain, and a wave that shares its SIMD with three others runs that chain at a quarter of the
        // speed; the critical path of a sweep -- every band starts ~130 columns behind the one above -- is what a small batch waits for
        int mwaves = tuning("FILL_MULTI_WAVES", 4), mch = tuning("FILL_MULTI_CH", 16) == 32 ? 32 : 16;
        if (!(mwaves == 4 || mwaves == 8 || mwaves == 16)) mwaves = 4;
        if (mwaves == 16) mch = 16;  // 16 rings of 32 columns do not fit the LDS
        const size_t groups = groups_per_slice(nBands, (size_t)mwaves, nz);
        bool launched = false;
        DeviceArray<unsigned int> sync;
        if (groups > 1 || couple > 0) {
            Fill2dProfDump prof((uint32_t)tuning("FILL_EXPERIMENT", 0), stream);
            sync = multi_sync_words(a, nBands, groups, nz, stream);
            a.couple = couple;
            a.experiment = prof.experiment;
            a.prof = prof.counters.get();
            // more LDS than half a CU has, so that no two of these workgroups share a CU (and its SIMDs)
            const size_t mlds = std::max<size_t>(fill2d_lds_bytes(mwaves, mch), 84 * 1024);
            const void* kernel = mwaves == 16  ? reinterpret_cast<const void*>(&fill2d_kernel_v3<16, 16>)
                                 : mwaves == 8 ? (mch == 32 ? reinterpret_cast<const void*>(&fill2d_kernel_v3<32, 8>) : reinterpret_cast<const void*>(&fill2d_kernel_v3<16, 8>))
                                               : (mch == 32 ? reinterpret_cast<const void*>(&fill2d_kernel_v3<32, 4>) : reinterpret_cast<const void*>(&fill2d_kernel_v3<16, 4>));
            launched = launch_multi(kernel, groups, nz, mwaves * kWave, &a, mlds, stream);
            // (the prologue has filled the first guess in: a coupled run is of copies, the caller drops them)
            if (!launched && couple > 0) return false;
        }
        if (!launched)
            launch_single(wide ? reinterpret_cast<const void*>(&fill2d_kernel_v2<32, 8>) : reinterpret_cast<const void*>(&fill2d_kernel_v2<16, 16>), nz,
                          waves * kWave, &a, fill2d_lds_bytes(waves, ch), stream);
        finish_systolic(error, stats, nz, h_nChanged, stream, "fill2d");
        return true;
    }
    if (couple > 0 || d_defaults) return false;
    DeviceArray<float> w(nx * ny * nz);
    Fill2dArgs a{};
    a.field = d_field;
    a.w = w.get();
    a.stats = stats.get();
    a.nx = (uint32_t)nx;
    a.ny = (uint32_t)ny;
    a.relaxCrit = relaxCrit;
    a.corrEff = corrEff;
    a.maxLoop = maxLoop;
    a.sumAlgo = tuning("SUM_ALGO", 1);
    fill2d_kernel<<<dim3((uint32_t)nz), kFillBlock, 0, stream>>>(a);
    FA_HIP(hipGetLastError());
    collect_stats(stats, nz, h_nChanged, stream, "fill2d");
    return true;
}

}  // namespace fimex_amd
