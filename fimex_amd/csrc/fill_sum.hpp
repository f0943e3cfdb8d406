// The sums that feed the first guess of the fills (mean, mean absolute deviation), in the reference's scan order: the device
// templates every kernel that sums uses, and the chip-wide version that fill_sum.hip launches.
#pragma once

#include "plan.hpp"

namespace fimex_amd {

constexpr int kFillBlock = 1024;

struct SliceStats {
    unsigned long long nUndef;
    double average;     // first guess (mean of the defined cells, or the caller's default value)
    double meanAbsDev;  // fill2d: relaxCrit * mean absolute deviation = the convergence criterion
    int status;         // 1 ok, -1 error
    int skip;           // nothing to fill or nothing defined: the slice is left alone
    unsigned long long sweepBound;  // creep fills: the loop ends after this many sweeps at the latest (:1430: the number of defined cells;
                                    // for a rectangle of a decomposed fill: of the whole slice)
};

namespace {

// sum of the defined values in scan order, double accumulator (interpolation.c:1256-1264, 1502-1513);
// mode 1: sum of |v - average| instead (:1288-1299); mode 2: only count the undefined cells.
//
// The additions form one dependent chain -- that is the point: the reference's order, hence its rounding.  All
// else is taken off the chain: waves 1.. turn tile t+1 into ready double addends in LDS (undefined -> +0.0, which
// leaves a sum that started at +0.0 unchanged; padding likewise) and count the undefined cells, while wave 0 walks
// tile t with nothing but 16-byte LDS reads and v_add_f64.  buf: 2 * kSumTile doubles of LDS.
constexpr int kSumTile = 2048;

__device__ __forceinline__ double sum_addend(float v, int mode, double average, unsigned int& nUndef)
{
    const bool undef = isnan(v);
    nUndef += undef;
    return undef ? 0.0 : (mode == 0 ? (double)v : fabs((double)v - average));
}

template <int BLOCK = kFillBlock>
__device__ double serial_sum(const float* __restrict__ f, size_t total, int mode, double average, double* buf,
                             unsigned long long* nUndefOut)
{
    __shared__ unsigned long long shCount;
    constexpr int kProducers = BLOCK - kWave;
    const size_t nTiles = (total + kSumTile - 1) / kSumTile;
    unsigned int myUndef = 0;
    double sum = 0;
    if (threadIdx.x == 0) shCount = 0;
    // tile 0 by everybody
    for (size_t i = threadIdx.x; i < (size_t)kSumTile; i += BLOCK)
        buf[i] = (i < total) ? sum_addend(f[i], mode, average, myUndef) : 0.0;
    __syncthreads();
    for (size_t t = 0; t < nTiles; ++t) {
        if (threadIdx.x < kWave) {
            if (mode != 2) {
                const double2* b2 = reinterpret_cast<const double2*>(buf + (t & 1) * kSumTile);
                double2 q0 = b2[0], q1 = b2[1], q2 = b2[2], q3 = b2[3];
#pragma unroll 2
                for (int g = 1; g <= kSumTile / 8; ++g) {  // the next 8 addends are read while these 8 are added
                    const int h = (g < kSumTile / 8) ? g : 0;
                    const double2 n0 = b2[4 * h], n1 = b2[4 * h + 1], n2 = b2[4 * h + 2], n3 = b2[4 * h + 3];
                    sum += q0.x; sum += q0.y; sum += q1.x; sum += q1.y;
                    sum += q2.x; sum += q2.y; sum += q3.x; sum += q3.y;
                    q0 = n0; q1 = n1; q2 = n2; q3 = n3;
                }
            }
        } else if (t + 1 < nTiles) {
            const size_t base = (t + 1) * kSumTile;
            double* dst = buf + ((t + 1) & 1) * kSumTile;
            for (size_t i = threadIdx.x - kWave; i < (size_t)kSumTile; i += kProducers)
                dst[i] = (base + i < total) ? sum_addend(f[base + i], mode, average, myUndef) : 0.0;
        }
        __syncthreads();
    }
    if (nUndefOut) {
        if (myUndef) atomicAdd(&shCount, (unsigned long long)myUndef);
        __syncthreads();
        *nUndefOut = shCount;
        __syncthreads();
    }
    return sum;  // valid in wave 0
}

// ---- the same sums without walking the chain: "binade-parallel" evaluation, bit for bit the sequential result.
//
// While the running sum S stays inside one binade [2^e, 2^(e+1)), it is a multiple of u = 2^(e-52) and every
// S <- fl(S + a) rounds the exact value to a multiple of u, so fl(S + a) = S + rn_u(a) whenever a is not exactly halfway
// between two multiples of u (rn_u: round to the nearest multiple).  The rounded addends k = rn_u(a) / u are integers and
// integer sums are associative: a chunk of 1024 elements contributes I = sum k, in any order, PROVIDED S provably stays
// inside the binade for all 1024 partial sums.  With A = sum |k| and m = |S| / u (an integer in [2^52, 2^53)) that is
// guaranteed by  m - A >= 2^52 + 1  and  m + A <= 2^53 - 1  (the +-1 keeps the exact, unrounded partial sums inside as
// well), and A < 2^50 keeps all integer arithmetic exact in doubles.  A chunk that fails any test -- a tie, a binade
// crossing, S = 0, non-finite values -- is re-evaluated at the binade S has by then, or walked element by element.
// Per super-block of 16 chunks: every wave evaluates its chunk at the binade S had after the previous super-block,
// then wave 0 strings the 16 results together (lanes = chunks, prefix over I) and repairs what failed.
constexpr int kSumE = 16;                 // elements per lane
constexpr int kChunk = kWave * kSumE;     // elements per wave and super-block
constexpr int kNoBinade = 0x7fffffff;

__device__ __forceinline__ double pow2d(int e) { return __longlong_as_double((long long)(e + 1023) << 52); }  // |e| < 1000
__device__ __forceinline__ int exponent_of(double s) { return (int)((__double_as_longlong(s) >> 52) & 0x7FF) - 1023; }
__device__ __forceinline__ bool binade_usable(double s, int e) { return s != 0.0 && e > -900 && e < 900; }  // excludes inf, NaN, subnormals
__device__ __forceinline__ double lane_value_d(double v, int idx)
{
    const long long b = __double_as_longlong(v);
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)b, idx), hi = (unsigned int)__builtin_amdgcn_readlane((int)(b >> 32), idx);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// v of the lane CTRL names (DPP: 0x110 + n = n lanes up within the row of 16, 0x142 / 0x143 = last lane of the previous
// row / of the first half), 0.0 where there is none or the row is masked out: cross-lane adds without an LDS round trip
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_d(double v)
{
    const long long b = __double_as_longlong(v);
    const unsigned int lo = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROW_MASK, 0xf, true);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, true);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// inclusive prefix sum within each row of 16 lanes
__device__ __forceinline__ double row_scan_d(double v)
{
    v += dpp_d<0x111>(v);
    v += dpp_d<0x112>(v);
    v += dpp_d<0x114>(v);
    v += dpp_d<0x118>(v);
    return v;
}
// sum over the wave, in every lane (exact integers: the order does not matter)
__device__ __forceinline__ double wave_sum_d(double v)
{
    v = row_scan_d(v);           // lane 15 of each row: the row's sum
    v += dpp_d<0x142, 0xa>(v);   // rows 1 and 3 += row before
    v += dpp_d<0x143, 0xc>(v);   // rows 2 and 3 += first half
    return lane_value_d(v, kWave - 1);
}

struct ChunkSum {
    double I, A;
    bool ok;
};

__device__ __forceinline__ void chunk_load(const float* __restrict__ f, size_t base, size_t total, float (&v)[kSumE])
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int j = 0; j < kSumE; ++j) {  // element j * 64 + lane of the chunk: coalesced; the integer sums do not care about order
        const size_t i = base + (size_t)j * kWave + lane;
        v[j] = (i < total) ? f[i] : 0.f;
    }
}

__device__ __forceinline__ void chunk_addends(const float (&v)[kSumE], size_t base, size_t total, int mode, double average,
                                              double (&a)[kSumE], unsigned int* nUndef)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int j = 0; j < kSumE; ++j) {
        const bool in = base + (size_t)j * kWave + lane < total;
        const bool undef = isnan(v[j]);
        if (nUndef) *nUndef += undef;
        a[j] = (undef || !in) ? 0.0 : (mode == 0 ? (double)v[j] : fabs((double)v[j] - average));
    }
}

// one wave, 1024 consecutive elements from `base` (already in v): integer image of the addends at binade e
__device__ ChunkSum chunk_eval(const float (&v)[kSumE], size_t base, size_t total, int mode, double average, int e, unsigned int* nUndef)
{
    double a[kSumE];
    chunk_addends(v, base, total, mode, average, a, nUndef);
    const double scale = pow2d(52 - e);
    double sI = 0, sA = 0;
    bool tie = false;
#pragma unroll
    for (int j = 0; j < kSumE; ++j) {
        const double t = a[j] * scale;  // exact: a power of two
        const double k = rint(t);
        tie |= (fabs(t - k) == 0.5);
        sI += k;
        sA += fabs(k);
    }
    ChunkSum r;
    r.I = wave_sum_d(sI);
    r.A = wave_sum_d(sA);
    r.ok = !__any(tie) && r.A < 0x1p50;  // false for inf and NaN as well
    return r;
}

// one wave, the same 1024 elements one after the other on the running sum
__device__ double chunk_chain(const float* __restrict__ f, size_t base, size_t total, int mode, double average, double S)
{
    float v[kSumE];
    double a[kSumE];
    chunk_load(f, base, total, v);
    chunk_addends(v, base, total, mode, average, a, nullptr);
#pragma unroll
    for (int j = 0; j < kSumE; ++j) {
        for (int l = 0; l < kWave; ++l) S += lane_value_d(a[j], l);
    }
    return S;
}

template <int BLOCK = kFillBlock>
__device__ double binade_sum(const float* __restrict__ f, size_t total, int mode, double average, unsigned long long* nUndefOut)
{
    constexpr int kWaves = BLOCK / kWave;
    static_assert(kWaves <= 16, "lanes 0..15 of wave 0 stand for the chunks of a super-block");
    constexpr size_t kSuper = (size_t)kWaves * kChunk;
    __shared__ double shI[kWaves], shA[kWaves];
    __shared__ int shOk[kWaves];
    __shared__ int shE;
    __shared__ unsigned long long shCount;
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned int myUndef = 0;
    double S = 0;  // wave 0
    if (threadIdx.x == 0) { shE = kNoBinade; shCount = 0; }
    __syncthreads();
    if (mode == 2) {
        for (size_t i = threadIdx.x; i < total; i += BLOCK) myUndef += isnan(f[i]);
    } else {
        float vNext[kSumE];
        chunk_load(f, (size_t)wave * kChunk, total, vNext);
        for (size_t sb = 0; sb < total; sb += kSuper) {
            const int e = shE;
            float vCur[kSumE];
#pragma unroll
            for (int j = 0; j < kSumE; ++j) vCur[j] = vNext[j];
            chunk_load(f, sb + kSuper + (size_t)wave * kChunk, total, vNext);  // the next super-block, while this one is worked on
            ChunkSum cs = chunk_eval(vCur, sb + (size_t)wave * kChunk, total, mode, average, e == kNoBinade ? 0 : e, &myUndef);
            if (lane == 0) { shI[wave] = cs.I; shA[wave] = cs.A; shOk[wave] = (cs.ok && e != kNoBinade) ? 1 : 0; }
            __syncthreads();
            if (wave == 0) {
                const int nCh = (int)(((total - sb < kSuper ? total - sb : kSuper) + kChunk - 1) / kChunk);
                const double I = lane < (uint32_t)kWaves ? shI[lane] : 0.0, A = lane < (uint32_t)kWaves ? shA[lane] : 0.0;
                const bool ok = lane < (uint32_t)kWaves && shOk[lane] != 0;
                int w0 = 0;
                while (w0 < nCh) {
                    int eS = exponent_of(S);
                    if (binade_usable(S, eS) && eS == e) {
                        const double n = fabs(S) * pow2d(52 - eS), sg = S < 0 ? -1.0 : 1.0;
                        const double x = ((int)lane >= w0 && (int)lane < nCh) ? sg * I : 0.0;
                        const double incl = row_scan_d(x);
                        const double m = n + (incl - x);  // |S| / u before chunk `lane`, if all chunks from w0 on can be taken
                        const bool good = ok && (m - A >= 0x1p52 + 1.0) && (m + A <= 0x1p53 - 1.0);
                        const unsigned long long bad = __ballot((int)lane >= w0 && (int)lane < nCh && !good);
                        const int wf = bad ? (int)__ffsll((long long)bad) - 1 : nCh;
                        if (wf > w0) S = sg * ((n + lane_value_d(incl, wf - 1)) * pow2d(eS - 52));
                        w0 = wf;
                        if (w0 == nCh) break;
                    }
                    // chunk w0 on its own: at the binade S is in now, else element by element
                    const size_t cb = sb + (size_t)w0 * kChunk;
                    eS = exponent_of(S);
                    bool done = false;
                    if (binade_usable(S, eS)) {
                        float vOne[kSumE];
                        chunk_load(f, cb, total, vOne);
                        const ChunkSum one = chunk_eval(vOne, cb, total, mode, average, eS, nullptr);
                        const double n = fabs(S) * pow2d(52 - eS), sg = S < 0 ? -1.0 : 1.0;
                        if (one.ok && (n - one.A >= 0x1p52 + 1.0) && (n + one.A <= 0x1p53 - 1.0)) {
                            S = sg * ((n + sg * one.I) * pow2d(eS - 52));
                            done = true;
                        }
                    }
                    if (!done) S = chunk_chain(f, cb, total, mode, average, S);
                    ++w0;
                }
                if (lane == 0) {
                    const int eS = exponent_of(S);
                    shE = binade_usable(S, eS) ? eS : kNoBinade;
                }
            }
            __syncthreads();
        }
    }
    if (nUndefOut) {
        if (myUndef) atomicAdd(&shCount, (unsigned long long)myUndef);
        __syncthreads();
        *nUndefOut = shCount;
        __syncthreads();
    }
    return S;  // valid in wave 0
}

// algo 0: the chain (serial_sum), 1: binade-parallel
template <int BLOCK = kFillBlock>
__device__ double scan_order_sum(const float* __restrict__ f, size_t total, int mode, double average, double* buf,
                                 unsigned long long* nUndefOut, int algo)
{
    if (algo == 0) return serial_sum<BLOCK>(f, total, mode, average, buf, nUndefOut);
    return binade_sum<BLOCK>(f, total, mode, average, nUndefOut);
}

}  // namespace

// ---- the chip-wide sum (fill_sum.hip): what its callers hand over
struct SumWork {
    double* approx;        // [slices][nChunks] plain sum of the chunk's addends (any order)
    double* I;             // integer image of the chunk at binade e
    double* A;
    int* e;                // predicted binade of the running sum before the chunk (kNoBinade: none)
    int* ok;
    unsigned int* undef;   // undefined cells of the chunk
    size_t nChunks;
};

struct SumJob {
    const float* values;   // [slices][total]
    size_t total;
    int mode;              // 0 sum, 1 sum of |v - average|, 2 count only
    const SliceStats* stats;  // mode 1: average per slice; slices with skip set are left out (nullptr: averageAll, none skipped)
    double averageAll;
};

// the two uses: a plain sum into host-visible cells (scan_sum), and the statistics of the fills
struct StitchOut {
    double* sum;                 // [slices] or nullptr
    unsigned long long* nUndef;  // [slices] or nullptr
    SliceStats* stats;           // fills: nullptr otherwise
    size_t total;
    int useDefault;
    float defaultVal;
    float relaxCrit;
};

struct SumBuffers {
    DeviceArray<double> approx, I, A;
    DeviceArray<int> e, ok;
    DeviceArray<unsigned int> undef;
    SumWork work{};
    SumBuffers(size_t total, size_t slices)
    {
        const size_t nChunks = ceil_div(total, (size_t)kChunk), n = nChunks * slices;
        approx.allocate(n); I.allocate(n); A.allocate(n); e.allocate(n); ok.allocate(n); undef.allocate(n);
        work = SumWork{approx.get(), I.get(), A.get(), e.get(), ok.get(), undef.get(), nChunks};
    }
};

void launch_chip_sum(const SumJob& j, const SumBuffers& b, size_t slices, const StitchOut& o, hipStream_t stream);

}  // namespace fimex_amd
