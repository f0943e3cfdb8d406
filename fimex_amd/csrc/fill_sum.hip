// Scan-order sums over the whole chip, and the sum entry point of the C ABI (run_scan_sum).
#include "fill_sum.hpp"

namespace fimex_amd {

namespace {

// ---- the same sum over the whole chip (algo 2).  One workgroup walking a 36 MB slice super-block by super-block takes
// 2.3 ms per pass, all of it synchronisation and the stitch of wave 0.  What a chunk needs is only the BINADE the running
// sum has when it arrives there, and an approximate prefix sum predicts that: (1) every chunk's plain double sum, (2) their
// exclusive prefix -> predicted binade per chunk, (3) every chunk's integer image at its predicted binade, (4) one wave per
// slice strings the chunks together exactly as wave 0 does above -- a chunk whose prediction is wrong (next to a binade
// crossing) or whose test fails is re-evaluated or walked element by element there.  The result is the reference's sum
// whatever the prediction was; a bad prediction only costs time.
// (SumWork, SumJob: fill_sum.hpp)
__device__ __forceinline__ bool sum_slice_active(const SumJob& j, uint32_t slice, double& average)
{
    average = j.averageAll;
    if (j.stats && j.mode == 1) {
        if (j.stats[slice].skip) return false;
        average = j.stats[slice].average;
    }
    return true;
}

// (grids of the per-chunk kernels are flat: blocks of a slice, then the next slice -- gridDim.y stops at 65535 slices)
__global__ void __launch_bounds__(kBlock) sum_approx_kernel(SumJob j, SumWork w, uint32_t blocksPerSlice)
{
    const uint32_t lane = threadIdx.x & (kWave - 1), slice = blockIdx.x / blocksPerSlice;
    const size_t c = (size_t)(blockIdx.x % blocksPerSlice) * (kBlock / kWave) + threadIdx.x / kWave;
    double average;
    if (c >= w.nChunks || !sum_slice_active(j, slice, average)) return;
    const float* f = j.values + (size_t)slice * j.total;
    float v[kSumE];
    double a[kSumE];
    unsigned int nUndef = 0;
    chunk_load(f, c * kChunk, j.total, v);
    chunk_addends(v, c * kChunk, j.total, j.mode == 2 ? 0 : j.mode, average, a, &nUndef);
    double s = 0;
#pragma unroll
    for (int k = 0; k < kSumE; ++k) s += a[k];
    s = wave_sum_d(s);
    const unsigned int u = (unsigned int)wave_sum_d((double)nUndef);
    if (lane == 0) {
        w.approx[(size_t)slice * w.nChunks + c] = s;
        w.undef[(size_t)slice * w.nChunks + c] = u;
    }
}

// exclusive prefix of the approximate chunk sums -> predicted binade; one workgroup per slice
__global__ void __launch_bounds__(kFillBlock) sum_predict_kernel(SumJob j, SumWork w)
{
    __shared__ double shTot[kFillBlock];
    const uint32_t slice = blockIdx.x;
    double average;
    if (!sum_slice_active(j, slice, average)) return;
    const double* ap = w.approx + (size_t)slice * w.nChunks;
    int* e = w.e + (size_t)slice * w.nChunks;
    const size_t per = (w.nChunks + kFillBlock - 1) / kFillBlock;
    const size_t c0 = (size_t)threadIdx.x * per, c1 = c0 + per < w.nChunks ? c0 + per : w.nChunks;
    double mine = 0;
    for (size_t c = c0; c < c1; ++c) mine += ap[c];
    shTot[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < kFillBlock; off <<= 1) {  // inclusive scan of the thread totals
        const double add = threadIdx.x >= (uint32_t)off ? shTot[threadIdx.x - off] : 0.0;
        __syncthreads();
        shTot[threadIdx.x] += add;
        __syncthreads();
    }
    double P = shTot[threadIdx.x] - mine;
    for (size_t c = c0; c < c1; ++c) {
        const int eP = exponent_of(P);
        e[c] = binade_usable(P, eP) ? eP : kNoBinade;
        P += ap[c];
    }
}

__global__ void __launch_bounds__(kBlock) sum_eval_kernel(SumJob j, SumWork w, uint32_t blocksPerSlice)
{
    const uint32_t lane = threadIdx.x & (kWave - 1), slice = blockIdx.x / blocksPerSlice;
    const size_t c = (size_t)(blockIdx.x % blocksPerSlice) * (kBlock / kWave) + threadIdx.x / kWave;
    double average;
    if (c >= w.nChunks || !sum_slice_active(j, slice, average)) return;
    const size_t idx = (size_t)slice * w.nChunks + c;
    const int e = w.e[idx];
    float v[kSumE];
    chunk_load(j.values + (size_t)slice * j.total, c * kChunk, j.total, v);
    const ChunkSum cs = chunk_eval(v, c * kChunk, j.total, j.mode, average, e == kNoBinade ? 0 : e, nullptr);
    if (lane == 0) {
        w.I[idx] = cs.I;
        w.A[idx] = cs.A;
        w.ok[idx] = (cs.ok && e != kNoBinade) ? 1 : 0;
    }
}

// inclusive prefix sum over the 64 lanes
__device__ __forceinline__ double wave_scan_d(double v)
{
    v = row_scan_d(v);
    v += dpp_d<0x142, 0xa>(v);
    v += dpp_d<0x143, 0xc>(v);
    return v;
}

// one wave per slice: the chunks in order, 64 at a time (lanes = chunks)
__device__ double stitch_chunks(const SumJob& j, const SumWork& w, uint32_t slice, double average, unsigned long long* nUndefOut)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const float* f = j.values + (size_t)slice * j.total;
    const size_t off = (size_t)slice * w.nChunks;
    double S = 0;
    unsigned long long undef = 0;
    for (size_t g0 = 0; g0 < w.nChunks; g0 += kWave) {
        const int nCh = (int)(w.nChunks - g0 < (size_t)kWave ? w.nChunks - g0 : (size_t)kWave);
        const bool mine = (int)lane < nCh;
        undef += mine ? w.undef[off + g0 + lane] : 0u;
        if (j.mode == 2) continue;
        const double I = mine ? w.I[off + g0 + lane] : 0.0, A = mine ? w.A[off + g0 + lane] : 0.0;
        const bool ok = mine && w.ok[off + g0 + lane] != 0;
        const int eC = mine ? w.e[off + g0 + lane] : kNoBinade;
        int w0 = 0;
        while (w0 < nCh) {
            int eS = exponent_of(S);
            if (binade_usable(S, eS)) {
                const double n = fabs(S) * pow2d(52 - eS), sg = S < 0 ? -1.0 : 1.0;
                const bool cand = (int)lane >= w0 && mine && ok && eC == eS;
                const double x = cand ? sg * I : 0.0;
                const double incl = wave_scan_d(x);
                const double m = n + (incl - x);  // |S| / u before chunk `lane`, if all chunks from w0 on can be taken
                const bool good = cand && (m - A >= 0x1p52 + 1.0) && (m + A <= 0x1p53 - 1.0);
                const unsigned long long bad = __ballot((int)lane >= w0 && mine && !good);
                const int wf = bad ? (int)__ffsll((long long)bad) - 1 : nCh;
                if (wf > w0) S = sg * ((n + lane_value_d(incl, wf - 1)) * pow2d(eS - 52));
                w0 = wf;
                if (w0 == nCh) break;
            }
            // chunk w0 on its own: at the binade S is in now, else element by element
            const size_t cb = (g0 + (size_t)w0) * kChunk;
            eS = exponent_of(S);
            bool done = false;
            if (binade_usable(S, eS)) {
                float vOne[kSumE];
                chunk_load(f, cb, j.total, vOne);
                const ChunkSum one = chunk_eval(vOne, cb, j.total, j.mode, average, eS, nullptr);
                const double n = fabs(S) * pow2d(52 - eS), sg = S < 0 ? -1.0 : 1.0;
                if (one.ok && (n - one.A >= 0x1p52 + 1.0) && (n + one.A <= 0x1p53 - 1.0)) {
                    S = sg * ((n + sg * one.I) * pow2d(eS - 52));
                    done = true;
                }
            }
            if (!done) S = chunk_chain(f, cb, j.total, j.mode, average, S);
            ++w0;
        }
    }
    if (nUndefOut) *nUndefOut = (unsigned long long)wave_sum_d((double)undef);  // < 2^53: exact
    return S;
}

__global__ void __launch_bounds__(kWave) sum_stitch_kernel(SumJob j, SumWork w, StitchOut o)
{
    const uint32_t slice = blockIdx.x;
    double average;
    if (!sum_slice_active(j, slice, average)) return;
    unsigned long long nUndef = 0;
    const double S = stitch_chunks(j, w, slice, average, &nUndef);
    if (threadIdx.x != 0) return;
    if (o.sum) o.sum[slice] = S;
    if (o.nUndef) o.nUndef[slice] = nUndef;
    if (!o.stats) return;
    SliceStats* st = o.stats + slice;
    if (j.mode != 1) {  // first pass: count, first guess (:1281, :1516)
        const unsigned long long nDef = o.total - nUndef;
        st->nUndef = nUndef;
        st->average = o.useDefault ? (double)o.defaultVal : ((nDef != 0) ? S / (double)nDef : 0.);
        st->status = 1;
        st->skip = (nDef == 0 || nUndef == 0);
        st->sweepBound = nDef;
    } else {            // second pass: the convergence criterion (:1302)
        const unsigned long long nDef = o.total - st->nUndef;
        st->meanAbsDev = (double)o.relaxCrit * (S / (double)nDef);
    }
}

}  // namespace

void launch_chip_sum(const SumJob& j, const SumBuffers& b, size_t slices, const StitchOut& o, hipStream_t stream)
{
    const size_t blocksPerSlice = ceil_div(b.work.nChunks, (size_t)(kBlock / kWave));
    FA_REQUIRE(blocksPerSlice * slices <= 0x7FFFFFFFull, "too many slices for one call");
    const dim3 perChunk((uint32_t)(blocksPerSlice * slices));
    sum_approx_kernel<<<perChunk, kBlock, 0, stream>>>(j, b.work, (uint32_t)blocksPerSlice);
    if (j.mode != 2) {
        sum_predict_kernel<<<dim3((uint32_t)slices), kFillBlock, 0, stream>>>(j, b.work);
        sum_eval_kernel<<<perChunk, kBlock, 0, stream>>>(j, b.work, (uint32_t)blocksPerSlice);
    }
    sum_stitch_kernel<<<dim3((uint32_t)slices), kWave, 0, stream>>>(j, b.work, o);
    FA_HIP(hipGetLastError());
}

namespace {

struct ScanSumArgs {
    const float* values;
    size_t n;
    int mode, algo;
    double average;
    double* sum;
    unsigned long long* nUndef;
};

__global__ void __launch_bounds__(kFillBlock) scan_sum_kernel(ScanSumArgs a)
{
    __shared__ __align__(16) double lds[2 * kSumTile];
    unsigned long long nUndef = 0;
    const double s = scan_order_sum(a.values, a.n, a.mode, a.average, lds, &nUndef, a.algo);
    if (threadIdx.x == 0) { *a.sum = s; *a.nUndef = nUndef; }
}

}  // namespace

void run_scan_sum(const float* d_values, size_t n, int mode, double average, int algo, double* h_sum, size_t* h_nUndefined, hipStream_t stream)
{
    FA_REQUIRE(mode >= 0 && mode <= 2 && algo >= 0 && algo <= 2, "scan_sum: mode 0..2, algo 0..2");
    DeviceArray<double> d_sum(1);
    DeviceArray<unsigned long long> d_undef(1);
    if (algo == 2 && n > 0) {
        const SumBuffers buffers(n, 1);
        SumJob j{d_values, n, mode, nullptr, average};
        StitchOut o{};
        o.sum = d_sum.get();
        o.nUndef = d_undef.get();
        launch_chip_sum(j, buffers, 1, o, stream);
        FA_HIP(hipStreamSynchronize(stream));
    } else {
        ScanSumArgs a{d_values, n, mode, algo == 2 ? 1 : algo, average, d_sum.get(), d_undef.get()};
        scan_sum_kernel<<<1, kFillBlock, 0, stream>>>(a);
        FA_HIP(hipGetLastError());
    }
    unsigned long long u = 0;
    FA_HIP(hipMemcpyAsync(h_sum, d_sum.get(), sizeof(double), hipMemcpyDeviceToHost, stream));
    FA_HIP(hipMemcpyAsync(&u, d_undef.get(), sizeof(u), hipMemcpyDeviceToHost, stream));
    FA_HIP(hipStreamSynchronize(stream));
    if (h_nUndefined) *h_nUndefined = (size_t)u;
}

}  // namespace fimex_amd
