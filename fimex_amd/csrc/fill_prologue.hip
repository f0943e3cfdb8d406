// What precedes the sweeps of the systolic fill kernels, and the host path of their launch (fill_prologue.hpp).
#include "fill_prologue.hpp"

#include <algorithm>
#include <vector>

namespace fimex_amd {

namespace {

// ---- what precedes the sweeps of both systolic kernels, as kernels of their own: the sums stay one workgroup per slice
// (the reference's order of additions), the first guess and the mask words are spread over the chip -- one workgroup
// streaming a 36 MB slice is latency bound (4 ms of a 15 ms call before the split).
__global__ void __launch_bounds__(kFillBlock) fill_stats_kernel(FillStatsArgs a)
{
    __shared__ __align__(16) double lds[2 * kSumTile];
    __shared__ double shAverage;
    __shared__ unsigned long long shUndef;
    const float* f = a.field + (size_t)blockIdx.x * a.total;
    SliceStats* st = a.stats + blockIdx.x;
    unsigned long long nUndef = 0;
    const double sum = scan_order_sum(f, a.total, a.useDefault ? 2 : 0, 0., lds, &nUndef, a.sumAlgo);
    if (threadIdx.x == 0) {
        const unsigned long long nDef = a.total - nUndef;
        shUndef = nUndef;
        shAverage = a.defaults ? a.defaults[blockIdx.x] : (a.useDefault ? (double)a.defaultVal : ((nDef != 0) ? sum / (double)nDef : 0.));  // :1281, :1516
        st->nUndef = nUndef;
        st->average = shAverage;
        st->status = 1;
        st->skip = (nDef == 0 || nUndef == 0);  // :1266-1269, :1384-1386
        st->sweepBound = a.bounds ? a.bounds[blockIdx.x] : nDef;
    }
    __syncthreads();
    nUndef = shUndef;
    const unsigned long long nDef = a.total - nUndef;
    if (a.devs) { if (threadIdx.x == 0) st->meanAbsDev = a.devs[blockIdx.x]; return; }
    if (!a.wantDeviation || nDef == 0 || nUndef == 0) return;
    const double dev = scan_order_sum(f, a.total, 1, shAverage, lds, nullptr, a.sumAlgo);
    if (threadIdx.x == 0) st->meanAbsDev = (double)a.relaxCrit * (dev / (double)nDef);  // :1302
}

struct FirstGuessArgs {
    float* field;
    const SliceStats* stats;
    uint32_t* mask;           // [nz][ny][mws]: fill2d NaN bits of the interior rows, creepfill "defined" bits of all rows
    unsigned char* mbRows;    // fill2d: [nz][2][nx] NaN mask of row 0 and row ny - 1
    unsigned char* mbCols;    // fill2d: [nz][2][ny] NaN mask of column 0 and column nx - 1
    uint32_t nx, ny, mws;
    uint32_t blocksPerSlice;
};

// One wave per row: undefined cells take the first guess (:1288-1299, :1408-1421) and the mask words are written in the
// row's skew (interior row y: bit x + ((y - 1) & 63)), eight row pieces in flight per wave.
template <bool CREEP>
__global__ void __launch_bounds__(kBlock) first_guess_kernel(FirstGuessArgs a)
{
    const uint32_t slice = blockIdx.x / a.blocksPerSlice;  // flat grid: gridDim.y stops at 65535 slices
    const SliceStats st = a.stats[slice];
    if (st.skip) return;
    const uint32_t nx = a.nx, ny = a.ny, mws = a.mws;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t y = (blockIdx.x % a.blocksPerSlice) * (kBlock / kWave) + threadIdx.x / kWave;
    if (y >= ny) return;
    const float guess = (float)st.average;
    float* row = a.field + ((size_t)slice * ny + y) * nx;
    const bool edgeRow = y == 0 || y == ny - 1;
    if (!CREEP && edgeRow) {
        unsigned char* mb = a.mbRows + ((size_t)slice * 2 + (y == 0 ? 0 : 1)) * nx;
        for (uint32_t x = lane; x < nx; x += kWave) {
            const bool u = isnan(row[x]);
            mb[x] = u;
            if (u) row[x] = guess;
        }
        return;
    }
    const uint32_t l = edgeRow ? 0u : ((y - 1) & (kWave - 1));
    uint32_t* mrow = a.mask + ((size_t)slice * ny + y) * mws;
    unsigned char* mbLeft = CREEP ? nullptr : a.mbCols + (size_t)slice * 2 * ny;
    constexpr int kAhead = 8;
    for (uint32_t base0 = 0; base0 < mws * 32; base0 += kAhead * kWave) {
        float v[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const int64_t x = (int64_t)base0 + k * kWave + lane - l;
            v[k] = (x >= 0 && x < (int64_t)nx && base0 + k * kWave < mws * 32) ? row[x] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kAhead; ++k) {
            const uint32_t base = base0 + k * kWave;
            if (base >= mws * 32) break;
            const int64_t x = (int64_t)base + lane - l;
            const bool in = x >= 0 && x < (int64_t)nx;
            const bool u = in && isnan(v[k]);
            const unsigned long long m = __ballot(CREEP ? (in && !u) : u);
            if (lane == 0) {
                mrow[base / 32] = (uint32_t)m;
                if (base / 32 + 1 < mws) mrow[base / 32 + 1] = (uint32_t)(m >> 32);
            }
            if (u) row[x] = guess;
            if (!CREEP) {
                if (in && x == 0) mbLeft[y] = u;
                if (in && x == (int64_t)nx - 1) mbLeft[ny + y] = u;
            }
        }
    }
}

}  // namespace

void launch_fill_stats(const FillStatsArgs& s, size_t nz, hipStream_t stream)
{
    fill_stats_kernel<<<dim3((uint32_t)nz), kFillBlock, 0, stream>>>(s);
    FA_HIP(hipGetLastError());
}

void launch_fill_prologue(bool creep, float* d_field, SliceStats* d_stats, size_t nx, size_t ny, size_t nz, uint32_t* mask, uint32_t mws,
                          unsigned char* mbRows, unsigned char* mbCols, bool wantDeviation, bool useDefault, float defaultVal, float relaxCrit,
                          hipStream_t stream, const double* d_defaults, const unsigned long long* d_bounds,
                          const double* d_devs)
{
    FillStatsArgs s{};
    s.defaults = d_defaults;
    s.bounds = d_bounds;
    s.devs = d_devs;
    s.field = d_field;
    s.stats = d_stats;
    s.total = nx * ny;
    s.wantDeviation = wantDeviation;
    s.useDefault = useDefault;
    s.defaultVal = defaultVal;
    s.relaxCrit = relaxCrit;
    // few slices: the sums over the whole chip (two reads of the data per sum, but 0.5 instead of 2.3 ms per 9 M-cell
    // pass); many slices: one workgroup per slice fills the chip already and reads the data once
    s.sumAlgo = tuning("SUM_ALGO", 3);
    if (s.sumAlgo == 3) s.sumAlgo = nz < (size_t)tuning("SUM_CHIP_NZ", 100) ? 2 : 1;
    if (d_defaults) s.sumAlgo = 1;  // only the undefined cells are counted
    if (s.sumAlgo >= 2) {
        const SumBuffers buffers(nx * ny, nz);
        StitchOut o{};
        o.stats = d_stats;
        o.total = nx * ny;
        o.useDefault = useDefault;
        o.defaultVal = defaultVal;
        o.relaxCrit = relaxCrit;
        SumJob first{d_field, nx * ny, useDefault ? 2 : 0, d_stats, 0.};
        launch_chip_sum(first, buffers, nz, o, stream);
        if (wantDeviation) {
            SumJob second{d_field, nx * ny, 1, d_stats, 0.};
            launch_chip_sum(second, buffers, nz, o, stream);
        }
        FA_HIP(hipStreamSynchronize(stream));  // the work arrays are released on return
    } else {
        launch_fill_stats(s, nz, stream);
    }
    FirstGuessArgs g{};
    g.field = d_field;
    g.stats = d_stats;
    g.mask = mask;
    g.mbRows = mbRows;
    g.mbCols = mbCols;
    g.nx = (uint32_t)nx;
    g.ny = (uint32_t)ny;
    g.mws = mws;
    const size_t rowBlocks = ceil_div(ny, (size_t)(kBlock / kWave));
    FA_REQUIRE(rowBlocks * nz <= 0x7FFFFFFFull, "too many slices for one call");
    g.blocksPerSlice = (uint32_t)rowBlocks;
    const dim3 grid((uint32_t)(rowBlocks * nz));
    if (creep) first_guess_kernel<true><<<grid, kBlock, 0, stream>>>(g);
    else first_guess_kernel<false><<<grid, kBlock, 0, stream>>>(g);
    FA_HIP(hipGetLastError());
}

int device_cus()
{
    int dev = 0, cus = 0;
    FA_HIP(hipGetDevice(&dev));
    FA_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    return cus;
}

// A grid whose workgroups wait for each other: all of them have to be resident at once.  hipLaunchCooperativeKernel checks the grid
// against the occupancy query and then launches like any other launch -- plain, cooperative and graph launches give identical
// residency (MI355X_MICROARCH.md, residency and cooperative launch).  The same check is made here and the launch is a plain one:
// 15-19 us less per call, and a process that is being profiled no longer dies in its exit handlers (rocprofv3 7.2 ends with
// SIGSEGV inside exit() after any cooperative launch, after its output is complete: profiles/r03_fill2d_nz16_abnormal_exit.txt).
// FILL_COOP=1 (tuning build) brings the cooperative launch back.  false: not every workgroup would be resident.
bool launch_resident(const void* kernel, dim3 grid, dim3 block, void** params, size_t ldsBytes, hipStream_t stream)
{
    if (tuning("FILL_COOP", 0) != 0) {
        if (hipLaunchCooperativeKernel(kernel, grid, block, params, (unsigned int)ldsBytes, stream) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    }
    int perCu = 0;
    const int cus = device_cus();
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, kernel, (int)block.x, ldsBytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if ((size_t)perCu * (size_t)cus < (size_t)grid.x * grid.y * grid.z) return false;
    FA_HIP(hipLaunchKernel(kernel, grid, block, params, ldsBytes, stream));
    return true;
}

void collect_stats(const DeviceArray<SliceStats>& d_stats, size_t nz, size_t* h_nChanged, hipStream_t stream, const char* what)
{
    std::vector<SliceStats> st(nz);
    FA_HIP(hipMemcpyAsync(st.data(), d_stats.get(), nz * sizeof(SliceStats), hipMemcpyDeviceToHost, stream));
    FA_HIP(hipStreamSynchronize(stream));
    bool failed = false;
    for (size_t z = 0; z < nz; ++z) {
        if (h_nChanged) h_nChanged[z] = (size_t)st[z].nUndef;
        if (st[z].status != 1) failed = true;
    }
    if (failed) throw Error(std::string(what) + ": slices need nx >= 2 and ny >= 2");
}

// ---- the systolic launch of a batch (fill_prologue.hpp)

// the systolic kernels pack "band, column" into 32-bit hand-off counters and address 66 rows through one buffer
bool systolic_fits(size_t nx, size_t ny)
{
    return nx >= 4 && ny >= 4 && fill_bands(ny) < (size_t)kMaxBands && nx < (1u << 19) && (size_t)(kWave + 2) * nx * 4 < 0xFFFFFFFFull;
}

// Small batches leave most of the chip idle at one workgroup per slice: the bands of a slice are dealt to several workgroups
// (one per CU: the rings fill the LDS), as many as there are groups of `wavesPerWg` bands and as fit the XCD the slice's
// workgroups share with the slices of the same i % 8.  1: one workgroup per slice.
size_t groups_per_slice(size_t nBands, size_t wavesPerWg, size_t nz)
{
    const size_t bandGroups = ceil_div(nBands, wavesPerWg);
    const size_t perXcd = ceil_div(nz, (size_t)kXcds);  // slices whose workgroups meet on one XCD
    const size_t cusPerXcd = (size_t)std::max(1, device_cus() / kXcds);
    const size_t groups = std::min(bandGroups, perXcd ? cusPerXcd / perXcd : (size_t)1);
    return (tuning("FILL_MULTI", 1) == 0 || groups < 2) ? 1 : groups;
}

DeviceArray<unsigned int> cleared_words(size_t n, hipStream_t stream)
{
    DeviceArray<unsigned int> words(n);
    FA_HIP(hipMemsetAsync(words.get(), 0, words.bytes(), stream));
    return words;
}

// `groups` workgroups per slice, every workgroup of the grid resident (they wait for each other); false: not launched, one
// workgroup per slice has to do the work
bool launch_multi(const void* kernel, size_t groups, size_t nz, int threads, void* args, size_t ldsBytes, hipStream_t stream)
{
    allow_dynamic_lds(kernel, ldsBytes);
    void* params[] = {args};
    const dim3 grid((uint32_t)(kXcds * groups * ceil_div(nz, (size_t)kXcds)));
    return launch_resident(kernel, grid, dim3((uint32_t)threads), params, ldsBytes, stream);
}

void launch_single(const void* kernel, size_t nz, int threads, void* args, size_t ldsBytes, hipStream_t stream)
{
    allow_dynamic_lds(kernel, ldsBytes);
    void* params[] = {args};
    FA_HIP(hipLaunchKernel(kernel, dim3((uint32_t)nz), dim3((uint32_t)threads), params, ldsBytes, stream));
}

void finish_systolic(const DeviceArray<unsigned int>& error, const DeviceArray<SliceStats>& stats, size_t nz, size_t* h_nChanged,
                     hipStream_t stream, const char* what)
{
    FA_HIP(hipGetLastError());
    unsigned int failed = 0;
    FA_HIP(hipMemcpyAsync(&failed, error.get(), sizeof(failed), hipMemcpyDeviceToHost, stream));
    collect_stats(stats, nz, h_nChanged, stream, what);  // synchronises the stream
    FA_REQUIRE(failed == 0, std::string(what) + ": a hand-off between waves or workgroups did not arrive (wait " + std::to_string(failed) +
                                " gave up); the field is not valid");
}

}  // namespace fimex_amd
