// Extraction: CDMExtractor::getDataSlice_ (src/CDMExtractor.cc:96-179) for one variable.  Some dimensions are
// reduced to picked positions (dimSlices_), the caller's SliceBuilder adds a window per dimension, and the result is the row-major
// array of the reduced shape in the variable's stored type: bytes are moved, never interpreted.
//
// The host normalises the description once per plan.  Dimensions of output length 1 fold into a base offset.  A dimension taken
// whole merges with its slower neighbour, so a pick of levels over whole planes becomes a few long runs.  What is left is a
// fastest dimension, whose output row is a list of runs that are contiguous in the source, and up to seven slower dimensions with
// one source offset per output index.  All offsets count elements in 64 bits; output indices are 32-bit where the output is
// shorter than 2^31 elements, since they are what the kernel divides.
//
// One streaming kernel per element size.  A lane writes one aligned 16-byte group of the flat output per step; the elements in
// front of the first group and behind the last go one by one (the `head` arrangement of scaled_convert.hip and quality.hip).  A
// group inside one run of one row loads its source in naturally aligned pieces of the widest power of two that divides the source
// address; any other group gathers element by element, stepping to the next run or row as it goes.  A row of one run (crops,
// whole-plane picks) needs no run table at all; otherwise the run of a group's first column is found by binary search in the run
// table and the following runs are reached by stepping (DESIGN.md 6.11 on why not a per-column table).
#include "extract.hpp"

#include <algorithm>
#include <limits>
#include <string>
#include <utility>

namespace fimex_amd {

namespace {

// ---------------------------------------------------------------------------------------------------------------- normalisation
struct Dim {
    uint64_t stride, length, size;                   // source stride in elements, source length, output length
    std::vector<std::pair<uint64_t, uint64_t>> runs;  // (first position, count) of neighbouring positions, ascending
    bool whole() const { return runs.size() == 1 && runs[0].first == 0 && runs[0].second == length; }
};

std::string dim_name(size_t d) { return "dimension " + std::to_string(d); }

Dim checked_dim(const fimex_amd_extract_dim& in, size_t d)
{
    Dim out{0, in.length, in.size, {}};
    FA_REQUIRE(in.length > 0 || in.size == 0, dim_name(d) + " has length 0 and a window of size " + std::to_string(in.size));
    if (in.reduced) {
        FA_REQUIRE(in.nPositions == 0 || in.positions != nullptr, "NULL positions of " + dim_name(d));
        for (size_t i = 0; i < in.nPositions; ++i) {
            FA_REQUIRE(i == 0 || in.positions[i - 1] < in.positions[i],
                       "the positions of " + dim_name(d) + " are not strictly ascending at entry " + std::to_string(i));
            FA_REQUIRE(in.positions[i] < in.length, "position " + std::to_string(in.positions[i]) + " of " + dim_name(d) +
                                                        " is beyond its length " + std::to_string(in.length));
        }
    }
    const size_t limit = in.reduced ? in.nPositions : in.length;
    FA_REQUIRE(in.start <= limit && in.size <= limit - in.start, "the window (" + std::to_string(in.start) + ", " + std::to_string(in.size) +
                                                                     ") of " + dim_name(d) + " is beyond its reduced length " +
                                                                     std::to_string(limit));
    if (in.size == 0) return out;
    if (!in.reduced) {
        out.runs.push_back({in.start, in.size});
        return out;
    }
    for (size_t i = in.start; i < in.start + in.size; ++i) {  // the chunks of :131-145
        const uint64_t p = in.positions[i];
        if (!out.runs.empty() && out.runs.back().first + out.runs.back().second == p) out.runs.back().second++;
        else out.runs.push_back({p, 1});
    }
    return out;
}

}  // namespace

ExtractTables extract_normalise(const fimex_amd_extract_dim* dims, size_t nDims)
{
    FA_REQUIRE(nDims > 0, "no dimensions (nDims == 0)");
    FA_REQUIRE(nDims <= FIMEX_AMD_EXTRACT_MAX_DIMS, "more than " + std::to_string(FIMEX_AMD_EXTRACT_MAX_DIMS) + " dimensions");
    FA_REQUIRE(dims != nullptr, "NULL dimensions");
    ExtractTables t;
    std::vector<Dim> d(nDims);
    size_t inElements = 1, outElements = 1;
    for (size_t i = 0; i < nDims; ++i) {
        d[i] = checked_dim(dims[i], i);
        d[i].stride = inElements;
        FA_REQUIRE(!__builtin_mul_overflow(inElements, dims[i].length, &inElements), "the source holds more elements than size_t counts");
    }
    for (size_t i = 0; i < nDims; ++i) outElements = inElements ? outElements * d[i].size : 0;  // each size <= its length: no overflow
    t.info.inElements = inElements;
    t.info.outElements = outElements;
    if (outElements == 0) return t;

    // D9: joinSlices cuts the fastest reduced dimension with more than one chunk into its chunks and every slower reduced one
    // position by position; a slower dimension that is not reduced stays whole inside each rectangle
    size_t cut = nDims;
    for (size_t i = 0; i < nDims && cut == nDims; ++i)
        if (dims[i].reduced && d[i].runs.size() > 1) cut = i;
    for (size_t i = cut + 1; i < nDims; ++i)
        if (!dims[i].reduced && d[i].size > 1) t.info.referenceOrderDiffers = 1;

    std::vector<Dim> k;
    for (const Dim& x : d) {
        if (x.size == 1) t.base += x.runs[0].first * x.stride;
        else k.push_back(x);
    }
    for (size_t i = 0; i + 1 < k.size();) {
        const Dim& f = k[i];
        Dim& s = k[i + 1];
        if (!f.whole() || s.stride != f.length * f.stride) {
            ++i;
            continue;
        }
        for (auto& r : s.runs) r = {r.first * f.length, r.second * f.length};
        s = Dim{f.stride, f.length * s.length, f.size * s.size, std::move(s.runs)};
        k.erase(k.begin() + (long)i);
    }
    if (k.empty()) k.push_back(Dim{1, 1, 1, {{0, 1}}});  // one element: the base offset says which

    const Dim& f = k[0];
    t.width = f.size;
    uint64_t col = 0;
    for (const auto& r : f.runs) {
        const uint64_t pieces = f.stride == 1 ? 1 : r.second;  // neighbouring positions are neighbours in memory at stride 1 only
        for (uint64_t p = 0; p < pieces; ++p) {
            t.runOut.push_back(col);
            t.runSrc.push_back((r.first + p) * f.stride);
            col += r.second / pieces;
        }
    }
    t.runOut.push_back(col);
    FA_REQUIRE(t.runSrc.size() <= std::numeric_limits<uint32_t>::max(), "more runs in a row than 32 bits count");
    for (size_t i = 1; i < k.size(); ++i) {
        std::vector<uint64_t> off;
        off.reserve(k[i].size);
        for (const auto& r : k[i].runs)
            for (uint64_t p = 0; p < r.second; ++p) off.push_back((r.first + p) * k[i].stride);
        t.slow.push_back(std::move(off));
    }
    t.info.kernelDims = k.size();
    t.info.fastestRuns = t.runSrc.size();
    return t;
}

void build_extract_plan(fimex_amd_extract_plan& plan, const ExtractTables& t)
{
    plan.info = t.info;
    if (t.info.outElements == 0) return;
    std::vector<uint64_t> all(t.runOut);
    all.insert(all.end(), t.runSrc.begin(), t.runSrc.end());
    for (const auto& s : t.slow) all.insert(all.end(), s.begin(), s.end());
    plan.tables.allocate(all.size());
    FA_HIP(hipMemcpy(plan.tables.get(), all.data(), all.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    ExtractArgs& a = plan.args;
    a.base = t.base;
    a.width = t.width;
    a.n = t.info.outElements;
    a.nSlow = (uint32_t)t.slow.size();
    a.nRuns = (uint32_t)t.runSrc.size();
    a.run0 = t.runSrc[0];
    a.runOut = plan.tables.get();
    a.runSrc = a.runOut + t.runOut.size();
    const uint64_t* next = a.runSrc + t.runSrc.size();
    for (size_t i = 0; i < t.slow.size(); ++i) {
        a.size[i] = t.slow[i].size();
        a.off[i] = next;
        next += t.slow[i].size();
    }
}

namespace {

// ----------------------------------------------------------------------------------------------------------------------- kernel
template <typename T>
union Pack {
    uint4 q;
    uint2 d[2];
    uint32_t w[4];
    uint16_t h[8];
    uint8_t b[16];
    T v[16 / sizeof(T)];
};

// the pieces are separate loads for the compiler as well: it may not fuse them into a wider load that is aligned to a piece only
#define FA_KEEP_LOADS_APART() asm volatile("" ::: "memory")

// 16 contiguous source bytes in pieces of the widest power of two that divides their address
template <typename T>
__device__ __forceinline__ void load_pieces(const T* p, Pack<T>& x)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (a % 16 == 0) {
        x.q = *reinterpret_cast<const uint4*>(p);
        return;
    }
    if constexpr (sizeof(T) <= 4) {
        if (a % 8 != 0) {
            if constexpr (sizeof(T) <= 2) {
                if (a % 4 != 0) {
                    if constexpr (sizeof(T) == 1) {
                        if (a % 2 != 0) {
#pragma unroll
                            for (int i = 0; i < 16; ++i) {
                                x.b[i] = reinterpret_cast<const uint8_t*>(p)[i];
                                FA_KEEP_LOADS_APART();
                            }
                            return;
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        x.h[i] = reinterpret_cast<const uint16_t*>(p)[i];
                        FA_KEEP_LOADS_APART();
                    }
                    return;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x.w[i] = reinterpret_cast<const uint32_t*>(p)[i];
                FA_KEEP_LOADS_APART();
            }
            return;
        }
    }
    x.d[0] = reinterpret_cast<const uint2*>(p)[0];
    FA_KEEP_LOADS_APART();
    x.d[1] = reinterpret_cast<const uint2*>(p)[1];
}

// source offset of output row r: one mixed-radix decode into the offset tables
template <typename I>
__device__ __forceinline__ uint64_t row_offset(const ExtractArgs& a, I r)
{
    uint64_t off = a.base;
    for (uint32_t d = 0; d < a.nSlow; ++d) {
        const I s = (I)a.size[d], q = r / s;
        off += a.off[d][r - q * s];
        r = q;
    }
    return off;
}

// an output element and where its source lies; next() steps to the following element without a search
template <typename I, bool kGeneral>
struct Cursor {
    const ExtractArgs& a;
    I r, c;          // row and column
    I runEnd;        // first column behind the run of c
    uint32_t k;      // that run
    uint64_t row;    // source offset of the row
    uint64_t delta;  // source offset of column c inside the row, less c (modulo 2^64)

    __device__ __forceinline__ Cursor(const ExtractArgs& a, I o) : a(a)
    {
        const I w = (I)a.width;
        r = o / w;
        c = o - r * w;
        row = row_offset<I>(a, r);
        if constexpr (kGeneral) {
            uint32_t lo = 0, hi = a.nRuns;  // the last run that starts at or in front of c
            while (hi - lo > 1) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.runOut[mid] <= (uint64_t)c) lo = mid;
                else hi = mid;
            }
            run(lo);
        } else {
            k = 0;
            runEnd = w;
            delta = a.run0;
        }
    }
    __device__ __forceinline__ void run(uint32_t run)
    {
        k = run;
        runEnd = (I)a.runOut[k + 1];
        delta = a.runSrc[k] - a.runOut[k];
    }
    __device__ __forceinline__ uint64_t src() const { return row + delta + c; }
    __device__ __forceinline__ I contiguous() const { return runEnd - c; }
    // never called on the last element of the output: there is no row behind it
    __device__ __forceinline__ void next()
    {
        if (++c < runEnd) return;
        if (c == (I)a.width) {
            c = 0;
            row = row_offset<I>(a, ++r);
            if constexpr (kGeneral) run(0);
        } else if constexpr (kGeneral) {
            run(k + 1);
        }
    }
};

template <typename T, typename I, bool kGeneral>
__global__ void __launch_bounds__(kBlock) extract_kernel(const T* __restrict__ in, T* __restrict__ out, const ExtractArgs a, I head)
{
    constexpr int kPer = 16 / sizeof(T);
    const I n = (I)a.n, groups = (n - head) / kPer;
    const I stride = (I)gridDim.x * kBlock, lane = (I)blockIdx.x * kBlock + threadIdx.x;
    for (I g = lane; g < groups; g += stride) {
        const I o = head + g * kPer;
        Cursor<I, kGeneral> cur(a, o);
        Pack<T> x;
        if (cur.contiguous() >= (I)kPer) {
            load_pieces(in + cur.src(), x);
        } else {
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                x.v[e] = in[cur.src()];
                if (e + 1 < kPer) cur.next();
            }
        }
        *reinterpret_cast<uint4*>(out + o) = x.q;
    }
    const I tail0 = head + groups * kPer, single = head + (n - tail0);
    for (I j = lane; j < single; j += stride) {
        const I i = j < head ? j : tail0 + (j - head);
        const Cursor<I, kGeneral> cur(a, i);
        out[i] = in[cur.src()];
    }
}

template <typename T>
void launch_t(const fimex_amd_extract_plan& plan, const void* d_in, void* d_out, hipStream_t stream)
{
    constexpr size_t kPer = 16 / sizeof(T);
    const ExtractArgs& a = plan.args;
    const size_t n = a.n;
    const size_t head = std::min<size_t>(((16 - reinterpret_cast<uintptr_t>(d_out) % 16) % 16) / sizeof(T), n);
    const size_t groups = (n - head) / kPer, single = n - groups * kPer;
    const size_t want = ceil_div(std::max(groups, single), kBlock);
    const size_t cap = (size_t)std::max(1, tuning("EXTRACT_MAX_BLOCKS", 256 * 8));
    const unsigned blocks = (unsigned)std::min(want, cap);
    const bool general = a.nRuns > 1 || tuning("EXTRACT_GENERAL", 0) != 0;
    const bool narrow = n < (size_t(1) << 31);  // every index, a lane's last stride included, stays below 2^32
    const T* in = static_cast<const T*>(d_in);
    T* out = static_cast<T*>(d_out);
    if (narrow && general) extract_kernel<T, uint32_t, true><<<blocks, kBlock, 0, stream>>>(in, out, a, (uint32_t)head);
    else if (narrow) extract_kernel<T, uint32_t, false><<<blocks, kBlock, 0, stream>>>(in, out, a, (uint32_t)head);
    else if (general) extract_kernel<T, uint64_t, true><<<blocks, kBlock, 0, stream>>>(in, out, a, (uint64_t)head);
    else extract_kernel<T, uint64_t, false><<<blocks, kBlock, 0, stream>>>(in, out, a, (uint64_t)head);
    FA_HIP(hipGetLastError());
}

}  // namespace

void launch_extract(const fimex_amd_extract_plan& plan, const void* d_in, size_t elem, void* d_out, hipStream_t stream)
{
    switch (elem) {
    case 1: launch_t<uint8_t>(plan, d_in, d_out, stream); break;
    case 2: launch_t<uint16_t>(plan, d_in, d_out, stream); break;
    case 4: launch_t<uint32_t>(plan, d_in, d_out, stream); break;
    default: launch_t<uint64_t>(plan, d_in, d_out, stream); break;
    }
}

}  // namespace fimex_amd
