// A series onto a new time axis: CDMTimeInterpolator::getDataSlice (src/CDMTimeInterpolator.cc:88-136) for every
// output step in one pass.  Per step the result is mifi_get_values_linear_weak_extrapol_f (src/interpolation.c:1085-1109) on
// Data::asFloat() of the two input slices: a static_cast per element, no scale, no fill value handling, as in the reference.
//
// The blend factor f and the branch it selects (copy A, copy B, blend, undefined) are wave-uniform and known on the host, so they
// arrive as kernel arguments: kLaunchSteps output steps per launch, nothing is copied to the device and nothing waits for the
// stream.  A lane owns four output cells (16 bytes of every output slice) and walks the steps of the launch.  It holds the two
// input values of the current pair in registers and writes every step of that pair from them; where the next pair starts at this
// pair's second slice, B moves over to A and one slice is loaded.  A new axis that never runs backwards therefore reads every
// input slice once per launch, and the first pair of a launch once more.  The groups start `head` cells into a slice, where
// the output is 16-byte aligned and the input as far as four elements need; the cells in front and behind the last whole group go
// one by one, and so does everything where the slices are no multiple of four cells long (they would start at other alignments).
// Where the cells alone cannot fill the chip, gridDim.y splits a launch at chunks of kChunkSteps steps; every chunk then loads its
// own first pair.  No LDS, no scratch; the grid is capped and strides.
#include "plan.hpp"

#include <algorithm>

namespace fimex_amd {

namespace {

constexpr int kLaunchSteps = FIMEX_AMD_TIME_LAUNCH_STEPS, kChunkSteps = FIMEX_AMD_TIME_CHUNK_STEPS;
constexpr size_t kComputeUnits = 256;

struct StepBlock {  // 16 bytes per step of kernel arguments, every one of them read by scalar loads
    uint32_t t1[kLaunchSteps], t2[kLaunchSteps];
    float f[kLaunchSteps];
    uint32_t cls[kLaunchSteps];
};

template <typename T, int V>
struct alignas(V * sizeof(T) < 16 ? V * sizeof(T) : 16) Stored {
    T v[V];
};

template <int V>
struct alignas(V * sizeof(float)) Floats {
    float v[V];
};

template <typename T, int V>
__device__ __forceinline__ Floats<V> load_as_float(const T* p)
{
    const Stored<T, V> x = *reinterpret_cast<const Stored<T, V>*>(p);
    Floats<V> r;
#pragma unroll
    for (int e = 0; e < V; ++e) r.v[e] = (float)x.v[e];  // Data::asFloat(), include/fimex/Utils.h:94-116
    return r;
}

// output steps [s0, s1) of this launch for the V cells from `cell` on; out points at the first output slice of the launch
template <typename T, int V>
__device__ __forceinline__ void walk(const T* __restrict__ in, float* __restrict__ out, size_t n, size_t cell, const StepBlock& sb, int s0, int s1)
{
    Floats<V> A{}, B{};
    uint32_t curT1 = 0, curT2 = 0;
    for (int s = s0; s < s1; ++s) {
        const uint32_t t1 = sb.t1[s], t2 = sb.t2[s];
        if (s == s0 || t1 != curT1 || t2 != curT2) {
            if (s != s0 && t1 == curT2) A = B;
            else A = load_as_float<T, V>(in + (size_t)t1 * n + cell);
            B = t2 == t1 ? A : load_as_float<T, V>(in + (size_t)t2 * n + cell);
            curT1 = t1;
            curT2 = t2;
        }
        const float f = sb.f[s];
        Floats<V> y;
        switch ((TimeStepClass)sb.cls[s]) {  // wave-uniform: a scalar branch around the vector loops
        case TimeStepClass::CopyA: y = A; break;  // the reference's memcpy: no 0 * NaN from the other slice (:1088-1093)
        case TimeStepClass::CopyB: y = B; break;
        case TimeStepClass::Blend:
#pragma unroll
            for (int e = 0; e < V; ++e) y.v[e] = blend_math::value(TimeStepClass::Blend, f, A.v[e], B.v[e]);  // :1045
            break;
        default:
#pragma unroll
            for (int e = 0; e < V; ++e) y.v[e] = undefined_f();  // :1100
        }
        *reinterpret_cast<Floats<V>*>(out + (size_t)s * n + cell) = y;
    }
}

template <typename T>
__global__ void __launch_bounds__(kBlock) time_kernel(const T* __restrict__ in, float* __restrict__ out, size_t n, size_t head,
                                                      const StepBlock sb, int steps)
{
    int s0 = 0, s1 = steps;
    if (gridDim.y > 1) {
        s0 = (int)blockIdx.y * kChunkSteps;
        s1 = s0 + kChunkSteps < steps ? s0 + kChunkSteps : steps;
    }
    const size_t stride = (size_t)gridDim.x * kBlock, lane = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t groups = (n - head) / 4;
    for (size_t g = lane; g < groups; g += stride) walk<T, 4>(in, out, n, head + 4 * g, sb, s0, s1);
    const size_t tail0 = head + groups * 4, single = head + (n - tail0);
    for (size_t j = lane; j < single; j += stride) walk<T, 1>(in, out, n, j < head ? j : tail0 + (j - head), sb, s0, s1);
}

// cells in front of the first group of four; n where the slices do not all start at the alignment of the first
template <typename T>
size_t head_cells(const T* in, const float* out, size_t n)
{
    if (n % 4) return n;
    constexpr size_t inAlign = alignof(Stored<T, 4>);
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), o0 = reinterpret_cast<uintptr_t>(out);
    for (size_t h = 0; h < 16 && h < n; ++h)
        if ((i0 + h * sizeof(T)) % inAlign == 0 && (o0 + h * sizeof(float)) % 16 == 0) return h;
    return n;
}

template <typename T>
void launch_typed(const T* in, size_t n, const TimeStep* steps, size_t nNew, float* out, hipStream_t stream)
{
    const size_t head = head_cells(in, out, n), groups = (n - head) / 4, single = n - groups * 4;
    const size_t want = ceil_div(groups > single ? groups : single, kBlock);
    const size_t cap = std::max(1, tuning("TIME_MAX_BLOCKS", 256 * 8));
    // 0: split the steps over gridDim.y where the cells leave compute units without two workgroups, 1: always, 2: never
    const int splitMode = tuning("TIME_SPLIT_Y", 0);
    const bool split = splitMode == 1 || (splitMode != 2 && want < 2 * kComputeUnits);
    for (size_t first = 0; first < nNew; first += kLaunchSteps) {
        const int len = (int)std::min<size_t>(kLaunchSteps, nNew - first);
        StepBlock sb{};
        for (int s = 0; s < len; ++s) {
            const TimeStep& st = steps[first + s];
            sb.t1[s] = st.t1;
            sb.t2[s] = st.t2;
            sb.f[s] = st.f;
            sb.cls[s] = (uint32_t)st.cls;
        }
        const dim3 grid((unsigned)(want < cap ? want : cap), split ? (unsigned)ceil_div(len, kChunkSteps) : 1u);
        time_kernel<T><<<grid, kBlock, 0, stream>>>(in, out + first * n, n, head, sb, len);
        FA_HIP(hipGetLastError());
    }
}

}  // namespace

// every argument has been checked (capi_time_quality.hip); n > 0 and nNew > 0, every t1 and t2 below the number of input slices
void launch_time_interpolate(const void* d_in, int cdmType, size_t n, const TimeStep* h_steps, size_t nNew, float* d_out, hipStream_t stream)
{
    for_cdm_type(cdmType, [&](auto v) {
        using T = decltype(v);
        launch_typed<T>(static_cast<const T*>(d_in), n, h_steps, nNew, d_out, stream);
    });
}

}  // namespace fimex_amd
