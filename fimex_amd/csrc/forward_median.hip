// Forward-mapping regrid: the median of medium buckets (a source finer than the target), one wave per target cell.  Two forms: by selection on keys (the product's), by ranks (the form before it, which
// the tuning build still reaches).  The order both follow, the keys and the selection loop are forward_math.hpp's.
#include "forward.hpp"

namespace fimex_amd {

namespace {

// What the two forms share: the bucket's cells in Q registers per lane (position q * 64 + lane of its scan order), read once; per slice
// their values, which of them the aggregate keeps, and the undefined results.  median(lane, v, kept, want, o) stores to o the value of
// rank `want` = size() / 2 among the kept ones.
template <bool UNDEF, int Q, class Median>
__device__ __forceinline__ void median_per_wave(const FwdArgs& a, Median median)
{
    WaveTarget w;
    if (!wave_target(a, w)) return;
    uint32_t idx[Q];
    bool has[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const uint32_t p = (uint32_t)q * kWave + w.lane;
        has[q] = p < w.len;
        idx[q] = has[q] ? a.src[w.b + p] : 0u;
    }
    for (uint32_t z = w.z0; z < w.z1; ++z) {
        const float* src = a.in + (size_t)z * a.inLayer;
        float v[Q];
        bool kept[Q];
        bool nanHere = false;
        uint32_t n = 0;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            v[q] = has[q] ? src[idx[q]] : 0.f;
            kept[q] = has[q] && keep<UNDEF>(v[q]);
            nanHere = nanHere || (has[q] && isnan(v[q]));
            n += (uint32_t)__popcll(__ballot(kept[q]));
        }
        float* o = a.out + (size_t)z * a.nOut + w.t;
        if (median_defined<UNDEF>(n, __ballot(nanHere) != 0)) median(w.lane, v, kept, n / 2, o);
        else if (w.lane == 0) *o = undefined_f();
    }
}

// Median of buckets of up to 64 * Q source cells, one wave per target cell: the bucket's values of one slice sit in Q registers per
// lane (position q * 64 + lane of the bucket's scan order), every kept value is broadcast once (v_readlane) and every lane counts,
// for its own values, how many kept values are smaller or equal-and-earlier -- its rank in the order std::nth_element's result
// follows (src/CachedForwardInterpolation.cc:49-53).  The one value of rank size() / 2 is the median; its lane stores it.
// n * Q comparisons per lane instead of the n * n loads of median_by_rank: 0.1-degree global -> 1-degree global (100 cells per
// bucket), 100 slices: 130 ms -> see DESIGN.md 6.
template <bool UNDEF, int Q>
__global__ void __launch_bounds__(kBlock) forward_apply_median_wave(FwdArgs a)
{
    median_per_wave<UNDEF, Q>(a, [](uint32_t lane, const float (&v)[Q], const bool (&kept)[Q], uint32_t want, float* o) __attribute__((always_inline)) {
        uint32_t rank[Q] = {};
#pragma unroll
        for (int q2 = 0; q2 < Q; ++q2) {
            unsigned long long m = __ballot(kept[q2]);  // wave-uniform: the loop below runs on the scalar unit
            while (m) {
                const int l = __ffsll((long long)m) - 1;
                m &= m - 1;
                const float u = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[q2]), l));
                const uint32_t pu = (uint32_t)q2 * kWave + (uint32_t)l;
#pragma unroll
                for (int q = 0; q < Q; ++q) rank[q] += precedes(u, pu, v[q], (uint32_t)q * kWave + lane) ? 1u : 0u;
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if (kept[q] && rank[q] == want) *o = v[q];  // exactly one value of the bucket has this rank
    });
}

// The same median by SELECTION instead of ranking: the kept values of a bucket, as keys whose unsigned order is the floats' order,
// sit in Q registers per lane; the key of rank size() / 2 is built bit by bit from the top -- "how many keys lie below the candidate?"
// is one comparison per register, whose result IS the ballot, a population count and a scalar decision: 32 rounds of Q vector and a
// handful of scalar instructions, whatever the bucket's length (ranking: one broadcast and 2 Q comparisons per VALUE; 100 cells per
// bucket, 100 slices: 13.1 ms -> see DESIGN.md 6).  The value comes back out of the key.  Only +0.0 and -0.0 compare equal without
// being the same bits: they share a key, and where the median is a zero, the order the reference's result follows ("less, or equal
// and earlier", src/CachedForwardInterpolation.cc:49-53) picks among the bucket's zeros by position.
template <bool UNDEF, int Q>
__global__ void __launch_bounds__(kBlock) forward_apply_median_select(FwdArgs a)
{
    median_per_wave<UNDEF, Q>(a, [](uint32_t lane, const float (&v)[Q], const bool (&kept)[Q], uint32_t want, float* o) __attribute__((always_inline)) {
        uint32_t key[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) key[q] = median_key(v[q], kept[q]);
        const uint32_t K = select_key(want, [&](uint32_t T) __attribute__((always_inline)) {
            uint32_t below = 0;
#pragma unroll
            for (int q = 0; q < Q; ++q) below += (uint32_t)__popcll(__ballot(key[q] < T));
            return below;
        });
        uint32_t bits = median_key_bits(K);
        if (K == kZeroKey) {
            // the median is a zero: the (want - #negative values)-th of the bucket's zeros in scan order supplies the sign
            uint32_t k = want;
#pragma unroll
            for (int q = 0; q < Q; ++q) k -= (uint32_t)__popcll(__ballot(key[q] < kZeroKey));
            bool found = false;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                unsigned long long m = __ballot(key[q] == kZeroKey);
                const uint32_t c = (uint32_t)__popcll(m);
                if (!found && k < c) {
                    for (uint32_t i = 0; i < k; ++i) m &= m - 1;
                    bits = (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v[q]), __ffsll((long long)m) - 1);
                    found = true;
                } else if (!found) {
                    k -= c;
                }
            }
        }
        if (lane == 0) *o = __uint_as_float(bits);
    });
}

}  // namespace

// by the plan's longest bucket: Q = 1 / 2 / 4 registers of values per lane
void launch_forward_median_wave(const FwdArgs& a, size_t maxBucket, bool undef, uint32_t chunks, hipStream_t stream)
{
    const dim3 g = wave_grid(a, chunks);
    const bool select = tuning("FWD_MEDIAN_SELECT", 1) != 0;  // 0: ranks by broadcast (the form before it)
    with_undef(undef, [&](auto u) {
        constexpr bool U = decltype(u)::value;
        if (maxBucket <= 64 && select) forward_apply_median_select<U, 1><<<g, kBlock, 0, stream>>>(a);
        else if (maxBucket <= 128 && select) forward_apply_median_select<U, 2><<<g, kBlock, 0, stream>>>(a);
        else if (maxBucket <= 128) forward_apply_median_wave<U, 2><<<g, kBlock, 0, stream>>>(a);
        else if (select) forward_apply_median_select<U, 4><<<g, kBlock, 0, stream>>>(a);
        else forward_apply_median_wave<U, 4><<<g, kBlock, 0, stream>>>(a);
    });
}

}  // namespace fimex_amd
