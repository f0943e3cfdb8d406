// The reference's forward aggregation rules (src/CachedForwardInterpolation.cc:38-59), stated once: what one value of a bucket does
// to the running result in push order, how a bucket is finished, the order the median follows, and which target cell a source cell
// falls into.  Every forward kernel (forward.hip, forward_median.hip, forward_tiled.hip, forward_plan.hip) takes them from here, and
// so does the host shim of tests/test_forward_math_host.py, which checks this file against the reference's results on the CPU, without a GPU:
// everything is __host__ __device__ and free of device builtins.  Compiled with -ffp-contract=off.
#pragma once

#include "plan.hpp"

#include <cmath>
#include <type_traits>

#define FA_HD __host__ __device__ __forceinline__

namespace fimex_amd {

// RoundAndClamp(0, n-1, -1), src/Utils.cc:42-58 (round(): half away from zero)
FA_HD int64_t round_clamp(double d, int64_t n)
{
    if (!(fabs(d) < 1073741824.0)) return -1;  // NaN / inf / beyond int: invalid
    const int64_t r = (int64_t)round(d);
    return (r >= 0 && r < n) ? r : -1;
}
// target cell of a source cell, src/CachedForwardInterpolation.cc:72-73 + :104-107
FA_HD uint32_t forward_target(double px, double py, int64_t outX, int64_t outY)
{
    const int64_t tx = round_clamp(px, outX), ty = round_clamp(py, outY);
    return (tx >= 0 && ty >= 0) ? (uint32_t)(ty * outX + tx) : kInvalidPos;
}

FA_HD bool is_nan(float v) { return v != v; }
template <bool UNDEF>
FA_HD bool keep(float v) { return UNDEF || !is_nan(v); }

constexpr bool is_sum(Aggregate a) { return a == Aggregate::Sum || a == Aggregate::Mean; }
// std::max_element / std::min_element: v replaces the running extremum only where it is strictly beyond it -- the first of equal
// elements stays, and a NaN on either side never wins
template <Aggregate A>
FA_HD bool beats(float v, float acc) { return A == Aggregate::Max ? acc < v : v < acc; }

// ---- the ordered step: "the first kept value" form (the lane kernels, the tiled kernel's tiles that are not staged) ----------------
// one value of a bucket in push order; acc and cnt start from 0
template <Aggregate A, bool UNDEF>
FA_HD void ordered_step(float v, float& acc, uint32_t& cnt)
{
    if (keep<UNDEF>(v)) {
        if (is_sum(A)) acc = acc + v;                      // std::accumulate(.., 0.f)
        else if (cnt == 0 || beats<A>(v, acc)) acc = v;    // a leading NaN sticks
        cnt++;
    }
}
// its finish is the padded step's below, finish<A, UNDEF>(acc, cnt, cnt, false): every kept value was counted, and a leading NaN is in acc

// a NaN inside an "undef" bucket: the reference's nth_element result is implementation-defined (comparator not a strict weak
// order); the documented intent (value + undef = undef) is kept.  n: the bucket's kept values
template <bool UNDEF>
FA_HD bool median_defined(uint32_t n, bool anyNan) { return n != 0 && !(UNDEF && anyNan); }

// The median of a bucket of at most two source cells, a running form of it: rank size()/2 of one value is the value, of two the larger
// one -- the second where they compare equal, which is what counting "less, or equal and earlier" picks (:49-53).
template <bool UNDEF>
FA_HD void median_of_two_step(float v, float& acc, uint32_t& cnt, bool& anyNan)
{
    if (keep<UNDEF>(v)) {
        if (UNDEF && is_nan(v)) anyNan = true;
        if (cnt == 0 || !(acc > v)) acc = v;
        cnt++;
    }
}
template <bool UNDEF>
FA_HD float median_of_two_finish(float acc, uint32_t cnt, bool anyNan) { return median_defined<UNDEF>(cnt, anyNan) ? acc : undefined_f(); }

// ---- the padded step (forward_tiled.hip's staged tiles), and the finish of every fold -----------------------------------------------
// One value of a bucket in scan order.  The arithmetic of ordered_step with nothing to decide per step beyond it: steps past the end
// of a lane's bucket read the slot's padding cell, whose value leaves the
// result alone (NaN where NaNs are skipped or never win a comparison; -0.0 for the sums that keep NaNs: x + -0.0 == x for every x,
// signed zeros included), and the kinds that keep undefined values know their count (the bucket's length) without counting.
//   max / min start from -inf / +inf instead of "the first kept value": a comparison with the first value then takes it, or leaves
//   an equal infinity -- the same value; a NaN in first place (kept by the "undef" kinds: std::max_element returns it) is looked at
//   separately (firstNan).
template <Aggregate A, bool UNDEF>
FA_HD void take(float v, float& acc, uint32_t& cnt)
{
    if (is_sum(A)) {
        if (UNDEF) acc = acc + v;                           // std::accumulate(.., 0.f), NaNs included
        else { const bool ok = v == v; acc = ok ? acc + v : acc; cnt += ok ? 1u : 0u; }
    } else {
        acc = beats<A>(v, acc) ? v : acc;
        if (!UNDEF) cnt += (v == v) ? 1u : 0u;
    }
}
template <Aggregate A, bool UNDEF>
FA_HD float start_value() { return (A == Aggregate::Max) ? -INFINITY : (A == Aggregate::Min) ? INFINITY : 0.f; }
template <Aggregate A, bool UNDEF>
FA_HD float padding_value() { return (is_sum(A) && UNDEF) ? -0.f : undefined_f(); }
// len: the bucket's length (what the "undef" kinds divide by); cnt: the kept values the others counted
template <Aggregate A, bool UNDEF>
FA_HD float finish(float acc, uint32_t cnt, uint32_t len, bool firstNan)
{
    const uint32_t n = UNDEF ? len : cnt;
    if (n == 0) return undefined_f();                        // empty bucket, src/CachedForwardInterpolation.cc:123-124
    if (!is_sum(A) && UNDEF && firstNan) return undefined_f();  // max / min
    return A == Aggregate::Mean ? acc / (float)n : acc;      // aggrMean: sum / size()
}

// ---- the median (std::nth_element at size()/2, :49-53) --------------------------------------------------------------------------------
// the order its result follows: less, or equal and earlier in the bucket
FA_HD bool precedes(float u, uint32_t posU, float v, uint32_t posV) { return u < v || (u == v && posU < posV); }

// value of rank size()/2 among the kept values of one bucket of one slice, by rank counting; at(j): the bucket's j-th value in push order
template <bool UNDEF, class At>
FA_HD float median_by_rank(uint32_t len, At at)
{
    uint32_t n = 0;
    bool anyNan = false;
    for (uint32_t j = 0; j < len; ++j) {
        const float v = at(j);
        if (is_nan(v)) anyNan = true;
        if (keep<UNDEF>(v)) n++;
    }
    float r = undefined_f();
    if (median_defined<UNDEF>(n, anyNan)) {
        const uint32_t want = n / 2;
        for (uint32_t j = 0; j < len; ++j) {
            const float v = at(j);
            if (!keep<UNDEF>(v)) continue;
            uint32_t rank = 0;
            for (uint32_t q = 0; q < len; ++q) {
                const float w = at(q);
                if (keep<UNDEF>(w)) rank += precedes(w, q, v, j) ? 1u : 0u;
            }
            if (rank == want) { r = v; break; }
        }
    }
    return r;
}

// The median by selection: kept values as keys whose unsigned order is the floats' order.  Only +0.0 and -0.0 compare equal without
// being the same bits: they share a key (the caller picks among a bucket's zeros by position); dropped values lie above every kept one.
constexpr uint32_t kZeroKey = 0x80000000u, kDroppedKey = 0xFFFFFFFFu;
FA_HD uint32_t median_key(float v, bool kept)
{
    const uint32_t bits = __builtin_bit_cast(uint32_t, v);
    const uint32_t ordered = bits ^ (((int32_t)bits < 0) ? 0xFFFFFFFFu : 0x80000000u);  // unsigned order = float order
    return !kept ? kDroppedKey : (v == 0.f ? kZeroKey : ordered);
}
// bits of the value a key stands for (kZeroKey: +0.0)
FA_HD uint32_t median_key_bits(uint32_t K) { return (K & 0x80000000u) ? (K ^ 0x80000000u) : ~K; }
// the key of rank `want`, bit by bit from the top: the largest candidate with at most `want` keys below it; below(T): how many keys are < T
template <class Below>
FA_HD uint32_t select_key(uint32_t want, Below below)
{
    uint32_t K = 0;
#pragma unroll
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t T = K | (1u << bit);
        K = (below(T) <= want) ? T : K;
    }
    return K;
}

// ---- dispatch: f(aggregate, undef) with both as compile-time constants (std::integral_constant) -----------------------------------------
template <class F>
void with_undef(bool undef, F&& f) { undef ? f(std::true_type{}) : f(std::false_type{}); }
// false: the median, whose kernels are chosen on their own (forward_median.hip)
template <class F>
bool with_aggregate(Aggregate a, bool undef, F&& f)
{
    switch (a) {
    case Aggregate::Sum: with_undef(undef, [&](auto u) { f(std::integral_constant<Aggregate, Aggregate::Sum>{}, u); }); return true;
    case Aggregate::Mean: with_undef(undef, [&](auto u) { f(std::integral_constant<Aggregate, Aggregate::Mean>{}, u); }); return true;
    case Aggregate::Max: with_undef(undef, [&](auto u) { f(std::integral_constant<Aggregate, Aggregate::Max>{}, u); }); return true;
    case Aggregate::Min: with_undef(undef, [&](auto u) { f(std::integral_constant<Aggregate, Aggregate::Min>{}, u); }); return true;
    default: return false;
    }
}

}  // namespace fimex_amd
