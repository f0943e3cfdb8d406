// Host shim of fimex_amd/csrc/forward_math.hpp for tests/test_forward_math_host.py: the header the forward kernels compile, evaluated
// on the CPU the way the kernels use it.  Buckets are values[offsets[i] .. offsets[i + 1]) in push order; one entry point per form
// of the rules.  Built for the host only by fimex_amd/build.py (hipcc --cuda-host-only -ffp-contract=off); needs no GPU.
#include "forward_math.hpp"

using namespace fimex_amd;

namespace {

constexpr uint32_t kGroup = 8;  // forward_tiled.hip walks a bucket eight steps at a time (kFtGroup)

template <class F>
void each_bucket(const uint32_t* offsets, int64_t nBuckets, float* out, F&& f)
{
    for (int64_t i = 0; i < nBuckets; ++i) out[i] = f(offsets[i], offsets[i + 1] - offsets[i]);
}

}  // namespace

#define BUCKET_ARGS const float* values, const uint32_t* offsets, int64_t nBuckets, float* out

// the lane kernels and the tiled kernel's tiles that are not staged; 0: done, -1: no such aggregate (the median has entries of its own)
extern "C" int forward_math_ordered(int aggregate, int undef, BUCKET_ARGS)
{
    return with_aggregate((Aggregate)aggregate, undef != 0, [&](auto A, auto U) {
        each_bucket(offsets, nBuckets, out, [&](uint32_t b, uint32_t len) {
            float acc = 0.f;
            uint32_t cnt = 0;
            for (uint32_t j = 0; j < len; ++j) ordered_step<A(), U()>(values[b + j], acc, cnt);
            return finish<A(), U()>(acc, cnt, cnt, false);
        });
    }) ? 0 : -1;
}

// the tiled kernel's staged tiles: a bucket padded to whole groups with the padding value, firstNan from its first element
extern "C" int forward_math_padded(int aggregate, int undef, BUCKET_ARGS)
{
    return with_aggregate((Aggregate)aggregate, undef != 0, [&](auto A, auto U) {
        each_bucket(offsets, nBuckets, out, [&](uint32_t b, uint32_t len) {
            const auto at = [&](uint32_t j) { return j < len ? values[b + j] : padding_value<A(), U()>(); };
            float acc = start_value<A(), U()>();
            uint32_t cnt = 0;
            const bool firstNan = len != 0 && is_nan(at(0));
            for (uint32_t j = 0; j < (len + kGroup - 1) / kGroup * kGroup; ++j) take<A(), U()>(at(j), acc, cnt);
            return finish<A(), U()>(acc, cnt, len, firstNan);
        });
    }) ? 0 : -1;
}

extern "C" void forward_math_median_by_rank(int undef, BUCKET_ARGS)
{
    with_undef(undef != 0, [&](auto U) {
        each_bucket(offsets, nBuckets, out, [&](uint32_t b, uint32_t len) { return median_by_rank<U()>(len, [&](uint32_t j) { return values[b + j]; }); });
    });
}

// buckets of at most two values (longer ones: NaN)
extern "C" void forward_math_median_of_two(int undef, BUCKET_ARGS)
{
    with_undef(undef != 0, [&](auto U) {
        each_bucket(offsets, nBuckets, out, [&](uint32_t b, uint32_t len) {
            float acc = 0.f;
            uint32_t cnt = 0;
            bool anyNan = false;
            for (uint32_t j = 0; j < len; ++j) median_of_two_step<U()>(values[b + j], acc, cnt, anyNan);
            return len <= 2 ? median_of_two_finish<U()>(acc, cnt, anyNan) : undefined_f();
        });
    });
}

// the selection kernel's median: the value out of the selected key, and the key itself (kDroppedKey where the median is undefined)
extern "C" void forward_math_median_select(int undef, BUCKET_ARGS, uint32_t* keys)
{
    with_undef(undef != 0, [&](auto U) {
        for (int64_t i = 0; i < nBuckets; ++i) {
            const float* v = values + offsets[i];
            const uint32_t len = offsets[i + 1] - offsets[i];
            uint32_t n = 0;
            bool anyNan = false;
            for (uint32_t j = 0; j < len; ++j) { n += keep<U()>(v[j]) ? 1u : 0u; anyNan = anyNan || is_nan(v[j]); }
            keys[i] = kDroppedKey;
            out[i] = undefined_f();
            if (!median_defined<U()>(n, anyNan)) continue;
            keys[i] = select_key(n / 2, [&](uint32_t T) {
                uint32_t below = 0;
                for (uint32_t j = 0; j < len; ++j) below += median_key(v[j], keep<U()>(v[j])) < T ? 1u : 0u;
                return below;
            });
            out[i] = __builtin_bit_cast(float, median_key_bits(keys[i]));
        }
    });
}

extern "C" void forward_math_keys(const float* values, int64_t n, uint32_t* keys, uint32_t* bits)
{
    for (int64_t i = 0; i < n; ++i) { keys[i] = median_key(values[i], true); bits[i] = median_key_bits(keys[i]); }
}

extern "C" void forward_math_targets(const double* px, const double* py, int64_t n, int64_t outX, int64_t outY, int64_t* rx, uint32_t* tgt)
{
    for (int64_t i = 0; i < n; ++i) { rx[i] = round_clamp(px[i], outX); tgt[i] = forward_target(px[i], py[i], outX, outY); }
}
