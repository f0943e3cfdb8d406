// Stand-alone run of the forward aggregation rules on the CPU, for a sanitizer build:
//
//   hipcc --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Ifimex_amd/csrc tests/forward_math_host_main.hip tests/forward_math_host.hip -o forward_math_host_main
//   ./forward_math_host_main
//
// Sends buckets of the lengths tests/test_forward_math_host.py uses -- NaNs, zeros of both signs, infinities and equal values among
// them, in arrays of exactly the buckets' size -- through every entry point of the shim once and prints how many results were
// defined.  Not run by pytest and not loaded into Python.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#define BUCKET_ARGS const float* values, const uint32_t* offsets, int64_t nBuckets, float* out
extern "C" int forward_math_ordered(int aggregate, int undef, BUCKET_ARGS);
extern "C" int forward_math_padded(int aggregate, int undef, BUCKET_ARGS);
extern "C" void forward_math_median_by_rank(int undef, BUCKET_ARGS);
extern "C" void forward_math_median_of_two(int undef, BUCKET_ARGS);
extern "C" void forward_math_median_select(int undef, BUCKET_ARGS, uint32_t* keys);
extern "C" void forward_math_keys(const float* values, int64_t n, uint32_t* keys, uint32_t* bits);
extern "C" void forward_math_targets(const double* px, const double* py, int64_t n, int64_t outX, int64_t outY, int64_t* rx, uint32_t* tgt);

int main()
{
    const uint32_t lengths[] = {0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 100, 129};
    const float kinds[] = {1.5f, -0.0f, 0.0f, NAN, 1.5f, -2.f, INFINITY, 1e-42f, -INFINITY, 281.5f, 0.0f};
    std::vector<uint32_t> offsets{0};
    for (uint32_t len : lengths) offsets.push_back(offsets.back() + len);
    const int64_t nb = (int64_t)offsets.size() - 1;
    std::vector<float> values(offsets.back()), out(nb);
    std::vector<uint32_t> keys(nb);
    long defined = 0, calls = 0;
    auto count = [&] { ++calls; for (float r : out) defined += r == r; };
    for (uint32_t shift = 0; shift < 11; ++shift) {
        for (size_t i = 0; i < values.size(); ++i) values[i] = kinds[(i * 7 + shift) % 11];
        for (int undef = 0; undef < 2; ++undef) {
            for (int aggregate = 0; aggregate < 5; ++aggregate) {
                if (forward_math_ordered(aggregate, undef, values.data(), offsets.data(), nb, out.data()) == 0) count();
                if (forward_math_padded(aggregate, undef, values.data(), offsets.data(), nb, out.data()) == 0) count();
            }
            forward_math_median_by_rank(undef, values.data(), offsets.data(), nb, out.data()); count();
            forward_math_median_of_two(undef, values.data(), offsets.data(), nb, out.data()); count();
            forward_math_median_select(undef, values.data(), offsets.data(), nb, out.data(), keys.data()); count();
        }
    }
    std::vector<uint32_t> k(values.size()), bits(values.size());
    forward_math_keys(values.data(), (int64_t)values.size(), k.data(), bits.data());
    const std::vector<double> pos{NAN, INFINITY, -INFINITY, 1e300, -1e300, -0.5, 0.5, 6.5, 6.4999999, 1073741824.0, -1073741824.0, 4294967296.0, 3.0};
    std::vector<int64_t> rx(pos.size());
    std::vector<uint32_t> tgt(pos.size());
    forward_math_targets(pos.data(), pos.data(), (int64_t)pos.size(), 7, 7, rx.data(), tgt.data());
    std::printf("%ld calls, %ld defined results of %ld\n", calls, defined, calls * (long)nb);
    return 0;
}
