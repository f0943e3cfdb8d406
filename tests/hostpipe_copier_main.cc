// ParallelCopier of fimex_amd/csrc/hostpipe_layout.hpp as a program of its own: tests/test_hostpipe_layout.py builds it with the
// host compiler, once with the thread sanitizer and once with the address and undefined-behaviour sanitizers, and runs it on the
// CPU.  Every copy goes from a patterned source into a destination with guard bytes on both sides; exit status 0 and the last
// line "copier ok" where every copy arrived whole and no guard byte changed.
//
// With up to 8 parts no length of 1 MiB or more leaves a part empty (that needs bytes < 4096 * parts * (parts - 1)), so the
// length whose rounded share leaves the last parts empty also runs on 31 workers, a count HOST_COPY_THREADS can ask for: there
// 1 MiB + 4097 bytes go in shares of 36864, and parts 29, 30 and the caller's own part 31 have nothing to copy.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hostpipe_layout.hpp"

using fimex_amd::hostpipe::ParallelCopier;

namespace {

constexpr size_t kMiB = (size_t)1 << 20;
constexpr size_t kGuard = 4096;
constexpr unsigned char kGuardByte = 0xA5, kStale = 0xCC;

int g_failures = 0;

unsigned char pattern(size_t i) { return (unsigned char)((i * 2654435761u) >> 11 ^ i >> 20); }

struct Buffers {
    explicit Buffers(size_t most) : src(most + 1024), dst(most + 2 * kGuard)
    {
        for (size_t i = 0; i < src.size(); ++i) src[i] = pattern(i);
    }
    std::vector<unsigned char> src, dst;
};

// one copy of `bytes` from src + shift; the shift makes a copy left over from the call before visible
void check_copy(ParallelCopier& c, Buffers& b, size_t bytes, size_t shift, int workers, const char* what)
{
    std::memset(b.dst.data(), kGuardByte, kGuard);
    std::memset(b.dst.data() + kGuard, kStale, bytes);
    std::memset(b.dst.data() + kGuard + bytes, kGuardByte, kGuard);
    c.copy(b.dst.data() + kGuard, b.src.data() + shift, bytes);
    bool ok = bytes == 0 || std::memcmp(b.dst.data() + kGuard, b.src.data() + shift, bytes) == 0;
    for (size_t i = 0; i < kGuard; ++i) ok = ok && b.dst[i] == kGuardByte && b.dst[kGuard + bytes + i] == kGuardByte;
    if (!ok) {
        size_t at = 0;
        while (at < bytes && b.dst[kGuard + at] == b.src[shift + at]) ++at;
        std::printf("FAILED: %s, %d workers, %zu bytes, shift %zu: first wrong byte %zu of %zu (or a guard byte)\n", what, workers, bytes, shift, at, bytes);
        ++g_failures;
    }
}

}  // namespace

int main()
{
    const size_t lengths[] = {0, 1, kMiB - 1, kMiB, kMiB + 1, kMiB + 4097, 3 * kMiB + 12345, 64 * kMiB};
    Buffers b(64 * kMiB);
    for (int workers : {0, 1, 3, 7, 31}) {
        for (int rep = 0; rep < 3; ++rep) {
            ParallelCopier idle(workers);  // made and destroyed with no copy in between
        }
        ParallelCopier c(workers);
        for (size_t n : lengths) check_copy(c, b, n, 0, workers, "one copy");
        // back to back on one copier: every copy a new generation, lengths on both sides of the 1 MiB threshold
        for (int i = 0; i < 400; ++i) check_copy(c, b, (i % 3 == 2 ? kMiB - 7 : kMiB) + (size_t)i * 37, (size_t)i, workers, "back to back");
        std::printf("%d workers: %zu lengths and 400 back-to-back copies\n", workers, sizeof lengths / sizeof *lengths);
    }
    if (g_failures) {
        std::printf("%d copies FAILED\n", g_failures);
        return 1;
    }
    std::printf("copier ok\n");
    return 0;
}
