// Stand-alone run of the projection string parser and point math on the CPU, for a sanitizer build:
//
//   hipcc --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Ifimex_amd/csrc tests/projection_host_main.hip tests/projection_host.hip fimex_amd/csrc/projection_parse.hip -o projection_host_main
//   python scripts/dump_projection_strings.py | ./projection_host_main
//
// Reads one pair per line, "source<TAB>target", sends a small mesh of points through projection_host_transform both ways and prints how
// many pairs were transformed and how many refused.  Not run by pytest and not loaded into Python.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

extern "C" int projection_host_transform(const char* src, const char* dst, double* x, double* y, int64_t n, char* err, size_t errLen);

int main()
{
    int done = 0, refused = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        const size_t tab = line.find('\t');
        if (tab == std::string::npos) continue;
        const std::string src = line.substr(0, tab), dst = line.substr(tab + 1);
        std::vector<double> x, y;
        for (int i = -4; i <= 4; ++i)
            for (int j = -3; j <= 3; ++j) { x.push_back(.35 * i); y.push_back(.5 * j); }  // radians: most of the globe, the poles included
        char err[16];  // shorter than every message: the shim must cut it
        if (projection_host_transform(src.c_str(), dst.c_str(), x.data(), y.data(), (int64_t)x.size(), err, sizeof err) != 0) { ++refused; continue; }
        if (projection_host_transform(dst.c_str(), src.c_str(), x.data(), y.data(), (int64_t)x.size(), err, sizeof err) != 0) { ++refused; continue; }
        ++done;
    }
    std::printf("%d pairs transformed there and back, %d refused\n", done, refused);
    return 0;
}
