// Host shim of fimex_amd/csrc/vertical_search.hpp for tests/test_vertical_search_host.py: the search for the pair of input levels
// around a target, run for one column after another on the CPU through the functions the vertical kernels call -- Column::level,
// monotonic_pair, and walk_pairs where it cannot be sure -- inside the kernels' loop: the monotonicity scan, groups of kGroup targets.  Built for the host only by
// fimex_amd/build.py (hipcc --cuda-host-only -ffp-contract=off); needs no GPU.
#include "vertical_search.hpp"

using namespace fimex_amd;

namespace {

template <int kGroup>
void search(const Levels& L, size_t ncol, const double* x, size_t nx, int bisect, unsigned* first, unsigned* second, unsigned char* walked,
            float* levels)
{
    for (size_t col = 0; col < ncol; ++col) {
        const Column in(L, 0, col, ncol);
        for (unsigned k = 0; k < L.nz; ++k) levels[col * L.nz + k] = in.level(k);
        int mono = 0;  // as in vertical_kernel
        if (bisect && L.nz >= 2) {
            bool inc = true, dec = true;
            float prev = in.level(0);
            for (unsigned k = 1; k < L.nz; ++k) {
                const float cur = in.level(k);
                inc &= prev < cur;
                dec &= prev > cur;
                prev = cur;
            }
            mono = inc ? 1 : dec ? -1 : 0;
        }
        for (size_t k0 = 0; k0 < nx; k0 += kGroup) {
            double xg[kGroup];
            unsigned f[kGroup], s[kGroup];
            bool walk[kGroup], anyWalk = false;
            for (int g = 0; g < kGroup; ++g) {
                xg[g] = x[col * nx + (k0 + g < nx ? k0 + g : nx - 1)];  // a short last group repeats its last target
                const int pair = monotonic_pair(in, (int)L.nz, mono, xg[g]);
                walk[g] = pair < 0;
                f[g] = (unsigned)pair & 0xffffu;
                s[g] = (unsigned)pair >> 16;
                anyWalk |= walk[g];
            }
            if (anyWalk) {
                unsigned wf[kGroup], ws[kGroup];
                walk_pairs<kGroup>(in, L.nz, xg, wf, ws);
                for (int g = 0; g < kGroup; ++g)
                    if (walk[g]) { f[g] = wf[g]; s[g] = ws[g]; }
            }
            for (int g = 0; g < kGroup && k0 + g < nx; ++g) {
                first[col * nx + k0 + g] = f[g];
                second[col * nx + k0 + g] = s[g];
                walked[col * nx + k0 + g] = walk[g];
            }
        }
    }
}

}  // namespace

extern "C" {

// The levels of ncol columns (t = 0, plane = ncol: ps [ncol], field [nz][ncol], c0 / c1 [nz] on the host) and nx targets per
// column, x [ncol][nx] -> first, second, walked [ncol][nx] and the float levels [ncol][nz].  bisect 0: every column is walked.
int vertical_search_host(int group, int kind, unsigned nz, const double* c0, const double* c1, double p0, double ptop, const float* ps,
                         const float* field, size_t ncol, const double* x, size_t nx, int bisect, unsigned* first, unsigned* second,
                         unsigned char* walked, float* levels)
{
    if (nz == 0 || nx == 0 || (group != 4 && group != 8)) return -1;
    Levels L{};
    L.kind = kind;
    L.nz = nz;
    L.c0 = c0;
    L.c1 = c1;
    L.p0 = p0;
    L.ptop = ptop;
    L.ps = ps;
    L.field = field;
    if (group == 8) search<8>(L, ncol, x, nx, bisect, first, second, walked, levels);
    else search<4>(L, ncol, x, nx, bisect, first, second, walked, levels);
    return 0;
}

}  // extern "C"
