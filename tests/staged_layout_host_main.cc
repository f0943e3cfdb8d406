// Stand-alone run of the staged forms' launch layout on the CPU, for a sanitizer build:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ifimex_amd/csrc
//       tests/staged_layout_host_main.cc tests/staged_layout_host.cc -o staged_layout_host_main
//   ./staged_layout_host_main
//
// Sends the sweeps of tests/test_staged_layout.py through every entry point of staged_layout_host.cc once -- the same ranges, output
// arrays of exactly the size asked for -- and prints what it counted.  Not run by pytest and not loaded into Python.
#include <cstdint>
#include <cstdio>
#include <vector>

struct Cut;
extern "C" {
void sl_flat_workgroup(uint32_t blockX, uint32_t nZChunks, uint32_t* slot, uint32_t* zc);
uint32_t sl_first_form_grid(uint32_t nTiles, uint32_t tilesX, uint32_t xcdRemap);
void sl_first_form_tiles(uint32_t gridX, uint32_t nTiles, uint32_t tilesX, uint32_t xcdRemap, uint32_t* tiles);
uint64_t sl_xcd_order(const uint32_t* bandOf, uint64_t nTiles, uint32_t nBands, uint32_t stripe, uint32_t* out, uint64_t cap);
Cut* sl_cut_new(uint32_t outX, uint32_t outY, uint32_t tileW, uint32_t tileH);
void sl_cut_free(Cut* c);
uint64_t sl_cut_count(const Cut* c);
void sl_cut_tiles(const Cut* c, uint32_t* out);
int sl_cut_refine(Cut* c, const uint32_t* nChunks);
int sl_cut_finish(Cut* c, uint64_t* total);
void sl_float_z_chunks(uint32_t nz0, uint32_t count, int tileMajor, uint32_t zpb, uint32_t ztail, uint32_t* zStart, uint32_t* n, uint8_t* ok);
void sl_typed_z_chunks(uint32_t nz0, uint32_t count, uint32_t zpb, uint32_t* zStart, uint32_t* n);
void sl_first_form_z(uint32_t nz0, uint32_t count, uint32_t zpb, uint32_t* zPerBlock, uint64_t* chunks);
int sl_max_z_chunks();
}

int main()
{
    unsigned long long sum = 0;
    for (uint32_t gridX = 8; gridX <= 64; gridX += 8)
        for (uint32_t n = 1; n <= 16; ++n)
            for (uint32_t b = 0; b < gridX * n; ++b) {
                uint32_t slot, zc;
                sl_flat_workgroup(b, n, &slot, &zc);
                sum += slot + zc;
            }
    for (uint32_t remap = 0; remap < 4; ++remap)
        for (uint32_t tilesX = 1; tilesX <= 5; ++tilesX)
            for (uint32_t nTiles = 1; nTiles <= 60; ++nTiles) {
                std::vector<uint32_t> tiles(sl_first_form_grid(nTiles, tilesX, remap));
                sl_first_form_tiles((uint32_t)tiles.size(), nTiles, tilesX, remap, tiles.data());
                for (uint32_t t : tiles) sum += t < nTiles;
            }
    uint32_t seed = 12345;
    auto rnd = [&](uint32_t n) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % n; };
    for (uint32_t nBands = 1; nBands <= 40; ++nBands)
        for (uint32_t stripe : {1u, 2u, 4u, 8u}) {
            std::vector<uint32_t> bandOf;
            for (uint32_t b = 0; b < nBands; ++b) bandOf.insert(bandOf.end(), 1 + rnd(5), b);
            const uint64_t n = sl_xcd_order(bandOf.data(), bandOf.size(), nBands, stripe, nullptr, 0);
            std::vector<uint32_t> order(n);
            sl_xcd_order(bandOf.data(), bandOf.size(), nBands, stripe, order.data(), n);
            for (uint32_t t : order) sum += t != 0xFFFFFFFFu;
        }
    // tile cutting with chunks = the weights of a tile's columns, summed; a slot holds 2000
    long passes = 0, kept = 0;
    for (uint32_t tileW : {64u, 128u, 256u, 512u})
        for (int trial = 0; trial < 60; ++trial) {
            const uint32_t widths[] = {64, 100, 512, 1000, 1024, 1500};
            const uint32_t outX = widths[rnd(6)], nBands = 1 + rnd(6), outY = nBands * 8 - rnd(8);
            const double levels[] = {0.0, 0.3, 0.8, 1.5, 3.0};
            std::vector<std::vector<uint32_t>> weight(nBands, std::vector<uint32_t>(outX));
            for (auto& row : weight) {
                const double level = levels[rnd(5)] * 2000 / tileW;
                for (uint32_t& w : row) w = (uint32_t)(level * (0.5 + rnd(1000) / 1000.0));
            }
            for (uint32_t s = rnd(5) == 4 ? 40 : rnd(3); s > 0; --s) weight[rnd(nBands)][rnd(outX)] = 2001;
            Cut* c = sl_cut_new(outX, outY, tileW, 8);
            for (int pass = 0; pass < 66; ++pass, ++passes) {
                std::vector<uint32_t> t(8 * sl_cut_count(c)), counts(sl_cut_count(c));
                sl_cut_tiles(c, t.data());
                for (size_t i = 0; i < counts.size(); ++i) {
                    uint64_t n = 0;
                    for (uint32_t x = t[8 * i]; x < t[8 * i] + t[8 * i + 2]; ++x) n += weight[t[8 * i + 6]][x];
                    counts[i] = n > 2000 ? 0xFFFFFFFFu : (uint32_t)n;
                }
                if (!sl_cut_refine(c, counts.data())) break;
            }
            uint64_t total = 0;
            kept += sl_cut_finish(c, &total) == 0;
            sum += total;
            sl_cut_free(c);
        }
    const uint32_t N = 4096, K = (uint32_t)sl_max_z_chunks() + 1;
    std::vector<uint32_t> zStart((size_t)N * K), n(N), per(N);
    std::vector<uint8_t> ok(N);
    std::vector<uint64_t> chunks(N);
    long refused = 0;
    for (uint32_t zpb = 1; zpb <= 64; ++zpb) {
        sl_float_z_chunks(1, N, 1, zpb, 0, zStart.data(), n.data(), ok.data());
        for (uint32_t ztail = 0; ztail <= 16; ++ztail) {
            sl_float_z_chunks(1, N, 0, zpb, ztail, zStart.data(), n.data(), ok.data());
            for (uint8_t o : ok) refused += o == 0;
        }
        sl_typed_z_chunks(1, N, zpb, zStart.data(), n.data());
        sl_first_form_z(1, N, zpb, per.data(), chunks.data());
        sum += n[N - 1] + chunks[N - 1];
    }
    std::printf("checksum %llu, %ld cutting passes, %ld of 240 forms kept, %ld chunk-major launches refused\n", sum, passes, kept, refused);
    return 0;
}
