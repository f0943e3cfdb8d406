// C entry points over the chunk-per-XCD launch order of fimex_amd/csrc/staged_layout.hpp for the CPU:
// tests/test_staged_layout_chunk_xcd.py compiles this file with g++ into a temporary directory and calls it through ctypes.
#include "staged_layout.hpp"

using namespace fimex_amd;

extern "C" {

// the table of n tiles (x0, w, band each) and the cohort of every entry
void scx_order(uint64_t n, const uint32_t* x0, const uint32_t* w, const uint32_t* band, uint32_t tileW, uint32_t by, uint32_t bx, uint32_t* order,
               uint32_t* cohort)
{
    std::vector<StagedTile> tiles(n);
    std::vector<uint32_t> bandOf(band, band + n);
    for (uint64_t i = 0; i < n; ++i) {
        tiles[i] = StagedTile{};
        tiles[i].x0 = x0[i];
        tiles[i].w = w[i];
    }
    std::vector<uint32_t> cohortOf;
    const std::vector<uint32_t> o = chunk_xcd_order(tiles, bandOf, tileW, by, bx, &cohortOf);
    std::copy(o.begin(), o.end(), order);
    std::copy(cohortOf.begin(), cohortOf.end(), cohort);
}

// slot[b], zc[b] of every workgroup b of a flat grid, by the launch's mode (what decode_workgroup calls on the device)
void scx_decode(uint32_t grid, uint32_t nZChunks, uint32_t chunkPerXcd, uint32_t* slot, uint32_t* zc)
{
    for (uint32_t b = 0; b < grid; ++b) flat_grid_workgroup(b, nZChunks, chunkPerXcd, slot[b], zc[b]);
}

uint32_t scx_chunk_count(uint64_t nz, uint32_t zpb) { return chunk_xcd_chunk_count(nz, zpb); }

int scx_launch_order(int wanted, int allow, uint64_t nz, uint32_t zpb) { return launch_order_of(wanted, allow != 0, nz, zpb); }

// zStart[kMaxZChunks + 1] and n of one batch; returns the rule's own answer
int scx_z_chunks(uint64_t nz, int order, uint32_t zpb, uint32_t* zStart, uint32_t* n)
{
    ZChunks zc{};
    const bool ok = float_z_chunks(nz, order, zpb, 0, zc);
    std::copy(zc.zStart, zc.zStart + kMaxZChunks + 1, zStart);
    *n = zc.n;
    return ok ? 1 : 0;
}

}  // extern "C"
