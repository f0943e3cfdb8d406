// C entry points over fimex_amd/csrc/staged_layout.hpp for the CPU: tests/staged_layout_host.py compiles this file with g++ into a
// temporary directory and calls it through ctypes; tests/staged_layout_host_main.cc calls it from a sanitizer build.
#include "staged_layout.hpp"

using namespace fimex_amd;

extern "C" {

void sl_flat_workgroup(uint32_t blockX, uint32_t nZChunks, uint32_t* slot, uint32_t* zc) { flat_workgroup(blockX, nZChunks, *slot, *zc); }

uint32_t sl_first_form_grid(uint32_t nTiles, uint32_t tilesX, uint32_t xcdRemap) { return first_form_grid(nTiles, tilesX, xcdRemap); }

// tiles[b] for every workgroup b of a grid of gridX
void sl_first_form_tiles(uint32_t gridX, uint32_t nTiles, uint32_t tilesX, uint32_t xcdRemap, uint32_t* tiles)
{
    for (uint32_t b = 0; b < gridX; ++b) tiles[b] = first_form_tile(b, xcdRemap, first_form_tiles_per_xcd(nTiles), tilesX);
}

// returns the table's length; writes at most cap entries
uint64_t sl_xcd_order(const uint32_t* bandOf, uint64_t nTiles, uint32_t nBands, uint32_t stripe, uint32_t* out, uint64_t cap)
{
    const std::vector<uint32_t> order = xcd_order(std::vector<uint32_t>(bandOf, bandOf + nTiles), nBands, stripe);
    for (size_t i = 0; i < order.size() && i < cap; ++i) out[i] = order[i];
    return order.size();
}

// ---- tile cutting: the state build_shape keeps between scans
struct Cut {
    uint32_t outX, step;
    std::vector<std::vector<StagedTile>> rows;
    std::vector<uint32_t> rowW;
    std::vector<StagedTile> tiles;
    std::vector<uint32_t> bandOf;
};

Cut* sl_cut_new(uint32_t outX, uint32_t outY, uint32_t tileW, uint32_t tileH)
{
    Cut* c = new Cut;
    c->outX = outX;
    c->step = tile_width_step(tileW);
    const uint32_t nBands = (outY + tileH - 1) / tileH;
    c->rows.resize(nBands);
    c->rowW.assign(nBands, widest_tile(tileW, c->step, outX));
    for (uint32_t b = 0; b < nBands; ++b) uniform_row(b * tileH, c->rowW[b], outX, c->rows[b]);
    flatten_bands(c->rows, c->tiles, c->bandOf);
    return c;
}
void sl_cut_free(Cut* c) { delete c; }
uint32_t sl_cut_step(const Cut* c) { return c->step; }
uint64_t sl_cut_count(const Cut* c) { return c->tiles.size(); }

// per tile: x0, y0, w, nChunks, chunkBase, gather (rsv[0]), band, width of its band
void sl_cut_tiles(const Cut* c, uint32_t* out)
{
    for (size_t i = 0; i < c->tiles.size(); ++i) {
        const StagedTile& t = c->tiles[i];
        const uint32_t v[8] = {t.x0, t.y0, t.w, t.nChunks, t.chunkBase, t.rsv[0], c->bandOf[i], c->rowW[c->bandOf[i]]};
        std::copy(v, v + 8, out + 8 * i);
    }
}

// one pass: nChunks[i] is what the scan counted for tile i (kTileTooLarge: does not fit; ignored for gather tiles, as tile_scan
// leaves them alone).  Returns whether the new tiles need another scan.
int sl_cut_refine(Cut* c, const uint32_t* nChunks)
{
    for (size_t i = 0; i < c->tiles.size(); ++i)
        if (c->tiles[i].rsv[0] == 0) c->tiles[i].nChunks = nChunks[i];
    const bool again = refine_bands(c->rows, c->rowW, c->step, c->outX, c->tiles.data());
    if (again) flatten_bands(c->rows, c->tiles, c->bandOf);
    return again ? 1 : 0;
}

// after the last pass: the 1/8 rule (returns 1 when the form is given up) and the chunkBase prefix
int sl_cut_finish(Cut* c, uint64_t* total)
{
    if (gather_share_too_large(c->tiles)) return 1;
    size_t t = 0;
    const bool fits = assign_chunk_bases(c->tiles, t);
    *total = t;
    return fits ? 0 : 2;
}

// ---- z chunks, for nz = nz0 .. nz0 + count - 1: zStart[i][kMaxZChunks + 1], n[i]; float rule: ok[i] too
void sl_float_z_chunks(uint32_t nz0, uint32_t count, int tileMajor, uint32_t zpb, uint32_t ztail, uint32_t* zStart, uint32_t* n, uint8_t* ok)
{
    for (uint32_t i = 0; i < count; ++i) {
        ZChunks zc{};
        ok[i] = float_z_chunks(nz0 + i, tileMajor != 0, zpb, ztail, zc) ? 1 : 0;
        std::copy(zc.zStart, zc.zStart + kMaxZChunks + 1, zStart + (size_t)i * (kMaxZChunks + 1));
        n[i] = zc.n;
    }
}
void sl_typed_z_chunks(uint32_t nz0, uint32_t count, uint32_t zpb, uint32_t* zStart, uint32_t* n)
{
    for (uint32_t i = 0; i < count; ++i) {
        const ZChunks zc = even_z_split(nz0 + i, typed_z_chunk_count(nz0 + i, zpb));
        std::copy(zc.zStart, zc.zStart + kMaxZChunks + 1, zStart + (size_t)i * (kMaxZChunks + 1));
        n[i] = zc.n;
    }
}
void sl_first_form_z(uint32_t nz0, uint32_t count, uint32_t zpb, uint32_t* zPerBlock, uint64_t* chunks)
{
    for (uint32_t i = 0; i < count; ++i) {
        const FirstFormZ z = first_form_z(nz0 + i, zpb);
        zPerBlock[i] = z.zPerBlock;
        chunks[i] = z.chunks;
    }
}
int sl_max_z_chunks() { return kMaxZChunks; }
uint32_t sl_tile_chunk_cap(uint32_t ldsBytes, uint32_t depth, uint32_t kmax, uint32_t nt, uint32_t cpc) { return tile_chunk_cap(ldsBytes, depth, kmax, nt, cpc); }

}  // extern "C"
