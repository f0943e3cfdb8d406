// The launch layout of the two LDS-staged regrid forms (staged.hip, staged2*.hip), stated once: how a target is cut into tiles,
// which XCD runs which tile, which slices a workgroup takes, and how a workgroup finds its tile and z chunk again.  Plain
// arithmetic without a HIP include: the plan builders and launchers call it on the host, the apply kernels call the decoders on
// the device, and tests/test_staged_layout.py (the chunk-per-XCD order: tests/test_staged_layout_chunk_xcd.py) compiles it with g++
// and checks on the CPU what no parity test shows -- that every tile is computed, and computed once.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define FA_LAYOUT_HD __host__ __device__ __forceinline__
#else
#define FA_LAYOUT_HD inline
#endif

namespace fimex_amd {

// A tile of the second staged form (Staged2Plan, plan.hpp): one height per plan, varying width.
struct StagedTile {
    uint32_t x0, y0, w;     // output columns [x0, x0 + w) of rows [y0, y0 + tileH)
    uint32_t nChunks;       // 16-byte chunks streamed per slice
    uint32_t chunkBase;     // first entry in chunkOff
    uint32_t rsv[3];        // rsv[0] = 1: a gather tile (not staged, the kernel reads its stencils from memory)
};

namespace layout {
constexpr uint32_t kXcds = 8;  // workgroup b of a launch runs on XCD b % 8 (plan.hpp holds it to common.hpp's kXcds)
}

constexpr int kMaxZChunks = 31;
constexpr uint32_t kSpareBytes = 1024;  // one wave instruction of LDS-DMA behind the ring (see SliceRing, staged2_ring.hpp)
constexpr uint32_t kTileTooLarge = 0xFFFFFFFFu;  // the tile scan's nChunks of a tile that does not fit a slot

// ---- tile cutting (second form)

// chunks of one slot: the workgroup's LDS less the spare KiB, in `depth` equal slots of whole wave instructions
inline uint32_t slot_chunks(uint32_t ldsBytes, uint32_t depth)
{
    return ((ldsBytes - kSpareBytes) / depth / 16u) & ~63u;
}

// chunks a tile may stage: a slot of the ring, kmax chunks per lane, and 16-bit LDS offsets that count elements (cpc per chunk)
inline uint32_t tile_chunk_cap(uint32_t ldsBytes, uint32_t depth, uint32_t kmax, uint32_t nt, uint32_t cpc)
{
    return std::min(std::min(slot_chunks(ldsBytes, depth), kmax * nt), 65535u / cpc);
}

// tile widths are multiples of this (a wave stores 64 consecutive cells)
inline uint32_t tile_width_step(uint32_t tileW) { return tileW >= 128 ? 64u : 32u; }

// the width every band starts with: the shape's, or the target's rounded up to a step
inline uint32_t widest_tile(uint32_t tileW, uint32_t step, uint32_t outX) { return std::min(tileW, (outX + step - 1) / step * step); }

// tiles of width w (the last one narrower) over [0, outX) of the band that starts at row y0
inline void uniform_row(uint32_t y0, uint32_t w, uint32_t outX, std::vector<StagedTile>& out)
{
    for (uint32_t x0 = 0; x0 < outX; x0 += w) {
        StagedTile t{};
        t.x0 = x0;
        t.y0 = y0;
        t.w = std::min(w, outX - x0);
        out.push_back(t);
    }
}

// the bands' tiles as one list, band after band, and the band of every tile
inline void flatten_bands(const std::vector<std::vector<StagedTile>>& rows, std::vector<StagedTile>& tiles, std::vector<uint32_t>& bandOf)
{
    tiles.clear();
    bandOf.clear();
    for (size_t b = 0; b < rows.size(); ++b)
        for (const StagedTile& t : rows[b]) { tiles.push_back(t); bandOf.push_back((uint32_t)b); }
}

// One refinement pass.  `scanned`: the tiles of flatten_bands as the tile scan left them (nChunks counted, kTileTooLarge for a
// tile that does not fit: too many chunks for a slot, too many source rows).  Such a tile makes its band narrower by one step
// when most tiles of the band fail (the band's cells cover more source: rows near the pole of the benchmark plan), otherwise it
// is split in two; at the narrowest width it becomes a gather tile.  Returns whether the new tiles need another scan.
inline bool refine_bands(std::vector<std::vector<StagedTile>>& rows, std::vector<uint32_t>& rowW, uint32_t step, uint32_t outX,
                         const StagedTile* scanned)
{
    auto failed_tile = [](const StagedTile& t) { return t.rsv[0] == 0 && t.nChunks == kTileTooLarge; };
    bool again = false;
    size_t i = 0;
    for (size_t b = 0; b < rows.size(); ++b) {
        const size_t n = rows[b].size();
        size_t failed = 0;
        for (size_t k = 0; k < n; ++k) {
            rows[b][k] = scanned[i + k];
            if (failed_tile(scanned[i + k])) ++failed;
        }
        i += n;
        if (failed == 0) continue;
        again = true;
        if (2 * failed > n && rowW[b] > step) {  // the whole band is too heavy: narrower tiles throughout
            const uint32_t y0 = rows[b][0].y0;
            rowW[b] -= step;
            rows[b].clear();
            uniform_row(y0, rowW[b], outX, rows[b]);
            continue;
        }
        std::vector<StagedTile> next;
        for (const StagedTile& t : rows[b]) {
            if (!failed_tile(t)) { next.push_back(t); continue; }
            if (t.w <= step) {  // cannot be split any further
                StagedTile g = t;
                g.nChunks = 0;
                g.rsv[0] = 1;
                next.push_back(g);
                continue;
            }
            StagedTile l = t, r = t;
            l.w = (t.w / 2 + step - 1) / step * step;
            r.x0 = t.x0 + l.w;
            r.w = t.w - l.w;
            l.nChunks = r.nChunks = 0;
            next.push_back(l);
            next.push_back(r);
        }
        rows[b].swap(next);
    }
    return again;
}

// More than 1/8 of the live cells (columns of tiles that read anything) in gather tiles: positions without spatial coherence,
// the gather kernels serve them better and the form is given up.
inline bool gather_share_too_large(const std::vector<StagedTile>& tiles)
{
    size_t gatherCells = 0, liveCells = 0;
    for (const StagedTile& t : tiles) {
        if (t.rsv[0] != 0) gatherCells += t.w;
        if (t.rsv[0] != 0 || t.nChunks != 0) liveCells += t.w;
    }
    return gatherCells * 8 > liveCells;
}

// chunkBase of every tile: the prefix sum of nChunks, returned in full.  false: a tile's base does not fit 32 bits.
inline bool assign_chunk_bases(std::vector<StagedTile>& tiles, size_t& total)
{
    total = 0;
    for (StagedTile& t : tiles) {
        if (total > 0xFFFFFFFFu) return false;
        t.chunkBase = (uint32_t)total;
        total += t.nChunks;
    }
    return true;
}

// ---- workgroup -> tile table (second form)

// Workgroups are dealt round-robin over the XCDs (b % 8 shares an L2); bands go to the XCDs in stripes of `stripe` bands, so that
// neighbours in x (and, inside a stripe, in y) run on the same XCD and meet in its L2: stripes of about `stripe` bands, their
// number a multiple of the XCD count so that every XCD gets equally many.  Fewer bands than XCDs (wide, short targets such as
// cross-sections): the tiles themselves are dealt round-robin.  order[k * 8 + x] is the k-th tile of XCD x, ~0u behind its last.
inline std::vector<uint32_t> xcd_order(const std::vector<uint32_t>& bandOf, uint32_t nBands, uint32_t stripe)
{
    using layout::kXcds;
    std::vector<std::vector<uint32_t>> perXcd(kXcds);
    uint32_t nStripes = (uint32_t)((nBands + stripe * kXcds / 2) / (stripe * kXcds)) * kXcds;
    if (nStripes < kXcds) nStripes = kXcds;
    if (nStripes > nBands) nStripes = std::max<uint32_t>(nBands / kXcds * kXcds, 1);
    for (size_t i = 0; i < bandOf.size(); ++i)
        perXcd[nBands < kXcds ? i % kXcds : ((uint64_t)bandOf[i] * nStripes / nBands) % kXcds].push_back((uint32_t)i);
    size_t longest = 0;
    for (auto& l : perXcd) longest = std::max(longest, l.size());
    std::vector<uint32_t> order(longest * kXcds, 0xFFFFFFFFu);
    for (uint32_t x = 0; x < kXcds; ++x)
        for (size_t k = 0; k < perXcd[x].size(); ++k) order[k * kXcds + x] = perXcd[x][k];
    return order;
}

// The table of the chunk-per-XCD order (chunk_xcd_workgroup below): XCD x runs z chunk x of EVERY tile, so all eight XCDs walk this
// one sequence of tiles and nothing is padded.  The sequence is cut into cohorts of `by` bands x `bx` tiles, as many workgroups as
// an XCD starts together, y fastest inside a cohort: vertical neighbours, which share most source lines (the target rows are
// tilted against the source rows), are adjacent entries and meet in the XCD's L2.  The rule, for bands of unequal tile counts:
//   band group   by consecutive bands;
//   column       of a tile: where its middle lies in units of the widest tile, (x0 + w / 2) / tileW;
//   cohort       the tiles of a band group in bx consecutive columns, in the order (column, band, x0); narrower tiles put more
//                than by * bx tiles there: the cohort is then cut after by * bx of them and the rest is a cohort of its own, so
//                that two tiles of one cohort are never more than by * bx - 1 entries apart.
// Cohorts follow each other column group by column group, band group after band group.  cohortOf (optional): the cohort of
// every entry of the result.
inline std::vector<uint32_t> chunk_xcd_order(const std::vector<StagedTile>& tiles, const std::vector<uint32_t>& bandOf, uint32_t tileW,
                                             uint32_t by, uint32_t bx, std::vector<uint32_t>* cohortOf = nullptr)
{
    by = std::max(by, 1u);
    bx = std::max(bx, 1u);
    tileW = std::max(tileW, 1u);
    struct Key {
        uint32_t group, columns, column, band, x0, tile;
    };
    std::vector<Key> keys(tiles.size());
    for (size_t i = 0; i < tiles.size(); ++i) {
        const uint32_t column = (tiles[i].x0 + tiles[i].w / 2) / tileW;
        keys[i] = Key{bandOf[i] / by, column / bx, column, bandOf[i], tiles[i].x0, (uint32_t)i};
    }
    std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
        if (a.group != b.group) return a.group < b.group;
        if (a.columns != b.columns) return a.columns < b.columns;
        if (a.column != b.column) return a.column < b.column;
        if (a.band != b.band) return a.band < b.band;
        return a.x0 < b.x0;
    });
    std::vector<uint32_t> order(keys.size());
    if (cohortOf) cohortOf->assign(keys.size(), 0);
    uint32_t cohort = 0, held = 0;
    for (size_t k = 0; k < keys.size(); ++k) {
        if (k > 0 && (keys[k].group != keys[k - 1].group || keys[k].columns != keys[k - 1].columns || held == by * bx)) {
            ++cohort;
            held = 0;
        }
        ++held;
        order[k] = keys[k].tile;
        if (cohortOf) (*cohortOf)[k] = cohort;
    }
    return order;
}

// ---- z chunks

// The order of a float launch of the second form (STAGE2_ORDER in the tuning build): which workgroup runs which tile and z chunk.
enum LaunchOrder : int {
    kChunkMajor = 0,   // two-dimensional grid: blockIdx.x -> xcd_order's table, blockIdx.y = z chunk
    kTileMajor = 1,    // flat_workgroup: an XCD owns whole tiles, the z chunks of a tile are consecutive workgroups of it
    kChunkPerXcd = 2,  // chunk_xcd_workgroup: an XCD owns z chunks, every XCD walks the same sequence of tiles
};

// slices [zStart[c], zStart[c + 1]) belong to z chunk c of n
struct ZChunks {
    uint32_t zStart[kMaxZChunks + 1];
    uint32_t n;
};

// n z chunks of one size (the first nz % n of them one slice longer)
inline ZChunks even_z_split(size_t nz, uint32_t n)
{
    ZChunks zc{};
    for (uint32_t c = 0, z = 0; c < n; ++c) {
        zc.zStart[c] = z;
        z += (uint32_t)nz / n + (c < (uint32_t)nz % n ? 1u : 0u);
    }
    zc.zStart[n] = (uint32_t)nz;
    zc.n = n;
    return zc;
}

// The chunk-per-XCD order needs a chunk count that is a multiple of the XCD count: 8 chunks, or 16 where the tile-major split of
// the same batch makes more than 8, provided that no chunk gets shorter than (zpb + 1) / 2 slices -- the shortest chunk the
// tile-major split makes of a batch longer than one chunk (zpb + 1 slices go in two).  0: the batch is too short, the launch
// keeps the tile-major order and its chunks.
inline uint32_t chunk_xcd_chunk_count(size_t nz, uint32_t zpb)
{
    if (zpb < 1) zpb = 1;
    if ((nz + zpb - 1) / zpb > 16) zpb = (uint32_t)((nz + 15) / 16);
    const size_t shortest = (zpb + 1) / 2;
    if ((nz + zpb - 1) / zpb > layout::kXcds && nz / (2 * layout::kXcds) >= shortest) return 2 * layout::kXcds;
    return nz / layout::kXcds >= shortest ? layout::kXcds : 0u;
}

// The order a launch runs when `wanted` is asked for: the chunk-per-XCD order only where the launch allows it (the pair kernels do
// not) and the batch is long enough, the tile-major order otherwise.
inline int launch_order_of(int wanted, bool allowChunkPerXcd, size_t nz, uint32_t zpb)
{
    return wanted == kChunkPerXcd && !(allowChunkPerXcd && chunk_xcd_chunk_count(nz, zpb) != 0) ? (int)kTileMajor : wanted;
}

// The z chunks of a float launch of the second form, nz slices in chunks of about zpb, by launch order (LaunchOrder).
// Tile-major order: at most 16 chunks of one size.  Chunk-per-XCD order: chunk_xcd_chunk_count chunks of one size, or the
// tile-major split where that is 0.  Chunk-major order (all tiles of chunk 0, then chunk 1, ...): at most
// kMaxZChunks - 6 before the tail; with ztail > 0 the chunks shrink towards the end of the launch so that the last workgroups are
// short ones (the last 2 * zpb slices go in halves of at least ztail).  false: more than kMaxZChunks chunks.
inline bool float_z_chunks(size_t nz, int order, uint32_t zpb, uint32_t ztail, ZChunks& zc)
{
    const bool tileMajor = order != kChunkMajor;
    if (zpb < 1) zpb = 1;
    if (order == kChunkPerXcd && chunk_xcd_chunk_count(nz, zpb) != 0) {
        zc = even_z_split(nz, chunk_xcd_chunk_count(nz, zpb));
        return true;
    }
    const size_t mostChunks = tileMajor ? 16 : (size_t)kMaxZChunks - 6;
    if ((nz + zpb - 1) / zpb > mostChunks) zpb = (uint32_t)((nz + mostChunks - 1) / mostChunks);
    if (tileMajor) {
        zc = even_z_split(nz, (uint32_t)((nz + zpb - 1) / zpb));
        return true;
    }
    zc = ZChunks{};
    for (uint32_t z = 0; z < nz;) {
        const uint32_t rem = (uint32_t)nz - z;
        uint32_t size = zpb;
        if (ztail > 0 && rem <= 2 * zpb) size = std::max(ztail, (rem + 1) / 2);
        if (size > rem || rem - size < (ztail + 1) / 2) size = rem;
        if (zc.n >= (uint32_t)kMaxZChunks) return false;
        zc.zStart[zc.n++] = z;
        z += size;
    }
    zc.zStart[zc.n] = (uint32_t)nz;
    return true;
}

// Stored types through the second form: even chunks of about zpb slices, at most 16, and at least four where the batch allows
// (nz / 6), so that short batches still fill the chip.
inline uint32_t typed_z_chunk_count(size_t nz, uint32_t zpb)
{
    if (zpb < 1) zpb = 1;
    if ((nz + zpb - 1) / zpb > 16) zpb = (uint32_t)((nz + 15) / 16);
    uint32_t n = (uint32_t)((nz + zpb - 1) / zpb);
    n = std::max<uint32_t>(n, (uint32_t)std::min<size_t>(4, nz / 6));
    return n < 1 ? 1 : n;
}

// First form: chunks of zPerBlock slices each (the last one shorter), zPerBlock between 1 and nz.
struct FirstFormZ {
    uint32_t zPerBlock;
    size_t chunks;
};
inline FirstFormZ first_form_z(size_t nz, uint32_t zpb)
{
    if (zpb < 1) zpb = 1;
    if (zpb > nz) zpb = (uint32_t)nz;
    return FirstFormZ{zpb, (nz + zpb - 1) / zpb};
}

// ---- workgroup -> tile (first form) and the flat grid of both forms

inline uint32_t first_form_tiles_per_xcd(uint32_t nTiles) { return (nTiles + layout::kXcds - 1) / layout::kXcds; }

// Workgroups of one z chunk.  xcdRemap 0: tiles in dispatch order (neighbours on different XCDs); 1: each XCD owns one contiguous
// run of tiles; >= 2: tile rows dealt to the XCDs in stripes of (xcdRemap - 1) rows, whole stripes per XCD.
inline uint32_t first_form_grid(uint32_t nTiles, uint32_t tilesX, uint32_t xcdRemap)
{
    using layout::kXcds;
    if (xcdRemap < 2) return first_form_tiles_per_xcd(nTiles) * kXcds;
    const uint32_t stripe = (xcdRemap - 1) * tilesX;
    return (uint32_t)((nTiles + (size_t)stripe * kXcds - 1) / ((size_t)stripe * kXcds)) * stripe * kXcds;
}

// the tile of workgroup b of first_form_grid; a result >= nTiles: none
FA_LAYOUT_HD uint32_t first_form_tile(uint32_t b, uint32_t xcdRemap, uint32_t tilesPerXcd, uint32_t tilesX)
{
    using layout::kXcds;
    if (xcdRemap == 1) return (b % kXcds) * tilesPerXcd + b / kXcds;
    if (xcdRemap >= 2) {
        const uint32_t stripe = (xcdRemap - 1) * tilesX;
        const uint32_t idx = b / kXcds;
        return ((idx / stripe) * kXcds + b % kXcds) * stripe + idx % stripe;
    }
    return b;
}

// Flat grid of gridX * n workgroups in tile-major order: workgroup s runs on XCD s % 8, and the k-th workgroup of an XCD is z
// chunk k % n of the XCD's tile k / n -- the z chunks of a tile are consecutive workgroups of one XCD.
FA_LAYOUT_HD void flat_workgroup(uint32_t blockX, uint32_t nZChunks, uint32_t& slot, uint32_t& zc)
{
    const uint32_t k = blockX / layout::kXcds;
    zc = k % nZChunks;
    slot = (k / nZChunks) * layout::kXcds + blockX % layout::kXcds;
}

// Flat grid of nTiles * n workgroups in chunk-per-XCD order, n a multiple of 8: workgroup s runs on XCD s % 8, and the k-th
// workgroup of XCD x is z chunk x + 8 * (k % (n / 8)) of entry k / (n / 8) of chunk_xcd_order's table -- with 8 chunks workgroup s
// is (entry s / 8, chunk s % 8); with 16 an XCD takes chunks x and x + 8 of an entry in turn.  The roles of the launch's three
// carriers: blockIdx.x alone says XCD, entry and chunk; order[] (the same for every XCD) turns the entry into a tile, ~0u = none;
// zStart[] turns the chunk into slices.
FA_LAYOUT_HD void chunk_xcd_workgroup(uint32_t blockX, uint32_t nZChunks, uint32_t& slot, uint32_t& zc)
{
    const uint32_t k = blockX / layout::kXcds, perXcd = nZChunks / layout::kXcds;
    slot = k / perXcd;
    zc = blockX % layout::kXcds + (k % perXcd) * layout::kXcds;
}

// the decoder of a flat grid by the launch's mode (Staged2Args::chunkPerXcd)
FA_LAYOUT_HD void flat_grid_workgroup(uint32_t blockX, uint32_t nZChunks, uint32_t chunkPerXcd, uint32_t& slot, uint32_t& zc)
{
    if (chunkPerXcd) chunk_xcd_workgroup(blockX, nZChunks, slot, zc);
    else flat_workgroup(blockX, nZChunks, slot, zc);
}

}  // namespace fimex_amd
