// LDS-staged backward regrid, second form: the bandwidth path of the headline metric from round 2 on.
//
// Same arithmetic as staged.hip / gather.hip (src/interpolation.c:862-1028) and the same idea -- a workgroup owns a tile of
// OUTPUT cells, streams the source row segments that tile needs HBM -> LDS by LDS-DMA for slice z + d while slice z is
// interpolated out of LDS -- with the structure that the access calibration of round 2 asks for
// (scripts/calib/stream_pattern.hip, profiles/calib/r02_stream_pattern_*.jsonl):
//   * workgroups of 256, 512 or 1024 threads on tiles 2-4 times as large: the lines at the ends of a row segment and the
//     halo rows are shared with the neighbouring tile, and only tiles that run in lockstep share them for certain;
//   * tiles of one height and VARYING width: an output cell of the benchmark plan covers 1.6 .. 3.3 source columns, so a
//     uniform tile grid sizes every LDS slot for the worst tile and leaves 40 % of it unused.  Here the plan narrows the
//     tiles of a tile row until every tile fits the same budget;
//   * one copy of the slice loop per number of DMA instructions a lane issues per slice (dispatch_un, staged2_ring.hpp);
//   * the plan stores the source offset of every 16-byte chunk of a tile, so the workgroup prologue is a coalesced load
//     instead of a binary search per chunk, and row segments start on 16-byte boundaries of the slice for any row length
//     (inX % 4 != 0 included: a reduced domain, src/CachedInterpolation.cc:159-200, crops to arbitrary widths);
//   * tile rows are dealt to the XCDs in stripes (neighbours in x share an L2) through a workgroup -> tile table; a second table
//     holds the tiles in the sequence every XCD walks when the XCDs own z chunks instead (chunk_xcd_order, staged_layout.hpp).
#include "staged2.hpp"
#include "staged_common.hpp"

#include <vector>

namespace fimex_amd {

namespace {

// Where the stencil of an output cell lies (see build_staged2_form, staged2.hpp): px / py, or pos / xf / yf (entry_need, stencil_math.hpp).
struct NeedSource {
    const double* px = nullptr;
    const double* py = nullptr;
    const uint32_t* pos = nullptr;
    const float* xf = nullptr;
    const float* yf = nullptr;
};

template <int STENCIL>
__device__ __forceinline__ CellNeed need_of(const NeedSource& n, size_t cell, int64_t ix, int64_t iy)
{
    if (n.px != nullptr) return classify<STENCIL>(n.px[cell], n.py[cell], ix, iy);
    return entry_need<STENCIL>(n.pos[cell], STENCIL == 2 ? n.xf[cell] : 0.f, STENCIL == 2 ? n.yf[cell] : 0.f, ix);
}

// One workgroup per tile, on the tile's footprint (TileFootprint, staged_common.hpp).  emit == 0: counts the 16-byte chunks of the
// tile's row segments (tiles[t].nChunks, kTileTooLarge = does not fit).  emit == 1: writes the chunk list and every output cell's
// LDS offsets (16 bits per stencil row, in elements).
// cpc: source cells per 16-byte chunk (4 for float slices, 8 / 16 for slices of 2- / 1-byte elements); LDS offsets count elements.
template <int STENCIL>
__global__ void __launch_bounds__(kBlock) tile_scan(NeedSource need, int64_t ix, int64_t iy,
                                                    uint32_t outX, uint32_t outY, uint32_t tileH, StagedTile* __restrict__ tiles,
                                                    uint32_t capChunks, int emit, uint32_t* __restrict__ chunkOff,
                                                    uint32_t* __restrict__ ldsA, uint32_t* __restrict__ ldsB, uint32_t cpc)
{
    __shared__ TileFootprint fp;
    const uint32_t t = blockIdx.x;
    const StagedTile T = tiles[t];
    if (T.rsv[0] != 0) return;  // not staged (see refine_bands, staged_layout.hpp)
    const uint32_t nCells = T.w * tileH;
    auto cells = [&](auto&& f) {
        for (uint32_t e = threadIdx.x; e < nCells; e += kBlock) {
            const uint32_t y = T.y0 + e / T.w, x = T.x0 + e % T.w;
            if (y >= outY) continue;
            const size_t cell = (size_t)y * outX + x;
            f(cell, need_of<STENCIL>(need, cell, ix, iy));
        }
    };
    const int nr = fp.scan(cells);
    const bool fits = nr >= 0 && fp.segments(nr, ix, iy, cpc, capChunks);
    if (!emit) {
        if (threadIdx.x == 0) tiles[t].nChunks = fits ? fp.rowChunk[nr] : kTileTooLarge;
        return;
    }
    if (nr < 0) return;
    const uint32_t total = fp.rowChunk[nr];
    for (uint32_t c = threadIdx.x; c < total; c += kBlock) {
        uint32_t lo = 0, hi = (uint32_t)nr - 1;  // last row whose first chunk <= c and that holds chunks
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (fp.rowChunk[mid] <= c) lo = mid; else hi = mid - 1;
        }
        chunkOff[T.chunkBase + c] = (uint32_t)(fp.segment_start((int)lo, ix) + cpc * (int64_t)(c - fp.rowChunk[lo]));
    }
    cells([&](size_t cell, const CellNeed& c) {
        uint32_t a, b;
        fp.offsets(c, cpc, a, b);
        ldsA[cell] = a;
        if (STENCIL == 4) ldsB[cell] = b;
    });
}

template <int STENCIL>
bool build_shape(const fimex_amd_regrid_plan& plan, Staged2Plan& s, const NeedSource& need, hipStream_t stream, const Shape2& sh, uint32_t stripe,
                 uint32_t cpc)
{
    const uint32_t outX = (uint32_t)plan.outX, outY = (uint32_t)plan.outY;
    const uint32_t tileH = sh.tileH;
    const uint32_t nBands = (uint32_t)ceil_div(outY, tileH);
    // the ring holds `depth` slots, each large enough for any tile (chunks rounded up to whole wave instructions)
    const uint32_t cap = tile_chunk_cap(sh.ldsBytes, sh.depth, (uint32_t)sh.kmax, (uint32_t)sh.nt, cpc);
    const uint32_t step = tile_width_step(sh.tileW);
    // Tiles (staged_layout.hpp): every band starts as tiles of the widest shape; the scan counts every tile's chunks, refine_bands
    // narrows or splits what does not fit, until everything fits or is a gather tile.  Too many cells in gather tiles: no staged plan.
    std::vector<StagedTile> tiles;
    std::vector<uint32_t> bandOf;
    std::vector<std::vector<StagedTile>> rows(nBands);
    std::vector<uint32_t> rowW(nBands, widest_tile(sh.tileW, step, outX));
    for (uint32_t b = 0; b < nBands; ++b) uniform_row(b * tileH, rowW[b], outX, rows[b]);
    DeviceArray<StagedTile> dTiles;
    for (int pass = 0;; ++pass) {
        flatten_bands(rows, tiles, bandOf);
        if (tiles.size() > 0x7FFFFFFFu / 8) return false;
        dTiles.allocate(tiles.size());
        FA_HIP(hipMemcpyAsync(dTiles.get(), tiles.data(), tiles.size() * sizeof(StagedTile), hipMemcpyHostToDevice, stream));
        tile_scan<STENCIL><<<(uint32_t)tiles.size(), kBlock, 0, stream>>>(need, (int64_t)plan.inX, (int64_t)plan.inY, outX, outY, tileH,
                                                                       dTiles.get(), cap, 0, nullptr, nullptr, nullptr, cpc);
        FA_HIP(hipGetLastError());
        FA_HIP(hipMemcpyAsync(tiles.data(), dTiles.get(), tiles.size() * sizeof(StagedTile), hipMemcpyDeviceToHost, stream));
        FA_HIP(hipStreamSynchronize(stream));
        if (!refine_bands(rows, rowW, step, outX, tiles.data())) break;
        if (pass > 64) return false;
    }
    if (gather_share_too_large(tiles)) return false;
    size_t total = 0;
    FA_REQUIRE(assign_chunk_bases(tiles, total), "staged plan: too many chunks");
    if (total > 0xFFFFFFFFull) return false;
    FA_HIP(hipMemcpyAsync(dTiles.get(), tiles.data(), tiles.size() * sizeof(StagedTile), hipMemcpyHostToDevice, stream));
    const size_t n = plan.outX * plan.outY;
    s.chunkOff.allocate(std::max<size_t>(total, 1));
    s.ldsA.allocate(n);
    s.ldsB.allocate(STENCIL == 4 ? n : 0);
    tile_scan<STENCIL><<<(uint32_t)tiles.size(), kBlock, 0, stream>>>(need, (int64_t)plan.inX, (int64_t)plan.inY, outX, outY, tileH,
                                                                   dTiles.get(), cap, 1, s.chunkOff.get(), s.ldsA.get(), s.ldsB.get(), cpc);
    FA_HIP(hipGetLastError());
    const std::vector<uint32_t> order = xcd_order(bandOf, nBands, stripe);  // workgroup -> tile
    s.order.allocate(order.size());
    FA_HIP(hipMemcpyAsync(s.order.get(), order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    // and the table of the chunk-per-XCD order: cohorts of 8 bands x 4 tiles (STAGE2_COHORT_BANDS / _TILES), one XCD's 32 CUs
    const std::vector<uint32_t> orderCx = chunk_xcd_order(tiles, bandOf, sh.tileW, (uint32_t)std::max(1, tuning("STAGE2_COHORT_BANDS", 8)),
                                                          (uint32_t)std::max(1, tuning("STAGE2_COHORT_TILES", 4)));
    s.orderChunkXcd.allocate(orderCx.size());
    FA_HIP(hipMemcpyAsync(s.orderChunkXcd.get(), orderCx.data(), orderCx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    FA_HIP(hipStreamSynchronize(stream));
    s.tiles = std::move(dTiles);
    s.nt = (uint32_t)sh.nt;
    s.per = (uint32_t)sh.per;
    s.kmax = (uint32_t)sh.kmax;
    s.tileH = tileH;
    s.tileWMax = sh.tileW;
    s.nTiles = (uint32_t)tiles.size();
    s.gridX = (uint32_t)order.size();
    s.ldsBytes = sh.ldsBytes;
    s.depth = sh.depth;
    s.totalChunks = total;
    s.stagedCells = total * cpc;
    s.valid = true;
    return true;
}

}  // namespace

bool build_staged2_form(const fimex_amd_regrid_plan& plan, Staged2Plan& form, const double* d_px, const double* d_py, const Shape2& sh,
                        uint32_t stripe, uint32_t cpc, hipStream_t stream)
{
    const NeedSource need = d_px ? NeedSource{d_px, d_py} : NeedSource{nullptr, nullptr, plan.pos.get(), plan.xf.get(), plan.yf.get()};
    switch (plan.kind) {
    case PlanKind::Nearest: return build_shape<1>(plan, form, need, stream, sh, stripe, cpc);
    case PlanKind::Bilinear: return build_shape<2>(plan, form, need, stream, sh, stripe, cpc);
    case PlanKind::Bicubic: return build_shape<4>(plan, form, need, stream, sh, stripe, cpc);
    default: return false;
    }
}

// Workgroup shape by stencil (tuning: STAGE2_NT / STAGE2_TW / STAGE2_LDS / STAGE2_STRIPE); false: no staged form for this
// plan (positions without spatial coherence), the caller keeps the gather kernels.
static bool build_staged2_shape(fimex_amd_regrid_plan& plan, Staged2Plan& target, int ntWanted, const double* d_px, const double* d_py, hipStream_t stream)
{
    if (plan.outX * plan.outY == 0) return false;
    // the float form of the bicubic stencil is as light as the bilinear one: it takes the bilinear shapes
    const bool cubic = plan.kind == PlanKind::Bicubic && !plan.bicubicFast;
    // measured on the benchmark plan (round 2's sweeps, profiles/LAB_NOTES_r01_r02.md): 1024 threads on 512 x 8 tiles (one workgroup per CU) for the
    // 1 x 1 and 2 x 2 stencils.  With the tile-major launch order 512 threads on 256 x 8 tiles (two workgroups per CU) run the
    // bilinear launch 2.5-3.5 % faster on two boxes (2.19 against 2.27 ms) and 4 % slower on two others (2.41 against 2.31 ms), and
    // lose on the 1 x 1 stencil and on short batches everywhere: the shape that behaves the same on every box is kept.  The 4 x 4
    // stencil in float arithmetic takes 256 x 8 tiles on 512 threads (its halo makes taller or wider tiles stage more), in the
    // reference's arithmetic it is FP64-bound and prefers 128 x 8 tiles on 512 threads.
    const int nt = ntWanted > 0 ? ntWanted : tuning("STAGE2_NT", (cubic || plan.bicubicFast) ? 512 : 1024);
    Shape2 sh{};
    sh.nt = nt;
    sh.per = cubic ? 2 : 4;
    // chunks per lane: 1024 threads hold one slot of at most 80 KB
    sh.kmax = cubic ? (nt == 256 ? 4 : 3) : (nt == 1024 ? 5 : 6);
    sh.tileW = (uint32_t)tuning("STAGE2_TW", cubic ? 64 * (nt / 256) : nt / 2);
    // LDS of one workgroup: 3 / 2 / 1 workgroups per CU (160 KB)
    sh.ldsBytes = (uint32_t)tuning("STAGE2_LDS_KB", nt == 256 ? 52 : (nt == 512 ? 79 : 159)) * 1024u;
    sh.depth = (uint32_t)tuning("STAGE2_DEPTH", 2);
    if (!finish_shape(sh, 32)) return false;
    // tile rows go to the XCDs one by one (row r to XCD r % 8): with the tile-major launch order the eight XCDs then work on eight
    // neighbouring tile rows at any time.  (With the chunk-major order stripes of 8 rows per XCD fetched 10.2 instead of 11.1 GB for
    // the bilinear launch at the same time; with the tile-major order stripes of 2, 4 or 8 rows lose 3-6 %.)
    const uint32_t stripe = (uint32_t)std::max(1, tuning("STAGE2_STRIPE", 1));
    return build_staged2_form(plan, target, d_px, d_py, sh, stripe, 4, stream);
}

bool build_staged2_plan(fimex_amd_regrid_plan& plan, const double* d_px, const double* d_py, hipStream_t stream)
{
    if (!build_staged2_shape(plan, plan.staged2, 0, d_px, d_py, stream)) return false;
    // the bilinear plan also holds the 512-thread shape (two workgroups per CU): faster on some devices for long batches,
    // slower on others and for short ones -- fimex_amd_regrid_plan_tune_device decides on the spot, the default stays
    if (plan.kind == PlanKind::Bilinear && plan.staged2.nt == 1024 && tuning("STAGE2_ALT", 1) != 0)
        build_staged2_shape(plan, plan.staged2Alt, 512, d_px, d_py, stream);
    // likewise the 4 x 4 stencil in float arithmetic: 256 threads on 128 x 8 tiles (three workgroups per CU) beside 512 threads on
    // 256 x 8 (2.38 against 2.41 ms in one process, round 2, profiles/LAB_NOTES_r01_r02.md)
    if (plan.kind == PlanKind::Bicubic && plan.bicubicFast && plan.staged2.nt == 512 && tuning("STAGE2_ALT", 1) != 0)
        build_staged2_shape(plan, plan.staged2Alt, 256, d_px, d_py, stream);
    return true;
}

}  // namespace fimex_amd
