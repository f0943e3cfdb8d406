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
//   * tile rows are dealt to the XCDs in stripes (neighbours in x share an L2) through a workgroup -> tile table.
#include "staged2.hpp"
#include "staged_common.hpp"

#include <vector>

namespace fimex_amd {

namespace {

// One workgroup per tile.  emit == 0: counts the 16-byte chunks of the tile's row segments (tiles[t].nChunks, ~0u = does not
// fit).  emit == 1: writes the chunk list and every output cell's LDS offsets (16 bits per stencil row, in floats).
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

// cpc: source cells per 16-byte chunk (4 for float slices, 8 / 16 for slices of 2- / 1-byte elements); LDS offsets count elements.
template <int STENCIL>
__global__ void __launch_bounds__(kBlock) tile_scan(NeedSource need, int64_t ix, int64_t iy,
                                                    uint32_t outX, uint32_t outY, uint32_t tileH, StagedTile* __restrict__ tiles,
                                                    uint32_t capChunks, int emit, uint32_t* __restrict__ chunkOff,
                                                    uint32_t* __restrict__ ldsA, uint32_t* __restrict__ ldsB, uint32_t cpc)
{
    __shared__ int shRmin, shRmax, shFail;
    __shared__ int rowMin[kMaxRows], rowMax[kMaxRows];
    __shared__ uint32_t rowChunk[kMaxRows + 1];
    const uint32_t t = blockIdx.x;
    const StagedTile T = tiles[t];
    if (T.rsv[0] != 0) return;  // not staged (see build_shape)
    const uint32_t nCells = T.w * tileH;
    if (threadIdx.x == 0) { shRmin = 0x7FFFFFFF; shRmax = -1; shFail = 0; }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < nCells; e += kBlock) {
        const uint32_t y = T.y0 + e / T.w, x = T.x0 + e % T.w;
        if (y >= outY) continue;
        const size_t cell = (size_t)y * outX + x;
        const CellNeed c = need_of<STENCIL>(need, cell, ix, iy);
        if (c.valid) { atomicMin(&shRmin, (int)c.ya); atomicMax(&shRmax, (int)c.yb); }
    }
    __syncthreads();
    const int rmin = shRmin;
    const int nr = (shRmax >= rmin) ? shRmax - rmin + 1 : 0;
    if (nr > kMaxRows) {
        if (threadIdx.x == 0 && !emit) tiles[t].nChunks = 0xFFFFFFFFu;
        return;
    }
    for (int i = threadIdx.x; i < nr; i += kBlock) { rowMin[i] = 0x7FFFFFFF; rowMax[i] = -0x7FFFFFFF; }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < nCells; e += kBlock) {
        const uint32_t y = T.y0 + e / T.w, x = T.x0 + e % T.w;
        if (y >= outY) continue;
        const size_t cell = (size_t)y * outX + x;
        const CellNeed c = need_of<STENCIL>(need, cell, ix, iy);
        if (c.valid)
            for (int64_t r = c.ya; r <= c.yb; ++r) {
                atomicMin(&rowMin[r - rmin], (int)c.xa);
                atomicMax(&rowMax[r - rmin], (int)c.xb);
            }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t layer = ix * iy;
        uint32_t acc = 0;
        for (int i = 0; i < nr; ++i) {
            rowChunk[i] = acc;
            if (rowMax[i] >= rowMin[i]) {
                // the segment starts on a 16-byte boundary of the SLICE (the DMA moves 16 bytes per lane; aligned pieces stay
                // inside one line): it may begin up to 3 cells before the first cell needed, in the row above for x < 0
                const int64_t first = (int64_t)(rmin + i) * ix + rowMin[i];
                int64_t start = first & ~(int64_t)(cpc - 1);
                const uint32_t nch = (uint32_t)((first - start + (rowMax[i] - rowMin[i])) / cpc + 1);
                // a last chunk that would cross the end of the slice is moved back instead (unaligned, still whole; slices of
                // stored types hold a multiple of 4 bytes, so the chunk still starts on a 4-byte boundary)
                if (start + cpc * (int64_t)nch > layer) start = layer - cpc * (int64_t)nch;
                if (start < 0) shFail = 1;
                rowMin[i] = (int)(start - (int64_t)(rmin + i) * ix);  // column of the segment's first cell, may be negative
                acc += nch;
            }
        }
        rowChunk[nr] = acc;
        if (acc > capChunks) shFail = 1;
    }
    __syncthreads();
    if (!emit) {
        if (threadIdx.x == 0) tiles[t].nChunks = shFail ? 0xFFFFFFFFu : rowChunk[nr];
        return;
    }
    const uint32_t total = rowChunk[nr];
    for (uint32_t c = threadIdx.x; c < total; c += kBlock) {
        uint32_t lo = 0, hi = (uint32_t)nr - 1;  // last row whose first chunk <= c and that holds chunks
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (rowChunk[mid] <= c) lo = mid; else hi = mid - 1;
        }
        chunkOff[T.chunkBase + c] = (uint32_t)((int64_t)(rmin + (int)lo) * ix + rowMin[lo] + cpc * (int64_t)(c - rowChunk[lo]));
    }
    for (uint32_t e = threadIdx.x; e < nCells; e += kBlock) {
        const uint32_t y = T.y0 + e / T.w, x = T.x0 + e % T.w;
        if (y >= outY) continue;
        const size_t cell = (size_t)y * outX + x;
        const CellNeed c = need_of<STENCIL>(need, cell, ix, iy);
        uint32_t a = kInvalidPos, b = kInvalidPos;
        if (c.valid) {
            uint32_t off[4];
            for (int r = 0; r < 4; ++r) {
                const int64_t row = (c.ya + r <= c.yb) ? c.ya + r : c.yb;  // missing rows repeat the last one
                const int i = (int)(row - rmin);
                off[r] = rowChunk[i] * cpc + (uint32_t)(c.xa - rowMin[i]);
            }
            a = off[0] | (off[1] << 16);
            b = off[2] | (off[3] << 16);
        }
        ldsA[cell] = a;
        if (STENCIL == 4) ldsB[cell] = b;
    }
}

template <int STENCIL>
bool build_shape(const fimex_amd_regrid_plan& plan, Staged2Plan& s, const NeedSource& need, hipStream_t stream, const Shape2& sh, uint32_t stripe,
                 uint32_t cpc)
{
    const uint32_t outX = (uint32_t)plan.outX, outY = (uint32_t)plan.outY;
    const uint32_t tileH = sh.tileH;
    const uint32_t nBands = (uint32_t)ceil_div(outY, tileH);
    // the ring holds `depth` slots, each large enough for any tile (chunks rounded up to whole wave instructions)
    uint32_t cap = std::min<uint32_t>(slot_chunks(sh.ldsBytes, sh.depth), (uint32_t)sh.kmax * sh.nt);
    cap = std::min<uint32_t>(cap, 65535u / cpc);  // 16-bit LDS offsets, in elements
    const uint32_t step = sh.tileW >= 128 ? 64u : 32u;  // tile widths are multiples of this (a wave stores 64 consecutive cells)
    // Tiles: every tile row starts as tiles of the widest shape.  A tile that does not fit (too many chunks for a slot, too
    // many source rows) makes its row narrower when most tiles of the row fail (the row's cells cover more source: rows near
    // the pole of the benchmark plan), otherwise it is split in two; at the narrowest width it becomes a gather tile
    // (rsv[0] = 1: the kernel reads its stencils from memory).  More than 1/8 of the cells that way: no staged plan.
    const uint32_t widest = std::min(sh.tileW, (outX + step - 1) / step * step);
    std::vector<StagedTile> tiles;
    std::vector<uint32_t> bandOf;
    auto uniform_row = [&](uint32_t b, uint32_t w, std::vector<StagedTile>& out) {
        for (uint32_t x0 = 0; x0 < outX; x0 += w) {
            StagedTile t{};
            t.x0 = x0;
            t.y0 = b * tileH;
            t.w = std::min(w, outX - x0);
            out.push_back(t);
        }
    };
    std::vector<std::vector<StagedTile>> rows(nBands);
    std::vector<uint32_t> rowW(nBands, widest);
    for (uint32_t b = 0; b < nBands; ++b) uniform_row(b, widest, rows[b]);
    DeviceArray<StagedTile> dTiles;
    for (int pass = 0;; ++pass) {
        tiles.clear();
        bandOf.clear();
        for (uint32_t b = 0; b < nBands; ++b)
            for (const StagedTile& t : rows[b]) { tiles.push_back(t); bandOf.push_back(b); }
        if (tiles.size() > 0x7FFFFFFFu / 8) return false;
        dTiles.allocate(tiles.size());
        FA_HIP(hipMemcpyAsync(dTiles.get(), tiles.data(), tiles.size() * sizeof(StagedTile), hipMemcpyHostToDevice, stream));
        tile_scan<STENCIL><<<(uint32_t)tiles.size(), kBlock, 0, stream>>>(need, (int64_t)plan.inX, (int64_t)plan.inY, outX, outY, tileH,
                                                                       dTiles.get(), cap, 0, nullptr, nullptr, nullptr, cpc);
        FA_HIP(hipGetLastError());
        FA_HIP(hipMemcpyAsync(tiles.data(), dTiles.get(), tiles.size() * sizeof(StagedTile), hipMemcpyDeviceToHost, stream));
        FA_HIP(hipStreamSynchronize(stream));
        bool again = false;
        size_t i = 0;
        for (uint32_t b = 0; b < nBands; ++b) {
            const size_t n = rows[b].size();
            size_t failed = 0;
            for (size_t k = 0; k < n; ++k) {
                rows[b][k] = tiles[i + k];
                if (tiles[i + k].rsv[0] == 0 && tiles[i + k].nChunks == 0xFFFFFFFFu) ++failed;
            }
            i += n;
            if (failed == 0) continue;
            again = true;
            if (2 * failed > n && rowW[b] > step) {  // the whole row is too heavy: narrower tiles throughout
                rowW[b] -= step;
                rows[b].clear();
                uniform_row(b, rowW[b], rows[b]);
                continue;
            }
            std::vector<StagedTile> next;
            for (const StagedTile& t : rows[b]) {
                if (t.rsv[0] != 0 || t.nChunks != 0xFFFFFFFFu) { next.push_back(t); continue; }
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
        if (!again) break;
        if (pass > 64) return false;
    }
    size_t gatherCells = 0, liveCells = 0;
    for (const StagedTile& t : tiles) {
        if (t.rsv[0] != 0) gatherCells += t.w;
        if (t.rsv[0] != 0 || t.nChunks != 0) liveCells += t.w;
    }
    if (gatherCells * 8 > liveCells) return false;  // positions without spatial coherence: the gather kernels serve them better
    size_t total = 0;
    for (auto& t : tiles) {
        FA_REQUIRE(total <= 0xFFFFFFFFu, "staged plan: too many chunks");
        t.chunkBase = (uint32_t)total;
        total += t.nChunks;
    }
    if (total > 0xFFFFFFFFull) return false;
    FA_HIP(hipMemcpyAsync(dTiles.get(), tiles.data(), tiles.size() * sizeof(StagedTile), hipMemcpyHostToDevice, stream));
    const size_t n = plan.outX * plan.outY;
    s.chunkOff.allocate(std::max<size_t>(total, 1));
    s.ldsA.allocate(n);
    s.ldsB.allocate(STENCIL == 4 ? n : 0);
    tile_scan<STENCIL><<<(uint32_t)tiles.size(), kBlock, 0, stream>>>(need, (int64_t)plan.inX, (int64_t)plan.inY, outX, outY, tileH,
                                                                   dTiles.get(), cap, 1, s.chunkOff.get(), s.ldsA.get(), s.ldsB.get(), cpc);
    FA_HIP(hipGetLastError());
    // workgroup -> tile: workgroups are dealt round-robin over the XCDs (b % 8 shares an L2); tile rows go to the XCDs in
    // stripes of `stripe` rows, so that neighbours in x (and, inside a stripe, in y) run on the same XCD and meet in its L2
    // (stripes of about `stripe` rows, their number a multiple of the XCD count so that every XCD gets equally many)
    std::vector<std::vector<uint32_t>> perXcd(kXcds);
    uint32_t nStripes = (uint32_t)((nBands + stripe * kXcds / 2) / (stripe * kXcds)) * kXcds;
    if (nStripes < (uint32_t)kXcds) nStripes = kXcds;
    if (nStripes > nBands) nStripes = std::max<uint32_t>(nBands / kXcds * kXcds, 1);
    // (fewer tile rows than XCDs -- wide, short targets such as cross-sections: the tiles themselves are dealt round-robin)
    for (size_t i = 0; i < tiles.size(); ++i)
        perXcd[nBands < (uint32_t)kXcds ? i % kXcds : ((uint64_t)bandOf[i] * nStripes / nBands) % kXcds].push_back((uint32_t)i);
    size_t longest = 0;
    for (auto& l : perXcd) longest = std::max(longest, l.size());
    std::vector<uint32_t> order(longest * kXcds, 0xFFFFFFFFu);
    for (int x = 0; x < kXcds; ++x)
        for (size_t k = 0; k < perXcd[x].size(); ++k) order[k * kXcds + x] = perXcd[x][k];
    s.order.allocate(order.size());
    FA_HIP(hipMemcpyAsync(s.order.get(), order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
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
