// Second LDS-staged regrid form, what its three translation units share: staged2_plan.hip (tile scan, shape choice, plan),
// staged2.hip (float kernel and launch), staged2_typed.hip (stored-type kernel, form cache and launch), staged2_vector.hip and
// staged2_vector_typed.hip (the pair kernels on float slices and on stored types).
#pragma once

#include "plan.hpp"

#include <algorithm>

namespace fimex_amd {

struct Shape2 {
    int nt, per, kmax;
    uint32_t depth;         // slices of the ring: one or two in flight while one is interpolated
    uint32_t tileW, tileH;  // widest tile
    uint32_t ldsBytes;
};

// Checks a shape whose nt, per, tileW, ldsBytes and depth are set (from defaults or tuning switches), derives tileH and clamps
// the LDS to what a workgroup may have.  Tile widths are multiples of `widthStep`.  false: no staged form with this shape.
inline bool finish_shape(Shape2& sh, uint32_t widthStep)
{
    if (!(sh.nt == 256 || sh.nt == 512 || sh.nt == 1024)) return false;
    const uint32_t outputs = (uint32_t)(sh.nt * sh.per);
    if (sh.tileW < widthStep || sh.tileW % widthStep != 0 || outputs % sh.tileW != 0) return false;
    sh.tileH = outputs / sh.tileW;
    if (sh.ldsBytes > 160u * 1024u - 64u) sh.ldsBytes = 160u * 1024u - 64u;
    if (sh.ldsBytes < 16u * 1024u) return false;
    sh.depth = sh.depth == 3 ? 3u : 2u;
    return true;
}

// staged2_plan.hip: tiles, chunk lists and LDS offsets of `form` for slices with `cpc` source cells per 16-byte chunk (4 for
// float slices, 8 / 16 for 2- / 1-byte elements).  Where the stencil of an output cell lies: from the caller's positions (plan
// creation), or, with d_px == nullptr -- the forms of stored types are built on first use, long after the positions are gone --
// from the gather plan the positions were turned into.  false: no staged form (positions without spatial coherence).
bool build_staged2_form(const fimex_amd_regrid_plan& plan, Staged2Plan& form, const double* d_px, const double* d_py, const Shape2& sh,
                        uint32_t stripe, uint32_t cpc, hipStream_t stream);

// staged2_typed.hip: the plan's staged form for slices of elemBytes-byte elements (2 or 1), built on first use and kept with the
// plan; nullptr: none.  The stored-type kernel and the stored-type pair kernel (staged2_vector_typed.hip) run on it.
const Staged2Plan* staged2_typed_form(const fimex_amd_regrid_plan& plan, uint32_t elemBytes, hipStream_t stream);

namespace {

struct Staged2Args {
    const float* in;
    float* out;
    const StagedTile* tiles;
    const uint32_t* order;
    const uint32_t* chunkOff;
    const uint32_t *ldsA, *ldsB;
    const uint32_t* pos;  // gather plan (gather.hip): source cell of the stencil's corner, for the tiles that are not staged
    const float *xf, *yf;
    const double *xfd, *yfd;
    uint32_t outX, outY, tileH;
    uint32_t inX;
    uint32_t inBytes;    // one source slice
    uint32_t nOut;
    uint32_t nz;
    uint32_t zStart[kMaxZChunks + 1];  // slices [zStart[c], zStart[c + 1]) belong to z chunk c
    uint32_t nZChunks;    // > 0: flat grid, the z chunks of a tile are consecutive workgroups of one XCD; 0: z chunk = blockIdx.y
    uint32_t chunkPerXcd;  // flat grid only.  1: the chunk-per-XCD order, `order` is chunk_xcd_order's table (chunk_xcd_workgroup)
    uint32_t slotChunks;  // 16-byte chunks of one slot of the slice ring (a multiple of 64: whole wave instructions)
    uint32_t flags;      // tuning build only: 1 no source loads, 2 no result stores (STAGE2_ABLATE); the float kernel's store policy from 8 on
};

// everything of the kernels' argument but the z chunks: slices of elemBytes-byte elements through form `s` of the plan
inline Staged2Args staged2_args(const fimex_amd_regrid_plan& plan, const Staged2Plan& s, const void* d_in, void* d_out, uint32_t elemBytes, size_t nz)
{
    Staged2Args a{};
    a.in = static_cast<const float*>(d_in);
    a.out = static_cast<float*>(d_out);
    a.tiles = s.tiles.get();
    a.order = s.order.get();
    a.chunkOff = s.chunkOff.get();
    a.ldsA = s.ldsA.get();
    a.ldsB = s.ldsB.get();
    a.pos = plan.pos.get();
    a.xf = plan.xf.get();
    a.yf = plan.yf.get();
    a.xfd = plan.xfd.get();
    a.yfd = plan.yfd.get();
    a.outX = (uint32_t)plan.outX;
    a.outY = (uint32_t)plan.outY;
    a.tileH = s.tileH;
    a.inX = (uint32_t)plan.inX;
    a.inBytes = (uint32_t)(plan.inX * plan.inY * elemBytes);
    a.nOut = (uint32_t)(plan.outX * plan.outY);
    a.nz = (uint32_t)nz;
    a.slotChunks = slot_chunks(s.ldsBytes, s.depth);
    a.flags = (uint32_t)tuning("STAGE2_ABLATE", 0);
    return a;
}

// the z chunks of a launch into the kernels' argument; flat: the grid is one-dimensional, in tile-major order (flat_workgroup,
// staged_layout.hpp) until the launcher says otherwise
inline void set_z_chunks(Staged2Args& a, const ZChunks& zc, bool flat)
{
    std::copy(zc.zStart, zc.zStart + kMaxZChunks + 1, a.zStart);
    a.nZChunks = flat ? zc.n : 0u;
    a.chunkPerXcd = 0;
}

// the workgroup shape a float launch runs: the plan's choice (fimex_amd_regrid_plan_tune_device), or STAGE2_USE_ALT 0 / 1 in the
// tuning build
inline const Staged2Plan& staged2_shape_of(const fimex_amd_regrid_plan& plan)
{
    const int forced = tuning("STAGE2_USE_ALT", -1);
    const bool alt = plan.staged2Alt.valid && (forced >= 0 ? forced == 1 : plan.useAlt != 0);
    return alt ? plan.staged2Alt : plan.staged2;
}

// The z chunks of a float launch of nz slices (or pairs of slices) through shape `s`, written into `a`; returns the grid.
// `order` is the plan's LaunchOrder (staged_layout.hpp), STAGE2_ORDER 0 / 1 / 2 replaces it in the tuning build.
// Tile-major order (the default, 1): the chunks of a tile are consecutive workgroups of one XCD, so
// they start together and fetch the tile's per-output plan -- 12 bytes per cell, 0.05 GB per chunk of the benchmark
// launch -- once from memory instead of once per chunk, and the chip as a whole works on eight neighbouring tile rows;
// chunks of one size (about STAGE2_ZPB slices).  Measured on the benchmark plan (round 2's sweeps, profiles/LAB_NOTES_r01_r02.md): bilinear
// 2.40 -> 2.32 ms, nearest 2.32 -> 2.21 ms, 25 slices 0.322 -> 0.303 ms.
// Chunk-per-XCD order (2): the transpose -- XCD x runs z chunk x of every tile, through `s.orderChunkXcd`.  The chip works on the
// same 32 tiles x 8 chunks at any time, but a source line that two tiles need (nearly always vertical neighbours) is asked for
// twice in ONE L2 instead of in two; the per-output plan is fetched by every XCD.  Needs 8 or 16 chunks: batches too short for
// that (chunk_xcd_chunk_count) and launches with allowChunkPerXcd == false run tile-major.
// Chunk-major order (0, round 1 and early round 2): all tiles of chunk 0, then chunk 1, ...; the chunks shrink
// towards the end of the launch so that the last workgroups are short ones (STAGE2_ZTAIL).  The rules: float_z_chunks.
inline dim3 staged2_z_chunks(Staged2Args& a, const Staged2Plan& s, size_t nz, int order, bool allowChunkPerXcd)
{
    order = tuning("STAGE2_ORDER", order);
    const bool tileMajor = order != kChunkMajor;
    const uint32_t zpb = tileMajor ? staged2_zpb() : (uint32_t)tuning("STAGE2_ZPB", 50);
    const uint32_t ztail = tileMajor ? 0u : (uint32_t)tuning("STAGE2_ZTAIL", 10);  // 0: chunks of one size
    order = launch_order_of(order, allowChunkPerXcd, nz, zpb);  // (staged2_float_launch_order, staged2.hip, answers the same)
    ZChunks zc;
    FA_REQUIRE(float_z_chunks(nz, order, zpb, ztail, zc), "too many z chunks for one launch");
    set_z_chunks(a, zc, tileMajor);
    if (order == kChunkPerXcd) {
        a.chunkPerXcd = 1;
        a.order = s.orderChunkXcd.get();
        return dim3(s.nTiles * zc.n, 1, 1);
    }
    return dim3(tileMajor ? s.gridX * zc.n : s.gridX, tileMajor ? 1u : zc.n, 1);
}

}  // namespace
}  // namespace fimex_amd
