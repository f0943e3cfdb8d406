"""The first staged form (staged.hip: staged_apply<STENCIL, PER, KMAX, NBUF, T>) at every workgroup shape of its ladder, on every
element type, at the edges of its fit rule and through its slice loop.  Which switch reaches what: STAGE_PER + STAGE_K pin the
shape {outputs per lane, chunks per lane} when the plan is built (a plan that does not fit it holds no first form); STAGED2=0 and
TYPED_STAGED2=0 keep the second form away, so that nearest and bilinear floats and stored types run this one and plan.info() speaks
of it; STAGED_MIN_NZ=1 lets batches of one to three slices in; STAGE_ZPB sets the slices per z chunk, STAGE_NBUF and TYPED_NBUF the
ring depth (1, 3, 4, 6 where launch_staged admits them for the shape, else 2), STAGE_ORDER=1 the flat tile-major grid and XCD the
tile -> XCD map.  The product build reads no switch: there bicubic in the reference's arithmetic reaches all four of its shapes by
geometry alone (targets of one tile row), and STAGE_ZPB's default of 50 gives two and three z chunks at 51 and 101 slices.
Positions are affine maps, so that a tile's footprint can be computed: GEOMS is the table of every geometry used here with the
shape it lands in, the round ((k - 1) * 256, k * 256] of 4-cell chunks its fullest tile ends in (the kernel's DMA rounds for float
and 1-byte elements; 2-byte elements move padded 16-byte pieces in kmax / 2 + 1 rounds, which the -wide- cases fill) and the source
rows its tallest tile spans; the CPU tests hold the table to first_form_shape, the fit rule of build_staged_plan restated on
tile_chunks, and the GPU tests hold the plans the library builds to the same numbers.  plan.info() gives the tile size and the
staged cells, not the chunks per lane: rungs of one tile height ({4,4} and {4,6}, {8,8} and {8,12}, {2,3} and {2,4}, {4,6} and
{4,8}) are told apart by pinning one (test_rungs_pinned_on_the_ladder_geometries), and in the forced tests the pinned rung is the
only one the plan can hold.  Every comparison is bit for bit: float slices with cases.same against oracle.interpolate_values, stored
types with np.array_equal against the oracle's three steps, and every output lies between guard bytes that must survive (the typed
kernel stores single bytes and shorts), which is why the launchers here are guarded ones of their own.  Bicubic is the reference's
arithmetic throughout.  One geometry is not in the table: the map that overshoots the source (test_tiles_without_chunks_...), whose
cells outside the source the numpy footprint does not model; there the plan is only held to its tile size.
"""
import collections

import numpy as np
import pytest

import cases
import oracle
from test_gpu_staged2_shapes import MAX_ROWS, affine, tile_chunks

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


# stencil -> tile width, shapes {outputs per lane, chunks per lane} in the order build_staged_plan tries them
LADDER = {1: (128, ((4, 4), (4, 6), (8, 8))), 2: (128, ((4, 4), (4, 6), (8, 8), (8, 12))), 4: (32, ((2, 3), (2, 4), (4, 6), (4, 8)))}
METHOD = {1: oracle.NEAREST, 2: oracle.BILINEAR, 4: oracle.BICUBIC}
SHAPES = [(st, per, k) for st, (_, shapes) in LADDER.items() for per, k in shapes]
TYPES = (np.int8, np.uint8, np.int16, np.uint16)
FIRST_ONLY = {"STAGED2": "0", "TYPED_STAGED2": "0", "STAGED_MIN_NZ": "1"}


def tile_height(stencil, per):
    return per * 256 // LADDER[stencil][0]


def first_form_shape(stencil, px, py, inX, inY, outX, outY, force=None):
    """The fit rule of build_staged_plan: the first shape of the ladder (force: only that one, as STAGE_PER and STAGE_K do) whose
    tiles all hold at most kmax * 256 chunks of 4 cells and span at most MAX_ROWS source rows.  Returns the shape, or None, and the
    chunks per tile at the tile size of that shape (None: of the last one tried; a tile with too many rows counts None)."""
    tw, shapes = LADDER[stencil]
    counts = None
    for per, kmax in shapes:
        if force is None or force == (per, kmax):
            counts = tile_chunks(stencil, px, py, inX, inY, outX, outY, tw, tile_height(stencil, per), cpc=4)
            if None not in counts and max(counts) <= kmax * 256:
                return (per, kmax), counts
    return None, counts


def first_rows(stencil, py, outX, outY):
    """first and last source row of every output cell's stencil"""
    ya = (np.floor(py + 0.5) if stencil == 1 else np.floor(py)).astype(np.int64).reshape(outY, outX) - (1 if stencil == 4 else 0)
    return ya, ya + stencil - 1


def row_span(stencil, py, outX, outY, th):
    """source rows the tallest tile spans (tiles of one tile row span the same rows: py does not depend on x here)"""
    ya, yb = first_rows(stencil, py, outX, outY)
    return max(int(yb[y0:y0 + th].max() - ya[y0:y0 + th].min()) + 1 for y0 in range(0, outY, th))


def tile_segments(stencil, px, py, inX, outX, outY, x0, y0, w, h, cpc=4):
    """chunks of every row segment of one tile that holds any (the rows between, which no cell reads, are segments of no chunks)"""
    xa = (np.floor(px + 0.5) if stencil == 1 else np.floor(px)).astype(np.int64).reshape(outY, outX) - (1 if stencil == 4 else 0)
    ya, yb = first_rows(stencil, py, outX, outY)
    t = (slice(y0, y0 + h), slice(x0, x0 + w))
    xa, xb, ya, yb = xa[t], xa[t] + stencil - 1, ya[t], yb[t]
    seg = []
    for row in range(ya.min(), yb.max() + 1):
        use = (ya <= row) & (row <= yb)
        if use.any():
            lo, hi = xa[use].min(), xb[use].max()
            seg.append(int(((row * inX + lo) % cpc + hi - lo) // cpc + 1))
    return seg


# One geometry: px = x * rx + 1.3, py = y * ry + 1.6 on a target of outX x outY; the source holds the footprint and eight cells
# more, its row length rounded up to a multiple of 4 (this form takes no other).  force: the shape pinned with STAGE_PER and
# STAGE_K.  Expected: the shape the plan lands in (None: no first form), the DMA round of the fullest tile at that shape's tile
# size (of the last shape tried where none fits; None: a tile spans too many rows) and the rows of the tallest tile.
G = collections.namedtuple("G", "name stencil outX outY rx ry force shape rounds rows")

GEOMS = [
    # -- the ladder on a target of one tile row, no shape forced: each rung, the ratios that fill a shape to the last chunk, and one
    #    step further (source size and fullest tile in the comment)
    G("nearest-row-4.0", 1, 256, 8, 4.0, 4.0, None, (4, 4), 4, 29),      # 1032 x 40, 1024: exactly at capacity
    G("nearest-row-4.1", 1, 256, 8, 4.1, 4.1, None, (4, 6), 5, 29),      # 1060 x 40, 1048
    G("nearest-row-6.5", 1, 256, 8, 6.5, 6.5, None, (8, 8), 7, 46),      # 1672 x 60, 1656
    G("nearest-row-8.0", 1, 256, 8, 8.0, 8.0, None, (8, 8), 8, 57),      # 2056 x 72, 2040 of 2048
    G("nearest-row-8.1", 1, 256, 8, 8.1, 8.1, None, None, 9, 57),        # 2084 x 72, 2064
    G("bilinear-row-1.9", 2, 256, 8, 1.9, 1.9, None, (4, 4), 4, 15),     # 496 x 23, 915
    G("bilinear-row-3.0", 2, 256, 8, 3.0, 3.0, None, (4, 6), 6, 23),     # 776 x 32, 1536: exactly at capacity
    G("bilinear-row-3.1", 2, 256, 8, 3.1, 3.1, None, (8, 8), 7, 24),     # 804 x 32, 1600
    G("bilinear-row-4.0", 2, 256, 8, 4.0, 4.0, None, (8, 8), 8, 30),     # 1032 x 40, 2048: exactly at capacity
    G("bilinear-row-4.1", 2, 256, 8, 4.1, 4.1, None, (8, 12), 9, 31),    # 1060 x 40, 2096
    G("bilinear-row-6.0", 2, 256, 8, 6.0, 6.0, None, (8, 12), 12, 44),   # 1544 x 56, 3072: exactly at capacity
    G("bilinear-row-6.1", 2, 256, 8, 6.1, 6.1, None, None, 13, 45),      # 1572 x 56, 3120
    G("bicubic-row-2.2", 4, 64, 16, 2.2, 2.2, None, (2, 3), 3, 37),      # 148 x 43, 703
    G("bicubic-row-2.5", 4, 64, 16, 2.5, 2.5, None, (2, 4), 4, 42),      # 168 x 48, 882
    G("bicubic-row-2.8", 4, 64, 16, 2.8, 2.8, None, (4, 6), 5, 46),      # 188 x 52, 1058
    G("bicubic-row-3.4", 4, 64, 16, 3.4, 3.4, None, (4, 8), 7, 55),      # 228 x 62, 1540
    G("bicubic-row-4.0", 4, 64, 16, 4.0, 4.0, None, (4, 8), 8, 64),      # 264 x 72, 2048: exactly at capacity
    G("bicubic-row-4.1", 4, 64, 16, 4.1, 4.1, None, None, 9, 66),        # 272 x 73, 2176
    # -- rungs pinned on those geometries: the shape just before the chosen one does not fit, and a shape that an equally tall
    #    neighbour could be mistaken for (plan.info() names the tile size, not the chunks per lane) does
    G("nearest-row-4.1-forced-4-4", 1, 256, 8, 4.1, 4.1, (4, 4), None, 5, 29),
    G("nearest-row-6.5-forced-4-6", 1, 256, 8, 6.5, 6.5, (4, 6), None, 7, 46),
    G("bilinear-row-3.1-forced-4-6", 2, 256, 8, 3.1, 3.1, (4, 6), None, 7, 24),
    G("bilinear-row-3.1-forced-8-8", 2, 256, 8, 3.1, 3.1, (8, 8), (8, 8), 7, 24),
    G("bilinear-row-4.0-forced-8-8", 2, 256, 8, 4.0, 4.0, (8, 8), (8, 8), 8, 30),
    G("bilinear-row-4.1-forced-8-8", 2, 256, 8, 4.1, 4.1, (8, 8), None, 9, 31),
    G("bicubic-row-4.0-forced-4-6", 4, 64, 16, 4.0, 4.0, (4, 6), None, 8, 64),
    G("bicubic-row-4.0-forced-4-8", 4, 64, 16, 4.0, 4.0, (4, 8), (4, 8), 8, 64),
    G("bicubic-row-2.5-forced-2-3", 4, 64, 16, 2.5, 2.5, (2, 3), None, 4, 42),
    G("bicubic-row-2.8-forced-2-4", 4, 64, 16, 2.8, 2.8, (2, 4), None, 5, 46),
    G("bicubic-row-3.4-forced-4-6", 4, 64, 16, 3.4, 3.4, (4, 6), None, 7, 55),
    # -- every shape forced: 2 x 2 whole tiles, the ragged copy (last tile column three cells short, last tile row of one row),
    #    and 2 x 1 whole tiles at a ratio that puts the fullest tile into the shape's last DMA round
    G("nearest-4-4-whole", 1, 256, 16, 1.5, 1.5, (4, 4), (4, 4), 2, 11),
    G("nearest-4-4-ragged", 1, 253, 17, 1.5, 1.5, (4, 4), (4, 4), 2, 11),
    G("nearest-4-4-last-round", 1, 256, 8, 4.0, 4.0, (4, 4), (4, 4), 4, 29),         # 1024
    G("nearest-4-6-whole", 1, 256, 16, 1.5, 1.5, (4, 6), (4, 6), 2, 11),
    G("nearest-4-6-ragged", 1, 253, 17, 1.5, 1.5, (4, 6), (4, 6), 2, 11),
    G("nearest-4-6-last-round", 1, 256, 8, 6.0, 6.0, (4, 6), (4, 6), 6, 43),         # 1528
    G("nearest-8-8-whole", 1, 256, 32, 1.5, 1.5, (8, 8), (8, 8), 4, 23),
    G("nearest-8-8-ragged", 1, 253, 33, 1.5, 1.5, (8, 8), (8, 8), 4, 23),
    G("nearest-8-8-last-round", 1, 256, 16, 4.0, 4.0, (8, 8), (8, 8), 8, 61),        # 2048
    G("bilinear-4-4-whole", 2, 256, 16, 1.5, 1.5, (4, 4), (4, 4), 3, 13),
    G("bilinear-4-4-ragged", 2, 253, 17, 1.5, 1.5, (4, 4), (4, 4), 3, 13),
    G("bilinear-4-4-last-round", 2, 256, 8, 1.9, 1.9, (4, 4), (4, 4), 4, 15),        # 915
    G("bilinear-4-6-whole", 2, 256, 16, 1.5, 1.5, (4, 6), (4, 6), 3, 13),
    G("bilinear-4-6-ragged", 2, 253, 17, 1.5, 1.5, (4, 6), (4, 6), 3, 13),
    G("bilinear-4-6-last-round", 2, 256, 8, 3.0, 3.0, (4, 6), (4, 6), 6, 23),        # 1536
    G("bilinear-8-8-whole", 2, 256, 32, 1.5, 1.5, (8, 8), (8, 8), 5, 25),
    G("bilinear-8-8-ragged", 2, 253, 33, 1.5, 1.5, (8, 8), (8, 8), 5, 25),
    G("bilinear-8-8-last-round", 2, 256, 16, 1.95, 1.95, (8, 8), (8, 8), 8, 31),     # 1953
    G("bilinear-8-12-whole", 2, 256, 32, 1.5, 1.5, (8, 12), (8, 12), 5, 25),
    G("bilinear-8-12-ragged", 2, 253, 33, 1.5, 1.5, (8, 12), (8, 12), 5, 25),
    G("bilinear-8-12-last-round", 2, 256, 16, 3.0, 3.0, (8, 12), (8, 12), 12, 47),   # 3072
    G("bicubic-2-3-whole", 4, 64, 32, 1.5, 1.5, (2, 3), (2, 3), 2, 27),
    G("bicubic-2-3-ragged", 4, 61, 33, 1.5, 1.5, (2, 3), (2, 3), 2, 27),
    G("bicubic-2-3-last-round", 4, 64, 16, 2.2, 2.2, (2, 3), (2, 3), 3, 37),         # 703
    G("bicubic-2-4-whole", 4, 64, 32, 1.5, 1.5, (2, 4), (2, 4), 2, 27),
    G("bicubic-2-4-ragged", 4, 61, 33, 1.5, 1.5, (2, 4), (2, 4), 2, 27),
    G("bicubic-2-4-last-round", 4, 64, 16, 2.5, 2.5, (2, 4), (2, 4), 4, 42),         # 882
    G("bicubic-4-6-whole", 4, 64, 64, 1.5, 1.5, (4, 6), (4, 6), 3, 51),
    G("bicubic-4-6-ragged", 4, 61, 65, 1.5, 1.5, (4, 6), (4, 6), 3, 51),
    G("bicubic-4-6-last-round", 4, 64, 32, 2.3, 2.3, (4, 6), (4, 6), 6, 75),         # 1500
    G("bicubic-4-8-whole", 4, 64, 64, 1.5, 1.5, (4, 8), (4, 8), 3, 51),
    G("bicubic-4-8-ragged", 4, 61, 65, 1.5, 1.5, (4, 8), (4, 8), 3, 51),
    G("bicubic-4-8-last-round", 4, 64, 32, 2.75, 2.75, (4, 8), (4, 8), 8, 89),       # 2047
    # -- 2-byte elements move 16-byte pieces of an image in which every segment is padded to an even number of chunks, in
    #    kmax / 2 + 1 rounds of 256: 2 x 1 whole tiles whose segments hold an odd number of chunks and fill the shape so far that
    #    the padded image reaches the last of those rounds (source size, chunks and padded pieces per tile in the comment)
    G("nearest-4-4-wide-last-round", 1, 256, 8, 10.7, 0.3, (4, 4), (4, 4), 4, 3),        # 2748 x 10, 1023 1023, 513 513
    G("nearest-4-6-wide-last-round", 1, 256, 8, 6.85, 0.85, (4, 6), (4, 6), 6, 7),       # 1764 x 14, 1526 1533, 763 770
    G("nearest-8-8-wide-last-round", 1, 256, 16, 4.9, 0.8, (8, 8), (8, 8), 8, 13),       # 1264 x 20, 2041 2028, 1027 1014
    G("bilinear-4-4-wide-last-round", 2, 256, 8, 2.25, 1.65, (4, 4), (4, 4), 4, 14),     # 584 x 21, 1022 1022, 518 518
    G("bilinear-4-6-wide-last-round", 2, 256, 8, 3.4, 1.65, (4, 6), (4, 6), 6, 14),      # 880 x 21, 1526 1526, 770 770
    G("bilinear-8-8-wide-last-round", 2, 256, 16, 2.25, 1.7, (8, 8), (8, 8), 8, 28),     # 584 x 35, 2044 2044, 1036 1036
    G("bilinear-8-12-wide-last-round", 2, 256, 16, 3.05, 1.9, (8, 12), (8, 12), 12, 31), # 788 x 38, 3038 3069, 1519 1550
    G("bicubic-2-3-wide-last-round", 4, 64, 16, 0.85, 4.0, (2, 3), (2, 3), 3, 64),       # 64 x 72, 512 576, 256 320
    G("bicubic-2-4-wide-last-round", 4, 64, 16, 1.95, 3.7, (2, 4), (2, 4), 4, 60),       # 132 x 67, 960 1020, 480 540
    G("bicubic-4-6-wide-last-round", 4, 64, 32, 1.35, 3.65, (4, 6), (4, 6), 6, 117),     # 96 x 124, 1404 1521, 702 819
    G("bicubic-4-8-wide-last-round", 4, 64, 32, 1.95, 3.75, (4, 8), (4, 8), 8, 120),     # 132 x 128, 1920 2040, 960 1080
    # -- the row limit: a tile of 160 source rows is staged, one of 161 or more is not
    G("nearest-rows-22.7", 1, 256, 8, 0.5, 22.7, None, (4, 4), 1, 160),
    G("nearest-rows-22.9", 1, 256, 8, 0.5, 22.9, None, None, None, 161),
    G("bilinear-rows-22.6", 2, 256, 8, 0.5, 22.6, None, (4, 4), 2, 160),
    G("bilinear-rows-22.7", 2, 256, 8, 0.5, 22.7, None, None, None, 161),
    G("bicubic-rows-10.4", 4, 64, 16, 0.5, 10.4, None, (2, 3), 2, 160),
    G("bicubic-rows-10.5", 4, 64, 16, 0.5, 10.5, None, None, None, 162),
    # -- nearest with source rows that no cell reads; narrow, tall footprints whose segments have an odd number of chunks;
    #    4 x 3 tiles (more tiles than XCDs)
    G("nearest-skipped-rows", 1, 256, 16, 1.3, 2.5, None, (4, 4), 2, 18),
    G("bilinear-odd-segments", 2, 256, 16, 0.5, 9.0, None, (4, 4), 2, 65),
    G("bicubic-odd-segments", 4, 64, 32, 0.5, 9.0, None, (2, 3), 2, 139),
    G("nearest-12-tiles", 1, 512, 24, 1.5, 1.5, None, (4, 4), 2, 11),
    G("bilinear-12-tiles", 2, 512, 24, 1.5, 1.5, None, (4, 4), 3, 13),
    G("bicubic-12-tiles", 4, 128, 48, 1.5, 1.5, None, (2, 3), 2, 27),
]
# -- the DMA rounds before the last one: 2 x 1 whole tiles again, the shape forced, (ratio, rows of a tile) for rounds 1 .. kmax - 1
EARLIER_ROUNDS = {
    (1, 4, 4): ((0.7, 6), (1.45, 11), (2.5, 18)),
    (1, 4, 6): ((0.7, 6), (1.45, 11), (2.5, 18), (3.5, 25), (4.5, 32)),
    (1, 8, 8): ((0.5, 8), (0.85, 13), (1.2, 19), (1.7, 26), (2.25, 34), (2.75, 42), (3.25, 49)),
    (2, 4, 4): ((0.6, 6), (1.15, 10), (1.5, 13)),
    (2, 4, 6): ((0.6, 6), (1.15, 10), (1.5, 13), (1.85, 15), (2.2, 18)),
    (2, 8, 8): ((0.4, 8), (0.8, 14), (1.05, 18), (1.25, 21), (1.45, 24), (1.65, 27), (1.8, 29)),
    (2, 8, 12): ((0.4, 8), (0.8, 14), (1.05, 18), (1.25, 21), (1.45, 24), (1.65, 27), (1.8, 29), (1.9, 31), (2.1, 34), (2.35, 37), (2.6, 41)),
    (4, 2, 3): ((0.8, 16), (1.55, 27)),
    (4, 2, 4): ((0.8, 16), (1.55, 27), (2.1, 36)),
    (4, 4, 6): ((0.55, 21), (1.05, 37), (1.45, 49), (1.75, 58), (2.0, 66)),
    (4, 4, 8): ((0.55, 21), (1.05, 37), (1.45, 49), (1.75, 58), (2.0, 66), (2.25, 74), (2.45, 80)),
}
for (_st, _per, _k), _ratios in EARLIER_ROUNDS.items():
    for _i, (_r, _rows) in enumerate(_ratios):
        GEOMS.append(G("%s-%d-%d-round-%d" % ({1: "nearest", 2: "bilinear", 4: "bicubic"}[_st], _per, _k, _i + 1), _st, 2 * LADDER[_st][0],
                       tile_height(_st, _per), _r, _r, (_per, _k), (_per, _k), _i + 1, _rows))
BY_NAME = {g.name: g for g in GEOMS}
assert len(BY_NAME) == len(GEOMS)


def names(part, stencil=None):
    return [g.name for g in GEOMS if part in g.name and stencil in (None, g.stencil)]


def positions(g):
    inX, inY = -(-(int(g.outX * g.rx) + 8) // 4) * 4, int(g.outY * g.ry) + 8
    return affine(g.outX, g.outY, g.rx, 1.3, 0)[0], affine(g.outX, g.outY, g.ry, 0, 1.6)[1], inX, inY


def footprint(g):
    """(shape, chunks per tile, rows of the tallest tile) of a geometry of the table, by the fit rule on the CPU"""
    px, py, inX, inY = positions(g)
    shape, counts = first_form_shape(g.stencil, px, py, inX, inY, g.outX, g.outY, g.force)
    per = (shape or g.force or LADDER[g.stencil][1][-1])[0]
    return shape, counts, row_span(g.stencil, py, g.outX, g.outY, tile_height(g.stencil, per))


# ---- the tests' own inputs, on the CPU
@pytest.mark.parametrize("name", list(BY_NAME))
def test_geometry_lands_in_its_shape_round_and_rows(name):
    g = BY_NAME[name]
    shape, counts, rows = footprint(g)
    rounds = None if None in counts else -(-max(counts) // 256)
    print(name, shape, counts, rows)
    assert (shape, rounds, rows) == (g.shape, g.rounds, g.rows)
    if shape is None:  # why nothing fits: too many rows, or more chunks than the last shape tried holds
        kmax = (g.force or LADDER[g.stencil][1][-1])[1]
        assert rows > MAX_ROWS if rounds is None else (rounds > kmax and rows <= MAX_ROWS)
    else:
        assert rounds <= shape[1] and rows <= MAX_ROWS and (g.force is None or shape == g.force)


def test_table_reaches_every_shape_and_every_dma_round_of_it():
    """All 11 shapes are chosen by a geometry that forces nothing and by forced ones with 2 x 2 whole tiles, and each has forced
    geometries of 2 x 1 whole tiles whose fullest tile lies in round 1, 2, ... kmax of 256 chunks.  For float and 1-byte elements
    (a chunk is one DMA piece) those are the kernel's rounds: in the last one every round of its unrolled DMA loop carries data, in
    the earlier ones the later rounds fetch nothing.  For 2-byte elements see test_wide_case_reaches_the_last_round_of_padded_pieces."""
    for st, per, k in SHAPES:
        mine = [g for g in GEOMS if g.stencil == st and g.shape == (per, k)]
        assert any(g.force is None for g in mine), (st, per, k)
        whole = [g for g in mine if g.force and g.outX % LADDER[st][0] == 0 and g.outY % tile_height(st, per) == 0]
        assert any(g.outY == 2 * tile_height(st, per) for g in whole), (st, per, k)
        assert {g.rounds for g in whole if g.outY == tile_height(st, per)} == set(range(1, k + 1)), (st, per, k)
    # the shapes that an unforced geometry fills to the last chunk
    full = {(g.stencil, g.shape) for g in GEOMS if g.shape and g.force is None and max(footprint(g)[1]) == g.shape[1] * 256}
    assert full == {(1, (4, 4)), (2, (4, 6)), (2, (8, 8)), (2, (8, 12)), (4, (4, 8))}


def padded_pieces(g):
    """16-byte pieces of every tile's image of 2-byte elements: each segment padded to an even number of chunks, two chunks a piece"""
    px, py, inX, inY = positions(g)
    tw, th = LADDER[g.stencil][0], tile_height(g.stencil, g.shape[0])
    return [sum((n + 1) // 2 for n in tile_segments(g.stencil, px, py, inX, g.outX, g.outY, x0, y0, tw, th))
            for y0 in range(0, g.outY, th) for x0 in range(0, g.outX, tw)]


@pytest.mark.parametrize("stencil,per,kmax", SHAPES)
def test_wide_case_reaches_the_last_round_of_padded_pieces(stencil, per, kmax):
    """short and unsigned short run kmax / 2 + 1 DMA rounds of 256 pieces: the fullest tile of the shape's wide case lies in the
    last one, which only chunks + segments of an odd number of chunks > kmax * 256 reaches; the last-round cases of whole chunks
    end one round earlier (nearest {4,4} at 1024 chunks in segments of 128: exactly 512 pieces)"""
    (name,) = names("-%d-%d-wide-last-round" % (per, kmax), stencil)
    g = BY_NAME[name]
    pieces, counts = padded_pieces(g), footprint(g)[1]
    print(name, counts, pieces)
    assert g.force == g.shape == (per, kmax) and max(counts) <= kmax * 256
    assert (kmax // 2) * 256 < max(pieces) <= (kmax // 2 + 1) * 256, (counts, pieces)
    plain = BY_NAME[name.replace("-wide", "")]
    assert max(padded_pieces(plain)) <= (kmax // 2 + 1) * 256


@pytest.mark.parametrize("name", names("odd-segments"))
def test_odd_segment_case_has_mostly_odd_segments(name):
    """of the row segments that hold chunks, more than half hold an odd number in every tile (2-byte elements pad those to whole
    16-byte pieces); the rows between are segments without chunks, which the piece search must skip"""
    g = BY_NAME[name]
    px, py, inX, inY = positions(g)
    tw, th = LADDER[g.stencil][0], tile_height(g.stencil, g.shape[0])
    counts = footprint(g)[1]
    tiles = [(x0, y0) for y0 in range(0, g.outY, th) for x0 in range(0, g.outX, tw)]
    for (x0, y0), total in zip(tiles, counts):
        seg = tile_segments(g.stencil, px, py, inX, g.outX, g.outY, x0, y0, tw, th)
        assert sum(seg) == total and 2 * sum(n % 2 for n in seg) > len(seg) and len(seg) < g.rows, (x0, y0, seg)


def test_skipped_rows_case_skips_rows():
    g = BY_NAME["nearest-skipped-rows"]
    px, py, inX, inY = positions(g)
    seg = tile_segments(1, px, py, inX, g.outX, g.outY, 0, 0, 128, 8)
    assert len(seg) == 8 and g.rows == 18  # 8 of the 18 rows a tile spans hold chunks


# ---- on the GPU
GUARD = 64  # bytes before and after every output (allocations are aligned to more, so the output stays 4-byte aligned)


def guarded(nbytes, launch):
    """runs launch(pointer to nbytes of output) between two guard zones and returns the output's bytes"""
    import torch
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    launch(buf.data_ptr() + GUARD)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + nbytes:] == 0xA5).all(), "guard bytes overwritten"
    return host[GUARD:GUARD + nbytes].copy()


class Case:
    """One geometry of the table with its fields and the oracle's answers, computed once and shared by the variants."""

    def __init__(self, name, nz):
        self.g, self.nz = BY_NAME[name], nz
        self.px, self.py, self.inX, self.inY = positions(self.g)
        self.dims = (self.inX, self.inY, self.g.outX, self.g.outY)
        self.method = METHOD[self.g.stencil]
        self.counts = footprint(self.g)[1]
        self.f = cases.field(nz, self.inY, self.inX, seed=len(name) + nz, extremes=False)
        self.want = oracle.interpolate_values(self.method, self.px, self.py, self.f, *self.dims)
        self.stored = {}

    def typed(self, dt, fill=True):
        """field of a stored type, fill value (one that occurs in the data, or NaN: none), the oracle's three steps, cells to compare"""
        if (dt, fill) not in self.stored:
            info = np.iinfo(dt)
            rng = np.random.default_rng(self.inX + 8 * np.dtype(dt).itemsize + int(info.min < 0))
            f = rng.integers(info.min, int(info.max) + 1, (self.nz, self.inY, self.inX)).astype(dt)
            bad = float(info.min + 3) if fill else float("nan")
            if fill:
                f.reshape(-1)[rng.random(f.size) < 0.03] = dt(bad)
            fl = oracle.interpolate_values(self.method, self.px, self.py, oracle.data2interpolation_array(f, bad), *self.dims)
            # without a fill value an undefined result becomes (T)NaN, which C leaves undefined: those cells are not compared
            self.stored[(dt, fill)] = (f, bad, oracle.interpolation_array2data(fl, oracle.cdm_type_of(dt), bad),
                                       np.ones(fl.shape, bool) if fill else ~np.isnan(fl))
        return self.stored[(dt, fill)]

    def plan(self, fa, monkeypatch, env=None):
        """the plan under the switches (None: the product build, which reads none), held to the table and the CPU footprint"""
        g = self.g
        if env is not None:
            env = dict(FIRST_ONLY, **env)
            if g.force:
                env.update(STAGE_PER=str(g.force[0]), STAGE_K=str(g.force[1]))
            for k, v in env.items():
                monkeypatch.setenv("FIMEX_AMD_" + k, v)
        else:
            assert g.force is None and g.stencil == 4  # nearest and bilinear floats would run the second form
        plan = fa.RegridPlan(self.method, self.px, self.py, *self.dims, bicubic=fa.BICUBIC_REFERENCE if g.stencil == 4 else None)
        info = plan.info()
        if g.shape:
            tile = (LADDER[g.stencil][0], tile_height(g.stencil, g.shape[0]))
            assert (info["tileW"], info["tileH"]) == tile and info["stagedCells"] == 4 * sum(self.counts), (g.name, info, self.counts)
        else:
            assert env is not None and info["stagedCells"] == 0, (g.name, info)
        return plan

    def check_float(self, fa, plan, what, nz=None, gather=False):
        import torch
        nz = nz or self.nz
        d_in = torch.from_numpy(np.ascontiguousarray(self.f[:nz])).cuda()
        apply = plan.apply_gather_device if gather else plan.apply_device
        raw = guarded(nz * self.g.outY * self.g.outX * 4,
                      lambda out: apply(d_in.data_ptr(), nz, out, torch.cuda.current_stream().cuda_stream))
        got = raw.view(np.float32).reshape(nz, self.g.outY, self.g.outX)
        assert cases.same(got, self.want[:nz]), (self.g.name, what, nz, cases.describe_mismatch(got, self.want[:nz]))

    def check_typed(self, fa, plan, dt, what, fill=True, nz=None):
        import torch
        nz = nz or self.nz
        f, bad, want, defined = self.typed(dt, fill)
        want, defined = want[:nz], defined[:nz]
        d_in = torch.from_numpy(np.ascontiguousarray(f[:nz]).view(np.uint8)).cuda()
        raw = guarded(want.nbytes, lambda out: fa.regrid_apply_typed_device(plan, d_in.data_ptr(), oracle.cdm_type_of(dt), nz, bad, out))
        got = raw.view(dt).reshape(want.shape)
        assert defined.any() and np.array_equal(got[defined], want[defined]), \
            (self.g.name, what, np.dtype(dt).name, fill, nz, int((got != want)[defined].sum()))

    def check_all(self, fa, plan, what, types=TYPES):
        self.check_float(fa, plan, what)
        for dt in types:
            self.check_typed(fa, plan, dt, what)


_cases = {}


def case(name, nz=5):
    if (name, nz) not in _cases:
        _cases[(name, nz)] = Case(name, nz)
    return _cases[(name, nz)]


# ---- shapes the product build picks by itself: bicubic on one tile row, one geometry per shape
@gpu
@pytest.mark.parametrize("name", ["bicubic-row-2.2", "bicubic-row-2.5", "bicubic-row-2.8", "bicubic-row-3.4"])
def test_product_build_reaches_every_bicubic_shape(fa, name):
    c = case(name)
    plan = c.plan(fa, None)
    c.check_all(fa, plan, "product")
    for dt in (np.uint8, np.int16):
        c.check_typed(fa, plan, dt, "product, no fill value", fill=False)
    c.check_float(fa, plan, "product, gather kernel", gather=True)


# ---- every shape, forced, with whole tiles
@gpu
@pytest.mark.parametrize("stencil,per,kmax", SHAPES)
def test_every_shape_forced(fa, tuning_build, monkeypatch, stencil, per, kmax):
    """2 x 2 whole tiles, the ragged copy, the last round of chunks and the last round of padded 16-byte pieces: float slices and
    the four stored types on each"""
    mine = [n for n in names("-%d-%d-" % (per, kmax), stencil) if n.endswith(("-whole", "-ragged", "-last-round"))]
    assert len(mine) == 4 and sum(n.endswith("-wide-last-round") for n in mine) == 1
    for name in mine:
        c = case(name)
        plan = c.plan(fa, monkeypatch, {})
        assert plan.info()["tileH"] == per * 256 // plan.info()["tileW"]
        c.check_all(fa, plan, "forced")


@gpu
@pytest.mark.parametrize("stencil,per,kmax", SHAPES)
def test_every_dma_round_of_every_shape(fa, tuning_build, monkeypatch, stencil, per, kmax):
    """the fullest tile ends in round 1, 2, ... kmax - 1 of 256 chunks (the last round: test_every_shape_forced); float and a
    1-byte type, whose DMA rounds these are, and a 2-byte type, whose kmax / 2 + 1 rounds of padded pieces end earlier still"""
    mine = names("-%d-%d-round-" % (per, kmax), stencil)
    assert len(mine) == kmax - 1
    for name in mine:
        c = case(name)
        c.check_all(fa, c.plan(fa, monkeypatch, {}), "rounds", types=(np.uint8, np.int16))


@gpu
@pytest.mark.parametrize("name", names("-forced-"))
def test_rungs_pinned_on_the_ladder_geometries(fa, tuning_build, monkeypatch, name):
    """the rung before the chosen one leaves the plan without a staged form; the chosen one, pinned, builds the same plan.  Together
    with the tile height this tells rungs of one tile size apart, which plan.info() alone cannot."""
    c = case(name)
    plan = c.plan(fa, monkeypatch, {})
    if c.g.shape:
        free = case(name[:name.index("-forced-")]).plan(fa, monkeypatch, {"STAGE_PER": "0", "STAGE_K": "0"})
        assert free.info() == plan.info()
    c.check_float(fa, plan, "pinned rung")


# ---- boundaries of the footprint
@gpu
@pytest.mark.parametrize("name", [n for n in names("-row-") if "forced" not in n])
def test_ladder_exact_capacity_and_one_step_further(fa, tuning_build, monkeypatch, name):
    """the ladder by itself on one tile row: a fullest tile of exactly kmax * 256 chunks (and 2040 of 2048) keeps its shape; a
    little more source moves the plan to the next shape or, at the ladder's end, drops the form"""
    c = case(name)
    c.check_all(fa, c.plan(fa, monkeypatch, {}), "ladder", types=(np.uint8, np.int16))


@gpu
@pytest.mark.parametrize("name", names("-rows-"))
def test_row_limit(fa, tuning_build, monkeypatch, name):
    """160 source rows per tile are staged; from 161 on there is no first form and whatever serves instead is as right"""
    c = case(name)
    c.check_all(fa, c.plan(fa, monkeypatch, {}), "rows", types=(np.uint8, np.int16))


@gpu
def test_skipped_source_rows(fa, tuning_build, monkeypatch):
    """nearest at 2.5 source rows per target row: segments without chunks in the chunk and the piece search"""
    c = case("nearest-skipped-rows")
    c.check_all(fa, c.plan(fa, monkeypatch, {}), "skipped rows", types=(np.uint8, np.int16))


@gpu
@pytest.mark.parametrize("name", names("odd-segments"))
def test_odd_segments_on_two_byte_types(fa, tuning_build, monkeypatch, name):
    c = case(name)
    c.check_all(fa, c.plan(fa, monkeypatch, {}), "odd segments", types=(np.int16, np.uint16))


@gpu
@pytest.mark.parametrize("stencil,dt", [(1, np.uint8), (2, np.int16), (4, np.int8)])
def test_tiles_without_chunks_and_partial_tiles(fa, tuning_build, monkeypatch, stencil, dt):
    """The last tile row of the target lies below the source (tiles without chunks: every slice is written as undefined), and the
    map overshoots the source on the other three sides and below the second tile row, so that undefined and border cells sit
    inside staged tiles."""
    import torch
    tw, th = LADDER[stencil][0], tile_height(stencil, LADDER[stencil][1][0][0])
    outX, outY, nz = 2 * tw - 3, 3 * th, 5
    px, py = affine(outX, outY, 1.3, -2.5, -1.7)
    inX, inY = int((outX - 1) * 1.3 - 2.5) // 4 * 4 - 4, int((2 * th - 1) * 1.3 - 1.7)
    py[2 * th * outX:] += inY + 5
    assert px.max() > inX + 2 and py.reshape(outY, outX)[:2 * th].max() > inY - 1 and py.reshape(outY, outX)[2 * th:].min() > inY + 4
    for k, v in FIRST_ONLY.items():
        monkeypatch.setenv("FIMEX_AMD_" + k, v)
    plan = fa.RegridPlan(METHOD[stencil], px, py, inX, inY, outX, outY, bicubic=fa.BICUBIC_REFERENCE if stencil == 4 else None)
    info = plan.info()
    assert (info["tileW"], info["tileH"]) == (tw, th) and info["stagedCells"] > 0 and info["undefinedCells"] > th * outX, info
    f = cases.field(nz, inY, inX, seed=stencil, extremes=False)
    want = oracle.interpolate_values(METHOD[stencil], px, py, f, inX, inY, outX, outY)
    assert np.isnan(want[:, 2 * th:]).all() and not np.isnan(want[:, :2 * th]).all()
    d_in = torch.from_numpy(f).cuda()
    got = guarded(want.size * 4, lambda out: plan.apply_device(d_in.data_ptr(), nz, out, torch.cuda.current_stream().cuda_stream))
    got = got.view(np.float32).reshape(want.shape)
    assert cases.same(got, want), cases.describe_mismatch(got, want)
    lim = np.iinfo(dt)
    rng = np.random.default_rng(stencil)
    t = rng.integers(lim.min, int(lim.max) + 1, (nz, inY, inX)).astype(dt)
    bad = float(lim.min + 3)
    t.reshape(-1)[rng.random(t.size) < 0.03] = dt(bad)
    code = oracle.cdm_type_of(dt)
    wantT = oracle.interpolation_array2data(
        oracle.interpolate_values(METHOD[stencil], px, py, oracle.data2interpolation_array(t, bad), inX, inY, outX, outY), code, bad)
    d_t = torch.from_numpy(t.view(np.uint8)).cuda()
    gotT = guarded(wantT.nbytes, lambda out: fa.regrid_apply_typed_device(plan, d_t.data_ptr(), code, nz, bad, out)).view(dt).reshape(wantT.shape)
    assert (wantT[:, 2 * th:] == dt(bad)).all() and np.array_equal(gotT, wantT), int((gotT != wantT).sum())


# ---- the slice loop and the launch layout, one shape per stencil
@gpu
@pytest.mark.parametrize("nz", [51, 101])
def test_product_build_two_and_three_z_chunks(fa, nz):
    """STAGE_ZPB is 50: 51 slices are chunks of 50 and 1, 101 slices chunks of 50, 50 and 1"""
    c = case("bicubic-row-2.2", nz)
    plan = c.plan(fa, None)
    c.check_float(fa, plan, "z chunks")
    c.check_typed(fa, plan, np.int16, "z chunks")


LOOP_CASES = [("nearest-8-8-whole", np.uint8), ("bilinear-4-6-whole", np.int16), ("bicubic-2-4-whole", np.uint16)]


@gpu
@pytest.mark.parametrize("name,dt", LOOP_CASES)
def test_z_chunks_shorter_than_equal_to_and_longer_than_the_ring(fa, tuning_build, monkeypatch, name, dt):
    """7 slices in chunks of 1, 2 and 3 (the last ragged), and batches of 1, 2 and 3 slices in one chunk, at ring depth 2"""
    c = case(name, 7)
    plan = c.plan(fa, monkeypatch, {})
    for nz in (1, 2, 3):
        c.check_float(fa, plan, "short batch", nz=nz)
        c.check_typed(fa, plan, dt, "short batch", nz=nz)
    for zpb in ("1", "2", "3"):
        monkeypatch.setenv("FIMEX_AMD_STAGE_ZPB", zpb)
        c.check_float(fa, plan, "STAGE_ZPB " + zpb)
        c.check_typed(fa, plan, dt, "STAGE_ZPB " + zpb)


@gpu
@pytest.mark.parametrize("name", ["nearest-4-4-whole", "bilinear-8-12-last-round", "bicubic-4-8-last-round"])
def test_ring_depths(fa, tuning_build, monkeypatch, name):
    """STAGE_NBUF 1, 3, 4 and 6: {4,4} admits all of them, {4,8} all but 6, {8,12} only 1 and 3 (4 and 6 run depth 2); with 7 slices
    in one chunk and in chunks of 2.  TYPED_NBUF 3 on a 2- and a 1-byte type."""
    c = case(name, 7)
    plan = c.plan(fa, monkeypatch, {})
    for nbuf in ("1", "3", "4", "6"):
        monkeypatch.setenv("FIMEX_AMD_STAGE_NBUF", nbuf)
        c.check_float(fa, plan, "STAGE_NBUF " + nbuf)
        c.check_float(fa, plan, "STAGE_NBUF " + nbuf, nz=2)
        monkeypatch.setenv("FIMEX_AMD_STAGE_ZPB", "2")
        c.check_float(fa, plan, "STAGE_NBUF " + nbuf + ", STAGE_ZPB 2")
        monkeypatch.delenv("FIMEX_AMD_STAGE_ZPB")
    monkeypatch.setenv("FIMEX_AMD_TYPED_NBUF", "3")
    for dt in (np.int16, np.uint8):
        c.check_typed(fa, plan, dt, "TYPED_NBUF 3")
        c.check_typed(fa, plan, dt, "TYPED_NBUF 3", nz=2)


@gpu
@pytest.mark.parametrize("name,dt", [(n, dt) for st, dt in ((1, np.int16), (2, np.uint8), (4, np.int16))
                                     for n in (names("12-tiles", st)[0], names("-whole", st)[0])])
def test_launch_order_and_xcd_map(fa, tuning_build, monkeypatch, name, dt):
    """The z-chunk-major grid and the flat tile-major one (STAGE_ORDER 1), each with the tile -> XCD maps 0 .. 3 and the order's
    own default, on 12 tiles and on 4 (8 XCDs); 7 slices in chunks of 3, 3 and 1."""
    c = case(name, 7)
    plan = c.plan(fa, monkeypatch, {"STAGE_ZPB": "3"})
    for order in ("0", "1"):
        monkeypatch.setenv("FIMEX_AMD_STAGE_ORDER", order)
        for xcd in (None, "0", "1", "2", "3"):
            if xcd is None:
                monkeypatch.delenv("FIMEX_AMD_XCD", raising=False)
            else:
                monkeypatch.setenv("FIMEX_AMD_XCD", xcd)
            c.check_float(fa, plan, ("STAGE_ORDER", order, "XCD", xcd))
            c.check_typed(fa, plan, dt, ("STAGE_ORDER", order, "XCD", xcd))
