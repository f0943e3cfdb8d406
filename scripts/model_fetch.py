#!/usr/bin/env python3
"""What the staged bilinear launch stages and fetches, modelled on the CPU from the positions alone.

  model_fetch.py [--variant default|one_percent] [--tile-w 512] [--tile-h 8] [--nz 200] [--json]

Plain numpy over workloads.BilinearRotatedPole, no GPU.  The tiles are cut by the library's own rules (refine_bands of
fimex_amd/csrc/staged_layout.hpp through tests/staged_layout_host.py, the tile scan replaced by the footprint below); the cohorts
are chunk_xcd_order's (tests/staged_layout_chunk_xcd_host.py).  Per tile and source row one span: the smallest and the largest
column any cell of the tile reads.  Aligned to 16 bytes the spans are what a workgroup stages ("staged cells", plan.info()'s
stagedCells: 12 082 148 per slice for the default variant and 9 673 512 for one_percent in BENCH_r03.json; the model gives both
figures exactly, tests/test_model_fetch.py).  Aligned to 128 bytes they are the lines a workgroup asks for.

Printed, per slice in source cells (lines x 32) and per launch of --nz slices in GB:
  lines summed over tiles       what crosses the fabric if no line is shared between workgroups;
  distinct lines                the floor: every line once;
  duplicates in x / in y        between the tiles of one band / between bands;
  per launch order              lines summed over the groups of tiles that share an L2 while they run, each group's lines counted
                                once: the present order (a tile's z chunks on one XCD, neighbouring bands on other XCDs: no
                                sharing between tiles) and the chunk-per-XCD order with cohorts of 8 x 4, 16 x 2 and 32 x 1.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import workloads  # noqa: E402

LINE_CELLS, CHUNK_CELLS, MAX_ROWS = 32, 4, 160  # 128-byte lines, 16-byte chunks, kMaxRows of a tile
COHORTS = [(8, 4), (16, 2), (32, 1)]


def positions(wl):
    """fractional source indices of every target cell (the source axes are regular: 0.01 degrees times the scale)"""
    lon, lat = wl.target_lonlat()
    px = (np.degrees(lon) - wl.src_lon[0]) / (wl.src_lon[1] - wl.src_lon[0])
    py = (np.degrees(lat) - wl.src_lat[0]) / (wl.src_lat[1] - wl.src_lat[0])
    return px.reshape(wl.outY, wl.outX), py.reshape(wl.outY, wl.outX)


class Footprint:
    """the 2 x 2 stencils of a bilinear plan: per cell the columns xa .. xb of rows ya .. yb, clamped to the source; cells
    outside it (more than half a cell beyond the rim) read nothing"""

    def __init__(self, wl):
        px, py = positions(wl)
        self.inX, self.inY = wl.inX, wl.inY
        self.defined = (px >= -0.5) & (px < wl.inX - 0.5) & (py >= -0.5) & (py < wl.inY - 0.5)
        fx, fy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
        self.xa, self.xb = np.clip(fx, 0, wl.inX - 1), np.clip(fx + 1, 0, wl.inX - 1)
        self.ya, self.yb = np.clip(fy, 0, wl.inY - 1), np.clip(fy + 1, 0, wl.inY - 1)

    def spans(self, x0, y0, w, h):
        """(row, lo, hi) of every source row the tile reads; None: more rows than a tile may span"""
        t = (slice(y0, y0 + h), slice(x0, x0 + w))
        d = self.defined[t]
        if not d.any():
            return np.zeros((0, 3), np.int64)
        ya, yb, xa, xb = self.ya[t][d], self.yb[t][d], self.xa[t][d], self.xb[t][d]
        r0, r1 = int(ya.min()), int(yb.max())
        if r1 - r0 >= MAX_ROWS:
            return None
        lo = np.full(r1 - r0 + 1, self.inX, np.int64)
        hi = np.full(r1 - r0 + 1, -1, np.int64)
        for rows in (ya, yb):
            np.minimum.at(lo, rows - r0, xa)
            np.maximum.at(hi, rows - r0, xb)
        used = hi >= 0
        return np.stack([np.arange(r0, r1 + 1)[used], lo[used], hi[used]], axis=1)

    def chunks(self, spans):
        """16-byte chunks of the spans (a row segment starts on a 16-byte boundary of the slice)"""
        first = spans[:, 0] * self.inX + spans[:, 1]
        return int(((first % CHUNK_CELLS + spans[:, 2] - spans[:, 1]) // CHUNK_CELLS + 1).sum())

    def lines(self, spans):
        """ids of the 128-byte lines of the slice that the staged chunks of the spans touch"""
        first = (spans[:, 0] * self.inX + spans[:, 1]) // CHUNK_CELLS * CHUNK_CELLS
        last = (spans[:, 0] * self.inX + spans[:, 2]) // CHUNK_CELLS * CHUNK_CELLS + CHUNK_CELLS - 1
        a, b = first // LINE_CELLS, last // LINE_CELLS
        n = b - a + 1
        return np.repeat(a, n) + (np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n))


def cut(fp, wl, tileW, tileH, cap):
    """the final tiles of the plan as (x0, y0, w, band), gather tiles left out (they stage nothing)"""
    import staged_layout_host as slh
    lib = slh.load()

    def scan(tiles):
        out = []
        for t in tiles:
            s = fp.spans(t.x0, t.y0, t.w, tileH)
            c = None if s is None else fp.chunks(s)
            out.append(slh.TOO_LARGE if c is None or c > cap else c)
        return out
    passes, kept, _ = slh.cut_tiles(lib, wl.outX, wl.outY, tileW, tileH, scan)
    assert kept, "the plan gives the staged form up"
    return [t for t in passes[-1] if not t.gather]


def distinct(sets):
    return int(len(np.unique(np.concatenate(sets)))) if sets else 0


def model(variant, tileW, tileH, nz, scale=1):
    import staged_layout_host as slh
    import staged_layout_chunk_xcd_host as cx
    wl = workloads.BilinearRotatedPole(scale=scale, variant=variant)
    fp = Footprint(wl)
    nt = tileW * tileH // 4  # four outputs per lane
    lds = {256: 52, 512: 79, 1024: 159}[nt] * 1024
    cap = slh.load().sl_tile_chunk_cap(lds, 2, 5 if nt == 1024 else 6, nt, CHUNK_CELLS)
    tiles = cut(fp, wl, tileW, tileH, cap)
    spans = [fp.spans(t.x0, t.y0, t.w, tileH) for t in tiles]
    lines = [fp.lines(s) for s in spans]
    band = np.array([t.band for t in tiles])
    staged = CHUNK_CELLS * sum(fp.chunks(s) for s in spans)
    summed = sum(len(l) for l in lines)
    per_band = sum(distinct([lines[i] for i in np.flatnonzero(band == b)]) for b in np.unique(band))
    overall = distinct(lines)
    gb = lambda n_lines: n_lines * LINE_CELLS * 4 * nz / 1e9
    out = {"variant": variant, "tile": [tileW, tileH], "nz": nz, "tiles": len(tiles), "chunk_cap": int(cap),
           "staged_cells_per_slice": staged,
           "lines_summed_over_tiles": {"cells_per_slice": summed * LINE_CELLS, "GB_per_launch": gb(summed)},
           "distinct_lines": {"cells_per_slice": overall * LINE_CELLS, "GB_per_launch": gb(overall)},
           "duplicates_x": {"cells_per_slice": (summed - per_band) * LINE_CELLS, "GB_per_launch": gb(summed - per_band)},
           "duplicates_y": {"cells_per_slice": (per_band - overall) * LINE_CELLS, "GB_per_launch": gb(per_band - overall)},
           "orders": {"tile_major (no sharing)": {"cells_per_slice": summed * LINE_CELLS, "GB_per_launch": gb(summed)}}}
    x0, w = np.array([t.x0 for t in tiles]), np.array([t.w for t in tiles])
    for by, bx in COHORTS:
        order, cohort = cx.order_of(cx.load(), x0, w, band, tileW, by, bx)
        n = sum(distinct([lines[i] for i in order[cohort == c]]) for c in range(int(cohort[-1]) + 1))
        out["orders"]["chunk_per_xcd %dx%d" % (by, bx)] = {"cohorts": int(cohort[-1]) + 1, "cells_per_slice": n * LINE_CELLS, "GB_per_launch": gb(n)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--variant", default="default", choices=["default", "one_percent"])
    ap.add_argument("--tile-w", type=int, default=512)
    ap.add_argument("--tile-h", type=int, default=8)
    ap.add_argument("--nz", type=int, default=200)
    ap.add_argument("--scale", type=int, default=1, help="shrinks every axis of the workload (tests)")
    ap.add_argument("--json", action="store_true", help="one JSON line instead of the table")
    a = ap.parse_args()
    m = model(a.variant, a.tile_w, a.tile_h, a.nz, a.scale)
    if a.json:
        print(json.dumps(m))
        return
    print("%s, %d x %d tiles (%d of them, at most %d chunks each), %d slices" % (m["variant"], a.tile_w, a.tile_h, m["tiles"], m["chunk_cap"], a.nz))
    print("%-34s %14s %10s" % ("", "cells / slice", "GB"))
    print("%-34s %14d %10.2f" % ("staged cells", m["staged_cells_per_slice"], m["staged_cells_per_slice"] * 4 * a.nz / 1e9))
    for k in ("lines_summed_over_tiles", "distinct_lines", "duplicates_x", "duplicates_y"):
        print("%-34s %14d %10.2f" % (k.replace("_", " "), m[k]["cells_per_slice"], m[k]["GB_per_launch"]))
    for k, v in m["orders"].items():
        print("%-34s %14d %10.2f" % ("fetched, " + k, v["cells_per_slice"], v["GB_per_launch"]))


if __name__ == "__main__":
    main()
