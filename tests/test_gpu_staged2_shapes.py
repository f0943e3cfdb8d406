"""The second staged form (staged2_ring.hpp and the kernels on it) on the paths that only FIMEX_AMD_<NAME> switches reach:
every number of DMA rounds per slice, ring depth 3, z chunks shorter than the ring, the chunk-major launch order, every
thread count, and on stored types single stores, depth 3, a tile row outside the source and a gather tile.

Positions are affine maps (px = x * r + ox, py = y * r + oy), so that a tile's footprint can be computed; targets are a few
tiles.  Everything is compared bit for bit with the oracle, except bicubic in float arithmetic: that one meets the tolerance of
test_bicubic_fast_arithmetic_within_the_stated_tolerance (1e-5 of the stencil's magnitude, same NaN positions) and its variants
are bit-equal among themselves.  Two tests hold the plans themselves to the CPU: the tile cutting (staged_layout.hpp, driven here with
a numpy footprint) against the plan the library builds, and the first staged form's footprint on a uniform grid.  What
test_stored_types_second_staged_form_edges covers (unaligned output, no fill value, fill
values at the ends of the range) is not repeated here.
"""
import numpy as np
import pytest

import cases
import oracle

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


def affine(outX, outY, r, ox, oy):
    y, x = np.meshgrid(np.arange(outY, dtype=np.float64), np.arange(outX, dtype=np.float64), indexing="ij")
    return (x * r + ox).ravel(), (y * r + oy).ravel()


MAX_ROWS = 160  # kMaxRows: source rows one tile may span


def tile_list_chunks(stencil, px, py, inX, inY, outX, outY, tiles, cpc=4):
    """16-byte chunks of each tile (x0, y0, w, h) as the tile footprint (TileFootprint, staged_common.hpp) counts them where all
    cells lie inside the source: per source row the smallest and largest column any cell of the tile needs, the segment's start
    aligned down to cpc cells of the slice.  (A last chunk past the end of the slice is pulled back, which does not change the
    count.)  None: the tile spans more than MAX_ROWS source rows."""
    first = np.floor(px + 0.5) if stencil == 1 else np.floor(px), np.floor(py + 0.5) if stencil == 1 else np.floor(py)
    xa, ya = (v.astype(np.int64).reshape(outY, outX) - (1 if stencil == 4 else 0) for v in first)
    xb, yb = xa + stencil - 1, ya + stencil - 1
    assert xa.min() >= 0 and xb.max() < inX and ya.min() >= 0 and yb.max() < inY
    counts = []
    for x0, y0, w, h in tiles:
        t = (slice(y0, y0 + h), slice(x0, x0 + w))
        n = 0
        for row in range(ya[t].min(), yb[t].max() + 1):
            use = (ya[t] <= row) & (row <= yb[t])
            if use.any():
                lo, hi = xa[t][use].min(), xb[t][use].max()
                n += ((row * inX + lo) % cpc + hi - lo) // cpc + 1
        counts.append(int(n) if yb[t].max() - ya[t].min() < MAX_ROWS else None)
    return counts


def tile_chunks(stencil, px, py, inX, inY, outX, outY, tw, th, cpc=4):
    """the same on a uniform grid of tw x th tiles"""
    return tile_list_chunks(stencil, px, py, inX, inY, outX, outY,
                            [(x0, y0, tw, th) for y0 in range(0, outY, th) for x0 in range(0, outX, tw)], cpc)


def run_float(fa, plan, f, nz, outX, outY):
    import torch
    d_in = torch.from_numpy(np.ascontiguousarray(f[:nz])).cuda()
    out = torch.empty((nz, outY, outX), dtype=torch.float32, device="cuda")
    plan.apply_device(d_in.data_ptr(), nz, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# kind -> method, switches at plan creation and launch, bicubic arithmetic
KINDS = {"nearest": (oracle.NEAREST, {}, None), "bilinear": (oracle.BILINEAR, {}, None),
         "bicubic": (oracle.BICUBIC, {"STAGED2": "2"}, "BICUBIC_REFERENCE"), "bicubic_float": (oracle.BICUBIC, {}, "BICUBIC_FAST")}


class FloatCase:
    """One geometry and field; the oracle's answer is computed once and shared by the variants."""

    def __init__(self, kind, inX, inY, outX, outY, r, ox, oy, nz):
        self.kind, self.shape, self.nz = kind, (inX, inY, outX, outY), nz
        self.method, self.env, self.arith = KINDS[kind]
        self.px, self.py = affine(outX, outY, r, ox, oy)
        self.f = cases.field(nz, inY, inX, seed=outX + nz, extremes=False)
        self.want = oracle.interpolate_values(self.method, self.px, self.py, self.f, inX, inY, outX, outY)
        self.first = None

    def plan(self, fa, monkeypatch, env):
        for k, v in dict(self.env, STAGED_MIN_NZ="1", **env).items():
            monkeypatch.setenv("FIMEX_AMD_" + k, v)
        plan = fa.RegridPlan(self.method, self.px, self.py, *self.shape, bicubic=getattr(fa, self.arith) if self.arith else None)
        assert plan.info()["stagedCells"] > 0
        return plan

    def check(self, fa, plan, nz, what):
        inX, inY, outX, outY = self.shape
        got = run_float(fa, plan, self.f, nz, outX, outY)
        if self.kind != "bicubic_float":
            assert cases.same(got, self.want[:nz]), (what, cases.describe_mismatch(got, self.want[:nz]))
            return
        if self.first is None:  # the tolerance once, then the variants against the first one
            from numpy.lib.stride_tricks import sliding_window_view
            self.first = got
            assert np.array_equal(np.isnan(got), np.isnan(self.want[:nz]))
            x0, y0 = np.floor(self.px).astype(np.int64) - 1, np.floor(self.py).astype(np.int64) - 1
            ok = (x0 >= 0) & (x0 + 3 < inX) & (y0 >= 0) & (y0 + 3 < inY)
            for z in range(nz):
                mag = np.zeros(self.px.size, np.float32)
                mag[ok] = sliding_window_view(np.abs(np.nan_to_num(self.f[z])), (4, 4)).max(axis=(2, 3))[y0[ok], x0[ok]]
                d = np.abs(got[z].ravel().astype(np.float64) - self.want[z].ravel())
                fin = np.isfinite(self.want[z].ravel())
                assert fin.any() and (d[fin] <= 1e-5 * mag[fin]).all(), (what, float((d[fin] / mag[fin]).max()))
        n = min(nz, len(self.first))
        assert cases.same(got[:n], self.first[:n]), (what, cases.describe_mismatch(got[:n], self.first[:n]))


# ---- DMA rounds per slice: 256 threads on 128 x 8 tiles, ratios that put every tile's chunk count into ((k - 1) * 256, k * 256]
UN_CASES = [(1, k + 1, r) for k, r in enumerate((0.7, 1.5, 2.5, 3.5, 4.5, 5.5))] + \
           [(2, k + 1, r) for k, r in enumerate((0.7, 1.1, 1.5, 1.8, 2.3, 2.8))]


def un_case(stencil, r):
    outX, outY = 256, 16
    inX, inY = int(outX * r) + 8, int(outY * r) + 8  # (nearest needs five source columns per output for six rounds: its tiles span 8 rows)
    px, py = affine(outX, outY, r, 1.3, 1.6)
    return px, py, inX, inY, outX, outY, tile_chunks(stencil, px, py, inX, inY, outX, outY, 128, 8)


@pytest.mark.parametrize("stencil,k,r", UN_CASES)
def test_dma_round_cases_fall_into_their_buckets(stencil, k, r):
    counts = un_case(stencil, r)[-1]
    assert len(counts) == 4 and all((k - 1) * 256 < c <= k * 256 for c in counts), counts


@gpu
@pytest.mark.parametrize("stencil,k,r", UN_CASES)
def test_every_number_of_dma_rounds(fa, tuning_build, monkeypatch, stencil, k, r):
    px, py, inX, inY, outX, outY, counts = un_case(stencil, r)
    for name, v in (("STAGE2_NT", "256"), ("STAGED_MIN_NZ", "1")):
        monkeypatch.setenv("FIMEX_AMD_" + name, v)
    method = oracle.NEAREST if stencil == 1 else oracle.BILINEAR
    plan = fa.RegridPlan(method, px, py, inX, inY, outX, outY)
    info = plan.info()
    assert (info["tileW"], info["tileH"]) == (128, 8) and info["stagedCells"] == 4 * sum(counts), (info, counts)
    f = cases.field(3, inY, inX, seed=k, extremes=False)
    want = oracle.interpolate_values(method, px, py, f, inX, inY, outX, outY)
    got = run_float(fa, plan, f, 3, outX, outY)
    assert cases.same(got, want), cases.describe_mismatch(got, want)


# ---- tile cutting, end to end: the default bilinear shape (1024 threads on 512 x 8 tiles, 5056 chunks per slot) on a map whose
# bands differ.  Rows 0 .. 31 stretch more and more (1.5 .. 4.4 source columns per output column), rows 32 .. 63 stay at 1.5, and in
# rows 32 .. 47 the columns from 768 on cover seven source columns each: some bands must narrow, some only split a tile.
def cutting_case():
    inX, inY, outX, outY = 4516, 85, 1024, 64
    y, x = np.meshgrid(np.arange(outY, dtype=np.float64), np.arange(outX, dtype=np.float64), indexing="ij")
    r = 1.5 + 3.0 * np.minimum(y, 31) / 32
    r[32:] = 1.5
    px = x * r + 1.3
    stretched = (y >= 32) & (y < 48) & (x >= 768)
    px[stretched] = 1152 + 7 * (x[stretched] - 768) + 1.3
    return px.ravel(), (1.2 * y + 1.6).ravel(), inX, inY, outX, outY


def cut_on_the_cpu(px, py, inX, inY, outX, outY):
    """refine_bands (staged_layout.hpp) driven by the numpy footprint above, as build_shape drives it with tile_scan"""
    import staged_layout_host as slh
    lib = slh.load()
    cap = lib.sl_tile_chunk_cap(159 * 1024, 2, 5, 1024, 4)
    assert cap == 5056

    def scan(tiles):
        counts = tile_list_chunks(2, px, py, inX, inY, outX, outY, [(t.x0, t.y0, t.w, 8) for t in tiles])
        return [slh.TOO_LARGE if c is None or c > cap else c for c in counts]
    return slh.cut_tiles(lib, outX, outY, 512, 8, scan)


def test_cutting_case_narrows_a_band_and_splits_tiles():
    """the case does what it is for: some band is narrower than 512, some band keeps its width and holds a split tile, and no tile
    is left to the gather kernel"""
    passes, kept, total = cut_on_the_cpu(*cutting_case())
    last = passes[-1]
    assert kept and len(passes) > 1 and not any(t.gather for t in last)
    assert any(t.band_w < 512 for t in last) and any(t.band_w == 512 and t.w < 512 and t.x0 + t.w < 1024 for t in last)
    print("bands:", {t.band: t.band_w for t in last}, "tiles:", len(last), "staged cells:", 4 * total)


@gpu
def test_tile_cutting_end_to_end(fa, tuning_build, monkeypatch):
    px, py, inX, inY, outX, outY = cutting_case()
    passes, kept, total = cut_on_the_cpu(px, py, inX, inY, outX, outY)
    assert kept
    monkeypatch.setenv("FIMEX_AMD_STAGED_MIN_NZ", "1")
    plan = fa.RegridPlan(oracle.BILINEAR, px, py, inX, inY, outX, outY)
    info = plan.info()
    assert info["stagedCells"] == 4 * total and info["tileW"] == max(t.w for t in passes[-1]) and info["tileH"] == 8, (info, total)
    f = cases.field(3, inY, inX, seed=7, extremes=False)
    want = oracle.interpolate_values(oracle.BILINEAR, px, py, f, inX, inY, outX, outY)
    got = run_float(fa, plan, f, 3, outX, outY)
    assert cases.same(got, want), cases.describe_mismatch(got, want)


# ---- the first staged form: bicubic in the reference's arithmetic keeps it (32 x 16 tiles of 256 threads, row segments of 4 cells)
@gpu
def test_first_form_footprint_and_values(fa, tuning_build, monkeypatch):
    inX, inY, outX, outY = 96, 52, 64, 32
    px, py = affine(outX, outY, 1.3, 1.3, 1.6)
    monkeypatch.setenv("FIMEX_AMD_STAGED_MIN_NZ", "1")
    plan = fa.RegridPlan(oracle.BICUBIC, px, py, inX, inY, outX, outY, bicubic=fa.BICUBIC_REFERENCE)
    info = plan.info()
    counts = tile_chunks(4, px, py, inX, inY, outX, outY, 32, 16, cpc=4)
    assert len(counts) == 4 and (info["tileW"], info["tileH"]) == (32, 16) and info["stagedCells"] == 4 * sum(counts), (info, counts)
    f = cases.field(3, inY, inX, seed=9, extremes=False)
    want = oracle.interpolate_values(oracle.BICUBIC, px, py, f, inX, inY, outX, outY)
    got = run_float(fa, plan, f, 3, outX, outY)
    assert cases.same(got, want), cases.describe_mismatch(got, want)


# ---- ring depth, z chunks shorter than the ring, launch order.  The map overshoots the source on every side: waves with
# undefined and border cells run the loop copy with the selections, the others the plain one.
@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_ring_depth_short_z_chunks_and_chunk_major_order(fa, tuning_build, monkeypatch, kind):
    """STAGE2_DEPTH 2 and 3 with 1, 2, 3 and 7 slices and with chunks of 2, 2, 2, 1 slices (the prologue's and the tail's
    conditions both run), then the chunk-major order (z chunk = blockIdx.y) with the same chunks."""
    case = FloatCase(kind, 320, 18, 256, 16, 1.3, -2.5, -1.7, nz=7)
    tile = (64, 8) if kind == "bicubic" else (128, 8)
    for depth in ("2", "3"):
        plan = case.plan(fa, monkeypatch, {"STAGE2_NT": "256", "STAGE2_DEPTH": depth})
        assert (plan.info()["tileW"], plan.info()["tileH"]) == tile
        for nz in (7, 1, 2, 3):
            case.check(fa, plan, nz, (depth, nz))
        monkeypatch.setenv("FIMEX_AMD_STAGE2_ZPB", "2")
        case.check(fa, plan, 7, (depth, "zpb 2"))
        for k, v in (("STAGE2_ORDER", "0"), ("STAGE2_ZTAIL", "1")):
            monkeypatch.setenv("FIMEX_AMD_" + k, v)
        case.check(fa, plan, 7, (depth, "chunk-major"))
        for k in ("STAGE2_ZPB", "STAGE2_ORDER", "STAGE2_ZTAIL"):
            monkeypatch.delenv("FIMEX_AMD_" + k)


@gpu
@pytest.mark.parametrize("kind,nts", [("nearest", (256, 512, 1024)), ("bilinear", (256, 512, 1024)), ("bicubic", (256, 512)),
                                      ("bicubic_float", (256, 512))])
def test_thread_counts(fa, tuning_build, monkeypatch, kind, nts):
    """STAGE2_NT: 128 x 8, 256 x 8 and 512 x 8 tiles (64 x 8 and 128 x 8 for bicubic in the reference's arithmetic) on a target
    of 600 x 12: a narrow last tile and a tile row that is half empty at every shape."""
    case = FloatCase(kind, 352, 6, 600, 12, 0.6, -1.2, -0.8, nz=5)
    for nt in nts:
        plan = case.plan(fa, monkeypatch, {"STAGE2_NT": str(nt)})
        assert plan.info()["tileW"] == (nt // 4 if kind == "bicubic" else nt // 2)
        case.check(fa, plan, 5, nt)


# ---- stored types.  Target rows 16 .. 23 (a whole tile row at every shape) lie below the source: tiles without chunks.  One
# cell of the first tile row points 185 rows further down than its neighbours: more source rows than a tile may span, so the
# plan splits that tile down to 64 columns and makes the piece with the outlier a gather tile.
def typed_case(dt, method, outX):
    inX, inY, outY, nz = 200, 190, 24, 5
    px = affine(outX, outY, 0.5, -0.8, 0)[0]
    py = affine(outX, outY, 12.0, 0, -1.0)[1]  # target row 0 lies above the source, row 15 in row 179, row 16 below it
    px[2 * outX + 10], py[2 * outX + 10] = 150.3, 185.4
    assert py.reshape(outY, outX)[16:].min() > inY and py.reshape(outY, outX)[:16].max() < inY - 1
    info = np.iinfo(dt)
    bad = float(info.min + 3)
    rng = np.random.default_rng(outX + np.dtype(dt).itemsize)
    f = rng.integers(info.min, int(info.max) + 1, (nz, inY, inX)).astype(dt)
    f.reshape(-1)[rng.random(f.size) < 0.03] = dt(bad)  # a fill value that occurs in the data
    want = oracle.interpolation_array2data(
        oracle.interpolate_values(method, px, py, oracle.data2interpolation_array(f, bad), inX, inY, outX, outY), oracle.cdm_type_of(dt), bad)
    return px, py, inX, inY, outY, nz, bad, f, want


def run_typed(fa, plan, f, nz, bad, want):
    import torch
    t = torch.from_numpy(f.view(np.uint8)).cuda()
    out = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda")
    fa.regrid_apply_typed_device(plan, t.data_ptr(), oracle.cdm_type_of(f.dtype), nz, bad, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(f.dtype).reshape(want.shape)


@gpu
@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR])
@pytest.mark.parametrize("dt", [np.int16, np.uint8])
@pytest.mark.parametrize("outX", [384, 383])
def test_stored_types_single_stores_depth_and_special_tiles(fa, tuning_build, monkeypatch, method, dt, outX):
    """STAGE2T_PAIR 0 and 1 on even and odd row lengths, STAGE2T_DEPTH 2 and 3 (512 threads), with the tiles described above."""
    px, py, inX, inY, outY, nz, bad, f, want = typed_case(dt, method, outX)
    for depth in ("2", "3"):
        monkeypatch.setenv("FIMEX_AMD_STAGE2T_DEPTH", depth)
        plan = fa.RegridPlan(method, px, py, inX, inY, outX, outY)
        assert plan.info()["stagedCells"] > 0
        for pair in ("1", "0"):
            monkeypatch.setenv("FIMEX_AMD_STAGE2T_PAIR", pair)
            got = run_typed(fa, plan, f, nz, bad, want)
            assert np.array_equal(got, want), (depth, pair, int((got != want).sum()))


@gpu
@pytest.mark.parametrize("nt", [256, 512, 1024])
@pytest.mark.parametrize("dt,method", [(np.int16, oracle.BILINEAR), (np.uint8, oracle.NEAREST)])
def test_stored_types_thread_counts(fa, tuning_build, monkeypatch, nt, dt, method):
    px, py, inX, inY, outY, nz, bad, f, want = typed_case(dt, method, 384)
    monkeypatch.setenv("FIMEX_AMD_STAGE2T_NT", str(nt))
    plan = fa.RegridPlan(method, px, py, inX, inY, 384, outY)
    got = run_typed(fa, plan, f, nz, bad, want)
    assert np.array_equal(got, want), int((got != want).sum())
