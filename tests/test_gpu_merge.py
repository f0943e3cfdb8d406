"""Grid merging on the GPU (include/fimex_amd.h): border smoothing, overlay and the fused CDMMerger against
tests/merge_ref.py, the CPU restatement that tests/test_merge_ref.py pins to the reference's known answers.

The bar is bit-identical, NaN positions and the sign of zero included: every operation of the kernels is the same IEEE operation in
the same order as the restatement's (float64 subtract, multiply, add, divide and square root are correctly rounded on both sides, the
regrids are those of the oracle).  Every cell is compared; the share of bit-identical cells is printed before the assertion.
"""
import functools

import numpy as np
import pytest

import merge_ref as mr
import oracle

pytestmark = pytest.mark.gpu

TILE_X, TILE_Y = 64, 4  # the workgroup tile of the merge kernels (csrc/merge.hip)
MULTI_TILE = (2 * TILE_X + 22, 2 * TILE_Y + 3)  # nx, ny: two full tiles and a partial one each way


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    lib = capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    assert hasattr(lib, "fimex_amd_merge_apply_device")
    return capi


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, np.float32)).cuda()  # a copy: the shared inputs are read-only


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _identical(got, want, label):
    """NaN in the same cells, every other cell the same 32 bits; prints the share of bit-identical cells first"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (label, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    same = (gn & wn) | (~gn & ~wn & (got.view(np.uint32) == want.view(np.uint32)))
    print("%s: %d cells, %d NaN, %.4f %% bit-identical" % (label, want.size, np.count_nonzero(wn), 100.0 * np.count_nonzero(same) / max(want.size, 1)))
    if not np.all(same):
        i = np.argwhere(~same)[0]
        raise AssertionError("%s: %d cells differ; first at %s: got %r want %r" % (label, np.count_nonzero(~same), tuple(i), got[tuple(i)], want[tuple(i)]))


# ---------------------------------------------------------------------------------------------------------------- border_smooth
SMOOTH_SHAPES = [(1, 1), (3, 9), (9, 3), (4, 4), (11, 11), (14, 14), (15, 17), MULTI_TILE]
SMOOTH_WIDTHS = [(5, 2), (1, 0), (3, 4), (9, 20)]  # (tw, bw): with the shapes above, wrapping bounds, overlapping and touching bands


@functools.lru_cache(maxsize=None)
def _smooth_fields(nx, ny, nz, seed):
    """(I, O): about 10 % NaN in each, placed independently, and a few infinities, zeros of either sign and equal values"""
    rng = np.random.default_rng(seed)
    I = rng.normal(280, 5, (nz, ny, nx)).astype(np.float32)
    O = rng.normal(280, 5, (nz, ny, nx)).astype(np.float32)
    n = I.size
    special = [(np.inf, 1.), (1., -np.inf), (np.inf, np.inf), (-np.inf, np.inf), (0., -0.), (-0., 0.), (0., 0.), (3.5, 3.5), (0., 1.), (-0., 2.)]
    for k, (vi, vo) in enumerate(special * 3):
        p = int(rng.integers(n))
        I.flat[p], O.flat[p] = vi, vo
    I[rng.random(I.shape) < 0.1] = np.nan
    O[rng.random(O.shape) < 0.1] = np.nan
    I.setflags(write=False)
    O.setflags(write=False)
    return I, O


def _smooth_all_ways(fa, nx, ny, tw, bw, seed):
    import torch
    for nz in (1, 3, 5):
        I, O = _smooth_fields(nx, ny, nz, seed + nz)
        for use_outer in (True, False):
            want = mr.border_smooth(I, O, tw, bw, use_outer)
            label = "border_smooth %dx%dx%d tw %d bw %d useOuter %d" % (nx, ny, nz, tw, bw, use_outer)
            dI, dO = _dev(I), _dev(O)
            out = torch.full((nz, ny, nx), -7.0, dtype=torch.float32, device="cuda")
            fa.border_smooth_device(dI.data_ptr(), dO.data_ptr(), out.data_ptr(), nx, ny, nz, tw, bw, use_outer, _stream())
            _identical(out.cpu().numpy(), want, label + " out of place")
            assert np.array_equal(dI.cpu().numpy().view(np.uint32), I.view(np.uint32)) and np.array_equal(dO.cpu().numpy().view(np.uint32), O.view(np.uint32))
            fa.border_smooth_device(dI.data_ptr(), dO.data_ptr(), dO.data_ptr(), nx, ny, nz, tw, bw, use_outer, _stream())
            _identical(dO.cpu().numpy(), want, label + " in place on the outer")
            dO = _dev(O)
            fa.border_smooth_device(dI.data_ptr(), dO.data_ptr(), dI.data_ptr(), nx, ny, nz, tw, bw, use_outer, _stream())
            _identical(dI.cpu().numpy(), want, label + " in place on the inner")


@pytest.mark.parametrize("widths", SMOOTH_WIDTHS, ids=lambda w: "tw%d-bw%d" % w)
@pytest.mark.parametrize("shape", SMOOTH_SHAPES, ids=lambda s: "%dx%d" % s)
def test_border_smooth(fa, shape, widths):
    _smooth_all_ways(fa, shape[0], shape[1], widths[0], widths[1], 1000 * shape[0] + shape[1])


def test_border_smooth_every_corner_distance(fa):
    """tw = 64 on 140 x 136: every corner pair (dx, dy) <= 64 occurs, so every double square root the kernel can take is compared"""
    kind, alpha = mr._alpha_planes(140, 136, 64, 2)
    assert np.count_nonzero(kind == 2) > 64 * 64 * 4 and np.unique(alpha[kind == 2]).size > 1000
    _smooth_all_ways(fa, 140, 136, 64, 2, 77)


def test_border_smooth_host(fa):
    I, O = _smooth_fields(MULTI_TILE[0], MULTI_TILE[1], 3, 5)
    _identical(fa.border_smooth_host(I, O, 5, 2, True), mr.border_smooth(I, O, 5, 2, True), "border_smooth host")
    _identical(fa.border_smooth_host(I[0], O[0], 3, 1, False), mr.border_smooth(I[0], O[0], 3, 1, False), "border_smooth host, one slice")


# ---------------------------------------------------------------------------------------------------------------------- overlay
@pytest.mark.parametrize("n", [1, 63, 65, 2 * 4 * 256 + 37], ids=lambda n: "n%d" % n)
def test_overlay(fa, n):
    import torch
    rng = np.random.default_rng(n)
    top, base = rng.normal(0, 1, n).astype(np.float32), rng.normal(0, 1, n).astype(np.float32)
    top[rng.random(n) < 0.4] = np.nan   # NaN in the top, in the base, in both
    base[rng.random(n) < 0.4] = np.nan
    top[0] = np.nan if n > 1 else top[0]
    if n > 4:
        top[1], base[1] = np.nan, np.nan
        top[2], base[2] = -0.0, 1.0
        top[3], base[3] = np.nan, -0.0
    want = mr.overlay(top, base)
    dT, dB = _dev(top), _dev(base)
    out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    fa.overlay_device(dT.data_ptr(), dB.data_ptr(), out.data_ptr(), n, _stream())
    _identical(out.cpu().numpy(), want, "overlay %d out of place" % n)
    fa.overlay_device(dT.data_ptr(), dB.data_ptr(), dB.data_ptr(), n, _stream())
    _identical(dB.cpu().numpy(), want, "overlay %d in place on the base" % n)
    dB = _dev(base)
    fa.overlay_device(dT.data_ptr(), dB.data_ptr(), dT.data_ptr(), n, _stream())
    _identical(dT.cpu().numpy(), want, "overlay %d in place on the top" % n)
    _identical(fa.overlay_host(top, base), want, "overlay %d host" % n)


# ------------------------------------------------------------------------------------------------------------------ merge_apply
class Axes:
    """a grid in a common plane: cell (i, j) lies at origin + i * ex * step + j * ey * step, ex the unit vector at `angle`"""

    def __init__(self, nx, ny, x0, y0, step, angle=0.0):
        self.nx, self.ny, self.x0, self.y0, self.step, self.angle = nx, ny, x0, y0, step, angle

    @property
    def shape(self):
        return self.ny, self.nx

    def mesh(self):
        i, j = np.meshgrid(np.arange(self.nx, dtype=np.float64), np.arange(self.ny, dtype=np.float64))
        c, s = np.cos(self.angle), np.sin(self.angle)
        return self.x0 + self.step * (c * i - s * j), self.y0 + self.step * (s * i + c * j)

    def index_of(self, X, Y):
        """fractional (column, row) of points of the plane on this grid"""
        c, s = np.cos(self.angle), np.sin(self.angle)
        dx, dy = (X - self.x0) / self.step, (Y - self.y0) / self.step
        return (c * dx + s * dy).ravel(), (-s * dx + c * dy).ravel()


def _pos(src, dst):
    return src.index_of(*dst.mesh())


OUTER = Axes(30, 28, 0., 0., 4.)
INNER_INSIDE = Axes(40, 36, 30.5, 28.25, 1.)        # 40 x 36 inside the 30 x 28 outer of four times the step
INNER_ROW_OUT = Axes(40, 36, 30.5, 110.5 - 35., 1.)  # its last row lies more than half an outer cell beyond the outer's last row (y = 108)
TARGET_ROTATED = Axes(2 * TILE_X + 9, 2 * TILE_Y + 39, 22.3, 31.7, 0.83, np.radians(17.))  # shifted and rotated: stencils straddle cells


def _extended_target(inner, outer):
    """the target of setTargetGridFromInner: both inner axes continued over the outer grid"""
    x = mr.extend_inner_axis(inner.x0 + inner.step * np.arange(inner.nx), outer.x0 + outer.step * np.arange(outer.nx))
    y = mr.extend_inner_axis(inner.y0 + inner.step * np.arange(inner.ny), outer.y0 + outer.step * np.arange(outer.ny))
    assert x.size > inner.nx and y.size > inner.ny and np.allclose(np.diff(x), inner.step) and np.allclose(np.diff(y), inner.step)
    return Axes(x.size, y.size, x[0], y[0], inner.step)


GEOMETRIES = {
    "inside-extended": (INNER_INSIDE, OUTER, _extended_target(INNER_INSIDE, OUTER)),
    "inside-rotated": (INNER_INSIDE, OUTER, TARGET_ROTATED),
    "rowout-rotated": (INNER_ROW_OUT, OUTER, TARGET_ROTATED),
}


@functools.lru_cache(maxsize=None)
def _merge_fields(geometry, nz):
    """(I, O) with NaN holes in the inner's interior and frame and in the outer"""
    inner, outer, _ = GEOMETRIES[geometry]
    rng = np.random.default_rng(nz * 31 + len(geometry))

    def field(g):
        X, Y = g.mesh()
        z = np.arange(nz, dtype=np.float64)[:, None, None]
        return (280 + 5 * np.sin(X / 17 + z) + 3 * np.cos(Y / 11 - z) + rng.normal(0, 0.3, (nz,) + g.shape)).astype(np.float32)

    I, O = field(inner), field(outer)
    I[:, 15:19, 20:24] = np.nan          # interior
    I[0, 0:3, 0:6] = np.nan              # frame and transition band, corner
    I[:, 30:36, 37:40] = np.nan          # frame, far corner
    I[rng.random(I.shape) < 0.01] = np.nan
    O[:, 9:11, 10:12] = np.nan           # under the inner grid
    O[:, 20:22, 3:5] = np.nan            # beside it
    O[rng.random(O.shape) < 0.01] = np.nan
    I.setflags(write=False)
    O.setflags(write=False)
    return I, O


@functools.lru_cache(maxsize=None)
def _positions(geometry):
    inner, outer, target = GEOMETRIES[geometry]
    return _pos(outer, inner), _pos(inner, target), _pos(outer, target)


@functools.lru_cache(maxsize=None)
def _want(geometry, nz, smooth_method, method, use_outer):
    inner, outer, target = GEOMETRIES[geometry]
    I, O = _merge_fields(geometry, nz)
    out, S = mr.merge(I, O, _positions(geometry), (inner.shape, outer.shape, target.shape), method, smooth_method, 5, 2, use_outer)
    out.setflags(write=False)
    return out, S


def _plans(fa, geometry, smooth_method, method, tw=5, bw=2, use_outer=True):
    inner, outer, target = GEOMETRIES[geometry]
    (oix, oiy), (itx, ity), (otx, oty) = _positions(geometry)
    oi = fa.RegridPlan(smooth_method, oix, oiy, outer.nx, outer.ny, inner.nx, inner.ny)
    it = fa.RegridPlan(method, itx, ity, inner.nx, inner.ny, target.nx, target.ny)
    ot = fa.RegridPlan(method, otx, oty, outer.nx, outer.ny, target.nx, target.ny)
    return fa.MergePlan(oi, it, ot, tw, bw, use_outer), (oi, it, ot)


B, N, C = oracle.BILINEAR, oracle.NEAREST, oracle.BICUBIC
# (geometry, method of step 1, method of steps 3 and 4, nz, useOuter)
MERGE_CASES = [
    ("inside-extended", B, B, 3, True),
    ("inside-extended", N, N, 1, True),
    ("inside-extended", C, C, 3, False),
    ("inside-rotated", B, C, 9, True),    # mixed: a bilinear step 1 in front of a bicubic step 3
    ("inside-rotated", B, B, 1, False),
    ("rowout-rotated", B, B, 9, False),
    ("rowout-rotated", C, C, 1, True),
    ("rowout-rotated", N, N, 3, False),
]


@pytest.mark.parametrize("case", MERGE_CASES, ids=lambda c: "%s-m%d-m%d-nz%d-outer%d" % c)
def test_merge_apply(fa, case):
    import torch
    geometry, smooth_method, method, nz, use_outer = case
    inner, outer, target = GEOMETRIES[geometry]
    I, O = _merge_fields(geometry, nz)
    want, S = _want(geometry, nz, smooth_method, method, use_outer)
    # the case holds what it is meant to hold
    if geometry.startswith("rowout"):  # invalid plan entries under the inner's last row: OI NaN -> I
        oi = oracle.interpolate_values(smooth_method, *_positions(geometry)[0], np.zeros(outer.shape, np.float32), outer.nx, outer.ny, inner.nx, inner.ny)
        assert np.all(np.isnan(oi[0, -1])) and not np.all(np.isnan(oi[0, -12]))
        _identical(S[:, -1], I[:, -1], "the smoothed inner's last row")
    assert np.isnan(want).any() and np.isfinite(want).mean() > 0.5 and (use_outer or np.isnan(S).any())
    label = "merge %s step1 %d steps34 %d nz %d useOuter %d" % case
    plan, keep = _plans(fa, geometry, smooth_method, method, 5, 2, use_outer)
    dI, dO = _dev(I), _dev(O)
    fused = torch.full((nz,) + target.shape, -7.0, dtype=torch.float32, device="cuda")
    chain = torch.full((nz,) + target.shape, -9.0, dtype=torch.float32, device="cuda")
    plan.apply_device(dI.data_ptr(), dO.data_ptr(), nz, fused.data_ptr(), _stream())
    plan.apply_chain_device(dI.data_ptr(), dO.data_ptr(), nz, chain.data_ptr(), _stream())
    fused, chain = fused.cpu().numpy(), chain.cpu().numpy()
    _identical(fused, want, label + " fused")
    _identical(chain, want, label + " chain")
    _identical(fused, chain, label + " fused against chain")
    assert np.array_equal(dI.cpu().numpy().view(np.uint32), I.view(np.uint32)) and np.array_equal(dO.cpu().numpy().view(np.uint32), O.view(np.uint32))
    plan.close()


def test_merge_apply_host(fa):
    geometry, nz = "inside-rotated", 3
    I, O = _merge_fields(geometry, nz)
    want, _ = _want(geometry, nz, B, B, True)
    plan, keep = _plans(fa, geometry, B, B)
    _identical(plan.apply_host(I, O), want, "merge host")
    plan.close()


def test_merge_smoothing_widths_reach_the_fused_kernel(fa):
    """another (tw, bw) than the default through the merge plan: the overlapping bands of a 40 x 36 inner with tw 15, bw 6"""
    import torch
    geometry, nz = "inside-extended", 3
    inner, outer, target = GEOMETRIES[geometry]
    I, O = _merge_fields(geometry, nz)
    want, _ = mr.merge(I, O, _positions(geometry), (inner.shape, outer.shape, target.shape), B, B, 15, 6, True)
    plan, keep = _plans(fa, geometry, B, B, 15, 6, True)
    dI, dO = _dev(I), _dev(O)
    out = torch.full((nz,) + target.shape, -7.0, dtype=torch.float32, device="cuda")
    plan.apply_device(dI.data_ptr(), dO.data_ptr(), nz, out.data_ptr(), _stream())
    _identical(out.cpu().numpy(), want, "merge tw 15 bw 6")
    plan.close()


# --------------------------------------------------------------------------------------- the reference's fixtures, end to end
@pytest.mark.parametrize("name", sorted(mr.KNOWN))
def test_reference_fixtures_through_the_library(fa, golden_dir, name):
    """test/testMerger.cc: positions from the library's project_axes and points2position, three regrid plans, the merge plan; the
    known answers within the reference's bounds, the whole field equal to the restatement fed with the same positions"""
    shape, known, bound = mr.KNOWN[name]
    c = mr.load_case(golden_dir, name)
    assert c["target"].shape == shape
    pos = mr.merge_positions(c["inner"], c["outer"], c["target"], project_axes=fa.project_axes_host, points2position=fa.points2position_host,
                             types=(fa.PROJ_AXIS, fa.LONGITUDE, fa.LATITUDE))
    (iy, ix), (oy, ox), (ty, tx) = mr.case_shapes(c)
    oi = fa.RegridPlan(fa.BILINEAR, pos[0][0], pos[0][1], ox, oy, ix, iy)
    it = fa.RegridPlan(fa.BILINEAR, pos[1][0], pos[1][1], ix, iy, tx, ty)
    ot = fa.RegridPlan(fa.BILINEAR, pos[2][0], pos[2][1], ox, oy, tx, ty)
    plan = fa.MergePlan(oi, it, ot)  # CDMMerger's defaults: LINEAR(5, 2), use the outer where the inner is undefined
    got = plan.apply_host(c["I"], c["O"])
    assert got.shape == (1,) + shape
    for kx, ky, expected in known:
        print("%s (%d, %d): %.6f, expected %s" % (name, kx, ky, float(got[0, ky, kx]), expected))
        assert abs(float(got[0, ky, kx]) - expected) < bound
    want, _ = mr.merge(c["I"], c["O"], pos, mr.case_shapes(c))
    _identical(got, want, name + " whole field")
    plan.close()


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(fa):
    import torch
    nan_free = _dev(np.zeros((2, 6, 5), np.float32))
    out = torch.zeros((2, 6, 5), dtype=torch.float32, device="cuda")
    p = (nan_free.data_ptr(), nan_free.data_ptr(), out.data_ptr())
    with pytest.raises(fa.FimexAmdError, match="transitionWidth == 0"):
        fa.border_smooth_device(*p, 5, 6, 2, 0, 2, True, _stream())
    with pytest.raises(fa.FimexAmdError, match="transitionWidth == 0"):
        fa.border_smooth_host(np.zeros((6, 5), np.float32), np.zeros((6, 5), np.float32), 0, 2)
    for nx, ny in ((0, 6), (5, 0)):
        with pytest.raises(fa.FimexAmdError, match="empty grid"):
            fa.border_smooth_device(*p, nx, ny, 2, 5, 2, True, _stream())
    with pytest.raises(fa.FimexAmdError, match="overlaps"):  # partly overlapping output
        fa.border_smooth_device(p[0], p[1], p[0] + 4, 5, 6, 2, 5, 2, True, _stream())
    with pytest.raises(fa.FimexAmdError, match="overlaps"):
        fa.overlay_device(p[0], p[2], p[0] + 4, 59, _stream())
    # nothing to do: no error, nothing written
    fa.border_smooth_device(0, 0, 0, 5, 6, 0, 5, 2, True, _stream())
    fa.overlay_device(0, 0, 0, 0, _stream())

    geometry = "inside-rotated"
    inner, outer, target = GEOMETRIES[geometry]
    plan, (oi, it, ot) = _plans(fa, geometry, B, B)
    with pytest.raises(fa.FimexAmdError, match="transitionWidth == 0"):
        fa.MergePlan(oi, it, ot, 0, 2)
    with pytest.raises(fa.FimexAmdError, match="do not chain"):
        fa.MergePlan(it, it, ot)   # "outer -> inner" reads the inner grid
    with pytest.raises(fa.FimexAmdError, match="do not chain"):
        fa.MergePlan(oi, ot, ot)   # "inner -> target" reads the outer grid
    with pytest.raises(fa.FimexAmdError, match="do not chain"):
        fa.MergePlan(oi, it, oi)   # "outer -> target" writes the inner grid
    rng = np.random.default_rng(3)
    fwd = fa.RegridPlan(fa.FORWARD_MEAN, rng.uniform(0, inner.nx - 1, outer.nx * outer.ny), rng.uniform(0, inner.ny - 1, outer.nx * outer.ny),
                        outer.nx, outer.ny, inner.nx, inner.ny)
    with pytest.raises(fa.FimexAmdError, match="backward plans"):
        fa.MergePlan(fwd, it, ot)
    # nz == 0 is a successful no-op, as for the regrid applies
    plan.apply_device(0, 0, 0, 0, _stream())
    plan.apply_chain_device(0, 0, 0, 0, _stream())
    with pytest.raises(fa.FimexAmdError, match="NULL"):
        plan.apply_device(0, 0, 1, 0, _stream())
    dI, dO = _dev(np.zeros((1,) + inner.shape, np.float32)), _dev(np.zeros((1,) + outer.shape, np.float32))
    with pytest.raises(fa.FimexAmdError, match="overlaps"):
        plan.apply_device(dI.data_ptr(), dO.data_ptr(), 1, dI.data_ptr(), _stream())
    if fa.device_count() >= 2:  # a plan on another device than the calling thread's
        fa.set_device(1)
        try:
            with pytest.raises(fa.FimexAmdError, match="lives on device"):
                plan.apply_device(p[0], p[0], 1, p[2], 0)
        finally:
            fa.set_device(0)
    plan.close()
