"""The vertical velocity on model levels, the grid distance and omega -> vertical wind on the GPU (include/fimex_amd.h, 8f n7) against
tests/vertical_velocity_ref.py, the CPU restatement that tests/test_vertical_velocity_ref.py pins to the reference's object code, and
against the recorded answers of tests/golden/vertical_velocity_answers.npz.  Every cell is compared; NaN and infinity positions must
be identical.

Tolerances, from the arithmetic:
  vertical velocity  |got - want| <= 2^-23 |want| + nz * 2^-50 * M.  The only operation that differs from the host is the FP64 log, a
                     couple of units in the last place (2^-51 relative); its error enters z once per level below the cell and enters w
                     multiplied by what M collects (the magnitude of the terms that cancel in w1 + w2, returned by the restatement);
                     the final rounding to float adds one float step.
  grid distance      |got - want| <= 2^-23 |want| + 6371000 * 2^-49 / sin(want / 6371000): one float step and the conditioning of
                     acos near 1 for an argument that carries a few units in the last place from sin and cos.
  omega              bit-identical (three float operations).
The share of bit-identical cells is printed (recorded in DESIGN.md 6.7, not asserted).
"""
import functools

import numpy as np
import pytest

import cases
import vertical_ref as vr
import vertical_velocity_ref as vv

pytestmark = pytest.mark.gpu

TILE_X, TILE_Y = 64, 4  # the workgroup tile of the divergence pass (csrc/vertical_velocity.hip)
MULTI_TILE = (2 * TILE_X + 22, 2 * TILE_Y + 3)  # nx, ny: two full tiles and a partial one each way


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    lib = capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    assert hasattr(lib, "fimex_amd_vertical_velocity_device")
    return capi


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return vv.load_fixture(golden_dir)


@functools.lru_cache(maxsize=None)
def _case(seed, nx, ny, nz, nt, nan_frac=0.0):
    """(case, want, M), computed once and shared; nobody writes to it."""
    c = vv.make_case(seed, nx, ny, nz, nt, nan_frac)
    want, M = vv.vertical_velocity(*vv.velocity_args(c))
    return c, want, M


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _compare(got, want, tol, label):
    """NaN and infinity positions identical, every finite cell within tol; prints the share of bit-identical cells."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN positions differ in %d cells" % (label, np.count_nonzero(gn != wn))
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), label + ": infinities differ"
    fin = np.isfinite(want)
    g, w = got[fin].astype(np.float64), want[fin].astype(np.float64)
    err = np.abs(g - w)
    t = np.broadcast_to(tol, want.shape)[fin]
    same = np.count_nonzero(got[fin].view(np.uint32) == want[fin].view(np.uint32))
    print("%s: %d finite cells, %d NaN, %.4f %% bit-identical, max error / tolerance %.3f"
          % (label, g.size, np.count_nonzero(wn), 100.0 * same / max(g.size, 1), float(np.max(err / np.maximum(t, 1e-300))) if g.size else 0.0))
    bad = err > t
    assert not np.any(bad), "%s: %d cells over the tolerance; worst: got %r want %r tol %r" % (
        label, np.count_nonzero(bad), g[bad][np.argmax((err - t)[bad])], w[bad][np.argmax((err - t)[bad])], t[bad][np.argmax((err - t)[bad])])


def _velocity_host(fa, c):
    nt, nz, ny, nx = c["t"].shape
    return fa.vertical_velocity_host(nx, ny, nt, *vv.velocity_args(c))


def _velocity_device(fa, c):
    """-> (w as a torch tensor, the tensors it was made from)."""
    import torch
    nt, nz, ny, nx = c["t"].shape
    d = {k: _dev(c[k]) for k in ("gridDistX", "gridDistY", "zs", "ps", "u", "v", "t")}
    w = torch.full((nt, nz, ny, nx), -7.0, dtype=torch.float32, device="cuda")
    fa.vertical_velocity_device(nx, ny, nt, c["dx"], c["dy"], d["gridDistX"].data_ptr(), d["gridDistY"].data_ptr(), c["ap"], c["b"],
                                d["zs"].data_ptr(), d["ps"].data_ptr(), d["u"].data_ptr(), d["v"].data_ptr(), d["t"].data_ptr(), w.data_ptr(),
                                stream=_stream())
    return w, d


# (nx, ny, nz, nt): the smallest grid, one level (w = 0), the two orientations, a multi-tile grid with a level group of four plus a
# remainder plus level 0 and three time steps (the scratch of one step is reused), and a deeper column
SHAPES = [(3, 3, 1, 1), (3, 3, 2, 1), (7, 5, 4, 1), (5, 7, 4, 3), MULTI_TILE + (6, 3), (67, 35, 10, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_vertical_velocity_matches_the_cpu_restatement(fa, shape):
    nx, ny, nz, nt = shape
    c, want, M = _case(20 + nx, nx, ny, nz, nt)
    assert np.all(np.isfinite(want)) and np.all(want[:, 0].view(np.uint32) == 0)
    got = _velocity_host(fa, c)
    assert np.all(got[:, 0].view(np.uint32) == 0), "w at level 0 is +0"
    _compare(got, want, vv.velocity_tolerance(want, M, nz), "vertical velocity %dx%dx%dx%d" % shape)
    if nz > 1 and nx * ny > 9:
        assert np.abs(want[:, 1:]).max() > 0.1 and np.max(M[:, 1:] / np.maximum(np.abs(want[:, 1:]), 1e-30)) > 100  # w1 and w2 cancel


@pytest.mark.parametrize("name", [c[0] for c in vv.RECORDED_VELOCITY])
def test_vertical_velocity_matches_the_recorded_answers(fa, fixture, name):
    c = {k: fixture["velocity.%s.%s" % (name, k)] for k in vv.VELOCITY_ARGS}
    c["dx"], c["dy"] = float(c["dx"]), float(c["dy"])
    want = fixture["velocity.%s.w" % name].view(np.float32)
    _, M = vv.vertical_velocity(*vv.velocity_args(c))
    _compare(_velocity_host(fa, c), want, vv.velocity_tolerance(want, M, want.shape[1]), "recorded vertical velocity " + name)


def test_vertical_velocity_with_nan(fa):
    """1 % NaN in T and u: NaN in exactly the reference's cells, and at least half of the cells stay finite, so that the NaN cannot
    hide the arithmetic."""
    nx, ny, nz, nt = 67, 35, 9, 1
    c, want, M = _case(31, nx, ny, nz, nt, 0.01)
    assert np.isnan(c["t"]).any() and np.isnan(c["u"]).any()
    assert np.isnan(want).any() and np.isfinite(want).mean() >= 0.5
    _compare(_velocity_host(fa, c), want, vv.velocity_tolerance(want, M, nz), "vertical velocity with NaN")


def test_vertical_velocity_with_a_non_positive_pressure(fa):
    """A negative ap puts the half-level pressure of one level below zero in the column of the lowest ps alone: whatever IEEE
    arithmetic gives there and in the cells that read it, in the same cells as the restatement."""
    nx, ny, nz, nt = 9, 7, 5, 1
    c = dict(vv.make_case(32, nx, ny, nz, nt))
    k = 2
    ah, bh = vv.half_levels(c["ap"], c["b"])
    ps = np.sort(c["ps"].astype(np.float64).reshape(-1))
    assert ps[0] < ps[1]
    c["ap"] = c["ap"].copy()
    c["ap"][k] = (-bh[k] * 0.5 * (ps[0] + ps[1]) + ah[k + 1]) / 2
    assert c["ap"][k] < 0
    ah, bh = vv.half_levels(c["ap"], c["b"])
    assert np.count_nonzero(ah[k] + bh[k] * c["ps"].astype(np.float64) <= 0) == 1
    want, M = vv.vertical_velocity(*vv.velocity_args(c))
    assert np.isnan(want).any() and np.isfinite(want).mean() >= 0.5
    _compare(_velocity_host(fa, c), want, vv.velocity_tolerance(want, M, nz), "vertical velocity with a non-positive pressure")


def test_vertical_velocity_host_and_device_entries_agree(fa):
    import torch
    nx, ny, nz, nt = MULTI_TILE + (6, 3)
    c, want, M = _case(20 + nx, nx, ny, nz, nt)
    w, _ = _velocity_device(fa, c)
    torch.cuda.synchronize()
    got = w.cpu().numpy()
    assert cases.same(got, _velocity_host(fa, c))
    _compare(got, want, vv.velocity_tolerance(want, M, nz), "vertical velocity, device entry")
    for t in range(1, nt):  # the time steps differ, so a stale scratch would show
        assert not np.array_equal(want[t], want[0])


def test_vertical_velocity_feeds_the_vertical_interpolation(fa):
    """u, v, T, ps and orography on hybrid levels -> w -> pressure levels, all on device buffers.  The interpolation must be
    vertical_ref's, bit for bit, of the same GPU-made w (w itself is compared in the tests above)."""
    import torch
    nx, ny, nz, nt = 67, 35, 10, 2
    c, _, _ = _case(41, nx, ny, nz, nt)
    level1 = np.array([1000.0, 30000.0, 60000.0, 85000.0, 200000.0])  # Pa; the first above every column, the last below the ground
    st = _stream()
    w, d = _velocity_device(fa, c)
    out = torch.zeros((nt, level1.size, ny, nx), dtype=torch.float32, device="cuda")
    fa.vertical_interpolate_device(vr.LIN, nx, ny, nt, w.data_ptr(), fa.VerticalLevels.hybrid_sigma_ap(c["ap"], c["b"], d["ps"].data_ptr()),
                                   out.data_ptr(), level1=level1, stream=st)
    torch.cuda.synchronize()
    field = w.cpu().numpy()
    levels = vr.level_field(vr.Levels(vr.HYBRID_SIGMA_AP, nz, ap=c["ap"], b=c["b"], ps=c["ps"]), nt, ny, nx)
    want = vr.interpolate(vr.LIN, field, levels, level1[None, :, None, None])
    got = out.cpu().numpy()
    assert cases.same(got, want), cases.describe_mismatch(got, want)
    assert np.all(np.isfinite(got[:, 1:4])) and np.abs(got[:, 1:4]).max() > 0.1


# ------------------------------------------------------------------ grid distance
GRIDS = [(3, 3), (7, 5), (5, 7), (13, 4), (1, 9), (9, 1), (2, 2), (300, 5)]  # 13 x 4: a chain of three in the last row; 300 x 5: six workgroups


def _check_grid(got, want, label):
    assert not np.isnan(want).any(), "the reference returns no NaN on such a grid"
    assert not np.isnan(got).any(), label + ": NaN"
    with np.errstate(invalid="ignore"):
        tol = np.where(want == 0, 0.0, vv.griddistance_tolerance(want))
    _compare(got, want, tol, "grid distance " + label)


@pytest.mark.parametrize("lat0", [0.5, 60.0, 89.0])
@pytest.mark.parametrize("shape", GRIDS, ids=lambda s: "%dx%d" % s)
def test_grid_distance_matches_the_cpu_restatement(fa, shape, lat0):
    import torch
    nx, ny = shape
    lon, lat = vv.make_grid(nx * 100 + ny, nx, ny, lat0=lat0)
    wx, wy, rc = vv.griddistance(lon, lat)
    assert rc == vv.OK and wx.min() > 0 and wy.min() > 0  # no duplicate points
    gx, gy = fa.griddistance_host(lon, lat)
    _check_grid(gx, wx, "%dx%d X at %g" % (nx, ny, lat0))
    _check_grid(gy, wy, "%dx%d Y at %g" % (nx, ny, lat0))
    d_lon, d_lat = _dev(lon, np.float64), _dev(lat, np.float64)
    dx, dy = torch.full((ny, nx), -1.0, device="cuda"), torch.full((ny, nx), -1.0, device="cuda")
    fa.griddistance_device(nx, ny, d_lon.data_ptr(), d_lat.data_ptr(), dx.data_ptr(), dy.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    assert cases.same(dx.cpu().numpy(), gx) and cases.same(dy.cpu().numpy(), gy)
    if nx > 1 and ny > 1:  # the copies are copies
        assert np.array_equal(gx[:-1, -1], gx[:-1, -2]) and np.array_equal(gy[:-1, -1], gy[:-1, -2])
        src = [(ny - 1) * nx + (i % ny) - ny for i in range(nx)]
        assert np.array_equal(gx[-1], gx.reshape(-1)[src]) and np.array_equal(gy[-1], gy.reshape(-1)[src])


@pytest.mark.parametrize("name", [g[0] for g in vv.RECORDED_GRIDS if g[0] != "g1x1"])
def test_grid_distance_matches_the_recorded_answers(fa, fixture, name):
    gx, gy = fa.griddistance_host(fixture["grid.%s.lon" % name], fixture["grid.%s.lat" % name])
    _check_grid(gx, fixture["grid.%s.gridDistX" % name].view(np.float32), "recorded %s X" % name)
    _check_grid(gy, fixture["grid.%s.gridDistY" % name].view(np.float32), "recorded %s Y" % name)


def test_grid_distance_of_one_point(fa, fixture):
    """Zeros and the reference's return code -1."""
    import ctypes
    import torch
    assert int(fixture["grid.g1x1.rc"]) == fa.ERROR and fixture["grid.g1x1.gridDistX"][0, 0] == 0
    lon, lat = np.array([10.0]), np.array([60.0])
    gx, gy = np.full(1, -1.0, np.float32), np.full(1, -1.0, np.float32)
    D, F = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    rc = fa.load().fimex_amd_griddistance_host(1, 1, lon.ctypes.data_as(D), lat.ctypes.data_as(D), gx.ctypes.data_as(F), gy.ctypes.data_as(F))
    assert rc == fa.ERROR and b"one point" in fa.load().fimex_amd_last_error()
    assert gx.view(np.uint32)[0] == 0 and gy.view(np.uint32)[0] == 0
    d = _dev(np.array([10.0, 60.0]), np.float64)
    out = torch.full((2,), -1.0, device="cuda")
    rc = fa.load().fimex_amd_griddistance_device(1, 1, d.data_ptr(), d.data_ptr() + 8, out.data_ptr(), out.data_ptr() + 4, _stream())
    torch.cuda.synchronize()
    assert rc == fa.ERROR and np.all(out.cpu().numpy().view(np.uint32) == 0)


# ------------------------------------------------------------------ omega
def _fa_levels(fa, lv, device=False):
    keep = []

    def big(v):
        if v is None or not device:
            return v
        t = _dev(v)
        keep.append(t)
        return t.data_ptr()
    out = fa.VerticalLevels(lv.kind, lv.nz, axis=lv.axis, sigma=lv.sigma, a=lv.a, ap=lv.ap, b=lv.b, p0=lv.p0, ptop=lv.ptop,
                            ps=big(lv.ps), field=big(lv.field))
    out._tensors = keep
    return out


def _check_omega(fa, lv, omega, t, want):
    import torch
    nt, nz, ny, nx = omega.shape
    host = fa.omega_to_vertical_wind_host(_fa_levels(fa, lv), nx, ny, nt, omega, t)
    assert cases.same(host, want), cases.describe_mismatch(host, want)
    dl = _fa_levels(fa, lv, device=True)
    d_omega, d_t = _dev(omega), _dev(t)
    out = torch.full(omega.shape, -7.0, dtype=torch.float32, device="cuda")
    fa.omega_to_vertical_wind_device(dl, nx, ny, nt, d_omega.data_ptr(), d_t.data_ptr(), out.data_ptr(), stream=_stream())
    fa.omega_to_vertical_wind_device(dl, nx, ny, nt, d_omega.data_ptr(), d_t.data_ptr(), d_omega.data_ptr(), stream=_stream())  # in place
    torch.cuda.synchronize()
    assert cases.same(out.cpu().numpy(), want) and cases.same(d_omega.cpu().numpy(), want)


@pytest.mark.parametrize("kind", vr.KINDS)
def test_omega_is_bit_identical(fa, fixture, kind):
    """Every level kind, host entry, device entry out of place and in place, with NaN and zero pressure among the cells; nx * ny above
    one workgroup and nz a group of four plus a remainder; then the recorded case of the kind."""
    nx, ny, nz, nt = 53, 7, 6, 2
    lv, omega, t = vv.make_omega_case(80 + kind, kind, nx, ny, nz, nt)
    p = vr.level_field(lv, nt, ny, nx)
    want = vv.omega_to_vertical_wind(omega, p, t)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).mean() > 0.5
    _check_omega(fa, lv, omega, t, want)
    c = {k.split(".", 2)[2]: v for k, v in fixture.items() if k.startswith("omega.kind%d." % kind)}
    lv = vr.Levels(int(c["kind"]), int(c["nz"]), p0=float(c["p0"]), ptop=float(c["ptop"]),
                   **{k: c[k] for k in ("axis", "sigma", "a", "ap", "b", "ps", "field") if k in c})
    _check_omega(fa, lv, c["omega"], c["t"], c["w"].view(np.float32))


# ------------------------------------------------------------------ arguments
def test_argument_errors(fa):
    import torch
    nx, ny, nz, nt = 8, 4, 3, 1
    vol = torch.zeros((nt, nz, ny, nx), dtype=torch.float32, device="cuda")
    out = torch.zeros_like(vol)
    pl = torch.full((nt, ny, nx), 100000.0, dtype=torch.float32, device="cuda")
    dbl = torch.zeros((2, ny, nx), dtype=torch.float64, device="cuda")
    ap, b = vv.hybrid_coefficients(nz)
    V, P, O, st = vol.data_ptr(), pl.data_ptr(), out.data_ptr(), _stream()

    def raises(match, fn, *a, **kw):
        with pytest.raises(fa.FimexAmdError, match=match):
            fn(*a, **kw)
    vel = fa.vertical_velocity_device
    raises("nx >= 3", vel, 2, ny, nt, 1000.0, 1000.0, P, P, ap, b, P, P, V, V, V, O)
    raises("ny >= 3", vel, nx, 2, nt, 1000.0, 1000.0, P, P, ap, b, P, P, V, V, V, O)
    raises("nz == 0", vel, nx, ny, nt, 1000.0, 1000.0, P, P, np.zeros(0), np.zeros(0), P, P, V, V, V, O)
    raises("grid distance", vel, nx, ny, nt, 1000.0, 1000.0, None, P, ap, b, P, P, V, V, V, O)
    raises("orography or surface pressure", vel, nx, ny, nt, 1000.0, 1000.0, P, P, ap, b, None, P, V, V, V, O)
    raises("orography or surface pressure", vel, nx, ny, nt, 1000.0, 1000.0, P, P, ap, b, P, None, V, V, V, O)
    raises("wind or temperature", vel, nx, ny, nt, 1000.0, 1000.0, P, P, ap, b, P, P, None, V, V, O)
    raises("wind or temperature", vel, nx, ny, nt, 1000.0, 1000.0, P, P, ap, b, P, P, V, V, None, O)
    raises("output", vel, nx, ny, nt, 1000.0, 1000.0, P, P, ap, b, P, P, V, V, V, None)
    raises("overlaps the air temperature", vel, nx, ny, nt, 1000.0, 1000.0, P, P, ap, b, P, P, V, V, O, O)
    assert fa.load().fimex_amd_vertical_velocity_device(nx, ny, nz, nt, 1000.0, 1000.0, P, P, None, None, P, P, V, V, V, O, st) == fa.ERROR
    assert b"NULL ap" in fa.load().fimex_amd_last_error()
    raises("nx >= 3", fa.vertical_velocity_host, 2, 3, 1, 1.0, 1.0, np.ones((3, 2)), np.ones((3, 2)), ap, b, np.ones((3, 2)), np.ones((1, 3, 2)),
           np.ones((1, nz, 3, 2)), np.ones((1, nz, 3, 2)), np.ones((1, nz, 3, 2)))
    grid = fa.griddistance_device
    raises("longitude or latitude", grid, nx, ny, None, dbl.data_ptr(), P, O)
    raises("output", grid, nx, ny, dbl.data_ptr(), dbl.data_ptr() + 8 * nx * ny, None, O)
    raises("empty grid", grid, 0, ny, dbl.data_ptr(), dbl.data_ptr(), P, O)
    raises("gridDistX overlaps gridDistY", grid, nx, ny, dbl.data_ptr(), dbl.data_ptr() + 8 * nx * ny, O, O + 4)
    axis = fa.VerticalLevels.from_axis(np.array([100.0, 500.0, 900.0]))
    om = fa.omega_to_vertical_wind_device
    raises("omega", om, axis, nx, ny, nt, None, V, O)
    raises("air temperature", om, axis, nx, ny, nt, V, None, O)
    raises("output", om, axis, nx, ny, nt, V, V, None)
    raises("overlaps omega", om, axis, nx, ny, nt, V, P, V + 4)
    raises("overlaps the air temperature", om, axis, nx, ny, nt, V, O, O)
    raises("nz == 0", om, fa.VerticalLevels.from_axis(np.zeros(0)), nx, ny, nt, V, V, O)
    raises("unknown vertical level kind", om, fa.VerticalLevels(9, nz), nx, ny, nt, V, V, O)
    raises("overlaps the level field", om, fa.VerticalLevels.from_field(O, nz), nx, ny, nt, V, V, O)
    # nothing to do is no error
    om(axis, 0, ny, nt, None, None, None)
    vel(nx, ny, 0, 1000.0, 1000.0, P, P, ap, b, None, None, None, None, None, None)
