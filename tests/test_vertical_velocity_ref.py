"""tests/vertical_velocity_ref.py, the CPU yardstick of the vertical velocity on model levels, against the reference's own object code
(oracle/_ref/libmifi_ref.so, where build() found a reference tree to compile it from) and against its recorded answers
(tests/golden/vertical_velocity_answers.npz, scripts/record_vertical_velocity_answers.py).  w and omega are compared bit for bit, NaN
positions included; the grid distance within vertical_velocity_ref.griddistance_tolerance, because numpy's sin / cos / arccos need
not be the C library's.  CPU only.
"""
import numpy as np
import pytest

import vertical_ref as vr
import vertical_velocity_ref as vv


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """float32 arrays: identical NaN positions, identical bits elsewhere."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    n = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), n) and np.array_equal(_bits(got)[~n], _bits(want)[~n])


def _check_grid(got, want, label):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert not np.isnan(want).any() and not np.isnan(got).any(), label
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.all((err <= vv.griddistance_tolerance(want)) | (got == want)), "%s: worst error %g" % (label, err.max())
    print("grid distance %s: %.2f %% bit-identical" % (label, 100.0 * np.mean(_bits(got) == _bits(want))))


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return vv.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def live():
    ref = vv.reference_lib()
    if ref is None:
        pytest.skip("oracle/_ref/libmifi_ref.so is absent: build() found no reference tree to compile it from")
    return ref


# ------------------------------------------------------------------ the recorded answers
def test_fixture_holds_the_cases(fixture):
    for name, nx, ny in vv.RECORDED_GRIDS:
        assert fixture["grid.%s.lon" % name].shape == (ny, nx)
        assert int(fixture["grid.%s.rc" % name]) == (vv.ERROR if nx * ny == 1 else vv.OK)
    for name, nx, ny, nz, nan_frac in vv.RECORDED_VELOCITY:
        w = fixture["velocity.%s.w" % name].view(np.float32)
        assert w.shape == (1, nz, ny, nx) and w.dtype == np.float32
        assert np.all(_bits(w[:, 0]) == 0), "w at level 0 is +0"
        assert np.isnan(w).any() == bool(nan_frac) and np.isfinite(w).mean() >= 0.5
    for kind in vr.KINDS:
        w = fixture["omega.kind%d.w" % kind].view(np.float32)
        assert np.isnan(w).any() and np.isinf(w).any() and np.isfinite(w).mean() > 0.5


def test_the_last_row_rule_is_not_the_row_above(fixture):
    """g[p] = g[p - ny]: on 13 x 4 the last row repeats its own first four cells (a chain of three), which the rule p - nx would
    not give."""
    gx = fixture["grid.g13x4.gridDistX"].view(np.float32)
    assert np.array_equal(gx[3, 4:8], gx[3, 0:4]) and np.array_equal(gx[3, 8:12], gx[3, 0:4]) and gx[3, 12] == gx[3, 0]
    assert np.array_equal(gx[3, 0:4], gx[2, 9:13]) and not np.array_equal(gx[3], gx[2])
    gy = fixture["grid.g5x7.gridDistY"].view(np.float32)  # ny > nx: the sources lie one and two rows up
    assert np.array_equal(gy[6], gy.reshape(-1)[30 - 7:35 - 7])


@pytest.mark.parametrize("name", [g[0] for g in vv.RECORDED_GRIDS])
def test_recorded_grid_distance(fixture, name):
    gx, gy, rc = vv.griddistance(fixture["grid.%s.lon" % name], fixture["grid.%s.lat" % name])
    assert rc == int(fixture["grid.%s.rc" % name])
    _check_grid(gx, fixture["grid.%s.gridDistX" % name].view(np.float32), name + " X")
    _check_grid(gy, fixture["grid.%s.gridDistY" % name].view(np.float32), name + " Y")


@pytest.mark.parametrize("name", [c[0] for c in vv.RECORDED_VELOCITY])
def test_recorded_vertical_velocity(fixture, name):
    w, M = vv.vertical_velocity(*[fixture["velocity.%s.%s" % (name, k)] for k in vv.VELOCITY_ARGS])
    want = fixture["velocity.%s.w" % name].view(np.float32)
    assert _same(w, want)
    assert M.shape == w.shape and np.all(M[np.isfinite(want)] >= np.abs(want[np.isfinite(want)]) * (1 - 1e-6))


@pytest.mark.parametrize("kind", vr.KINDS)
def test_recorded_omega(fixture, kind):
    c = {k.split(".", 2)[2]: v for k, v in fixture.items() if k.startswith("omega.kind%d." % kind)}
    lv = vr.Levels(int(c["kind"]), int(c["nz"]), p0=float(c["p0"]), ptop=float(c["ptop"]),
                   **{k: c[k] for k in ("axis", "sigma", "a", "ap", "b", "ps", "field") if k in c})
    nt, nz, ny, nx = c["omega"].shape
    p = vr.level_field(lv, nt, ny, nx)
    assert np.array_equal(_bits(p), _bits(c["p"]))
    assert _same(vv.omega_to_vertical_wind(c["omega"], p, c["t"]), c["w"].view(np.float32))


# ------------------------------------------------------------------ the live library
def test_live_library_gives_the_recorded_answers(live, fixture):
    for name, _, _ in vv.RECORDED_GRIDS:
        gx, gy, rc = live.griddistance(fixture["grid.%s.lon" % name], fixture["grid.%s.lat" % name])
        assert rc == int(fixture["grid.%s.rc" % name])
        assert np.array_equal(_bits(gx), fixture["grid.%s.gridDistX" % name]) and np.array_equal(_bits(gy), fixture["grid.%s.gridDistY" % name])
    for name in [c[0] for c in vv.RECORDED_VELOCITY]:
        w = live.vertical_velocity(*[fixture["velocity.%s.%s" % (name, k)] for k in vv.VELOCITY_ARGS])
        assert _same(w, fixture["velocity.%s.w" % name].view(np.float32)), name
    for kind in vr.KINDS:
        n = "omega.kind%d." % kind
        assert _same(live.omega_to_vertical_wind(fixture[n + "omega"], fixture[n + "p"], fixture[n + "t"]), fixture[n + "w"].view(np.float32))


@pytest.mark.parametrize("shape", [(7, 5, 4, 1, 0.0), (5, 7, 4, 2, 0.0), (3, 3, 2, 1, 0.0), (3, 9, 1, 1, 0.0), (67, 35, 9, 1, 0.0),
                                   (67, 35, 9, 2, 0.01), (130, 70, 65, 1, 0.0), (40, 30, 137, 1, 0.0)],
                         ids=lambda s: "%dx%dx%d" % s[:3] + ("nan" if s[4] else ""))
def test_vertical_velocity_against_the_live_library(live, shape):
    nx, ny, nz, nt, nan_frac = shape
    c = vv.make_case(nx + nz, nx, ny, nz, nt, nan_frac)
    w, _ = vv.vertical_velocity(*vv.velocity_args(c))
    want = live.vertical_velocity(*vv.velocity_args(c))
    assert _same(w, want)
    assert np.isnan(want).any() == bool(nan_frac) and np.isfinite(want).mean() >= 0.5


def test_non_positive_pressure_against_the_live_library(live):
    """A negative ap makes pm <= 0 in part of the columns: whatever IEEE arithmetic gives, in the same cells."""
    c = vv.make_case(77, 9, 7, 5, 1)
    c["ap"] = c["ap"].copy()
    c["ap"][2] = -60000.0
    want = live.vertical_velocity(*vv.velocity_args(c))
    assert np.isnan(want).any()
    assert _same(vv.vertical_velocity(*vv.velocity_args(c))[0], want)


@pytest.mark.parametrize("shape", [(7, 5), (5, 7), (13, 4), (67, 35), (3, 3), (1, 9), (9, 1), (2, 2), (1, 1)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("lat0", [0.5, 60.0, 89.0])
def test_grid_distance_against_the_live_library(live, shape, lat0):
    nx, ny = shape
    lon, lat = vv.make_grid(nx * 100 + ny, nx, ny, lat0=lat0)
    gx, gy, rc = vv.griddistance(lon, lat)
    wx, wy, wrc = live.griddistance(lon, lat)
    assert rc == wrc == (vv.ERROR if nx * ny == 1 else vv.OK)
    _check_grid(gx, wx, "%dx%d X" % shape)
    _check_grid(gy, wy, "%dx%d Y" % shape)


@pytest.mark.parametrize("kind", vr.KINDS)
def test_omega_against_the_live_library(live, kind):
    nx, ny, nz, nt = 9, 6, 7, 2
    lv, omega, t = vv.make_omega_case(kind, kind, nx, ny, nz, nt)
    p = vr.level_field(lv, nt, ny, nx)
    assert np.count_nonzero(p == 0) >= 2
    assert _same(vv.omega_to_vertical_wind(omega, p, t), live.omega_to_vertical_wind(omega, p, t))
