"""Pins tests/vertical_ref.py (the yardstick of the GPU vertical interpolation) to the reference: its own known answers for
the two searches, the level formulas and the blends, and the vectorised forms against the per-cell ones.  CPU only."""
import numpy as np
import pytest

import cases
import vertical_ref as vr


ARY = [1, 2, 3, 4, 4, -1, -2, 5]


# test/testUtils.cc:84-105
@pytest.mark.parametrize("x, want", [(1.5, (0, 1)), (4, (3, 7)), (-1, (5, 6)), (-3, (6, 5)), (5, (7, 3))])
def test_find_closest_distinct_elements_kats(x, want):
    assert vr.find_closest_distinct_elements(ARY, x) == want


# test/testUtils.cc:107-126
@pytest.mark.parametrize("x, want", [(1.5, (0, 1)), (4, (3, 7)), (-1, (5, 0)), (-3, (6, 5)), (5, (7, 3))])
def test_find_closest_neighbor_distinct_elements_kats(x, want):
    assert vr.find_closest_neighbor_distinct_elements(ARY, x) == want


def test_search_degenerate_columns():
    assert vr.find_closest_neighbor_distinct_elements([], 1.0) == (0, 0)
    assert vr.find_closest_neighbor_distinct_elements([3.0], 1.0) == (0, 0)
    assert vr.find_closest_neighbor_distinct_elements([3.0], 3.0) == (0, 0)
    assert vr.find_closest_neighbor_distinct_elements([3.0, 3.0, 3.0], 5.0) == (0, 0)
    # x on the FIRST element: lowDiff == highDiff == 0 and nothing is strictly closer (Utils.h:262-283)
    assert vr.find_closest_neighbor_distinct_elements([1.0, 2.0, 3.0], 1.0) == (0, 0)
    assert vr.find_closest_neighbor_distinct_elements([1.0, 2.0, 3.0], 2.0) == (1, 2)


def _close_percent(got, want, percent):
    """BOOST_CHECK_CLOSE: both relative differences within `percent` %."""
    d = abs(got - want)
    return d <= percent / 100 * abs(got) and d <= percent / 100 * abs(want)


# test/testVerticalCoordinates.cc:34-55
def test_sigma_pressure_kat():
    sigma = [1., .9, .8, .7, .6, .5, .1]
    want = [1015., 913.5, 812., 710.5, 609., 507.5, 101.5]
    lv = vr.Levels(vr.SIGMA, 7, sigma=sigma, ptop=0., ps=np.full((1, 1, 1), 1015., np.float32))
    got = vr.level_field(lv, 1, 1, 1)[0, :, 0, 0]
    assert got.dtype == np.float32
    for g, w in zip(got, want):
        assert _close_percent(float(g), w, 1e-3)


# test/testVerticalCoordinates.cc:57-90
def test_hybrid_sigma_pressure_kats():
    a = np.array([1., 3., 5., 7., 9., 0.00098881774, 0.000996283525])
    b = np.array([0., 0., 0.00011835, 0.00057981, 0.00158568, 0.98881774, 0.996283525])
    want = [1000., 3000., 5000.12, 7000.588, 9001.609, 1004.639, 1012.224]
    ps = np.full((1, 1, 1), 1015., np.float32)
    for lv in (vr.Levels(vr.HYBRID_SIGMA, 7, a=a, b=b, p0=1000., ps=ps), vr.Levels(vr.HYBRID_SIGMA_AP, 7, ap=a * 1000., b=b, ps=ps)):
        got = vr.level_field(lv, 1, 1, 1)[0, :, 0, 0]
        for g, w in zip(got, want):
            assert _close_percent(float(g), w, 1e-3)


def test_axis_and_field_levels():
    ax = np.array([1000., 850.5, 1e-3])
    got = vr.level_field(vr.Levels(vr.AXIS, 3, axis=ax), 2, 3, 4)
    assert got.shape == (2, 3, 3, 4) and np.array_equal(got[1, :, 2, 3], ax.astype(np.float32))
    f = cases.field(6, 3, 4, seed=1).reshape(2, 3, 3, 4)
    assert cases.same(vr.level_field(vr.Levels(vr.FIELD, 3, field=f), 2, 3, 4), f)


def _two_level(method, levels, data, x):
    return float(vr.interpolate_cell(method, np.array(levels, np.float32), np.array(data, np.float32), x))


# test/testInterpolation.cc:212-262, reached through search + blend on a two-level column
def test_log_blend_kats_through_the_search():
    for x, w in ((500., 729.073), (200., 370.927), (800., 912.781)):
        assert abs(_two_level(vr.LOG, [1000., 100.], [1000., 100.], x) - w) / w < 1e-5
    # beyond the column the fallback search finds a second level only when the closest one is not the column's first
    # (Utils.h:214-218 starts with v2Diff = v1Diff): the extrapolating KAT needs the 1000 level second
    assert abs(_two_level(vr.LOG, [100., 1000.], [100., 1000.], 1500.) - 1158.482) / 1158.482 < 1e-5
    assert np.isnan(_two_level(vr.LOG, [1000., 100.], [1000., 100.], 1500.))
    for x, w in ((500., 763.1873), (200., 408.0904), (800., 926.384)):
        assert abs(_two_level(vr.LOGLOG, [1000., 100.], [1000., 100.], x) - w) / w < 1e-5
    # MIFI_ERROR (a non-positive coordinate) leaves the reference's element unset: NaN in this restatement
    assert np.isnan(_two_level(vr.LOG, [1000., 100.], [1000., 100.], -1.))
    assert np.isnan(_two_level(vr.LOGLOG, [0., 100.], [1000., 100.], 5.))


# test/testInterpolation.cc:685-731: in0 = 200 at a = 2, in1 = 300 at b = 3, x = 0.5 .. 4.5
def test_linear_family_kats_through_the_search():
    want = {vr.LIN_NO_EXTRA: (np.nan, np.nan, 250, np.nan, np.nan), vr.LIN_CONST_EXTRA: (200, 200, 250, 300, 300),
            vr.LIN_WEAK_EXTRA: (np.nan, 150, 250, 350, np.nan), vr.LIN: (50, 150, 250, 350, 450)}
    for method, expect in want.items():
        for x, w in zip((0.5, 1.5, 2.5, 3.5, 4.5), expect):
            # outside the column the closest level must not be the first one (see the log KATs above)
            out = _two_level(method, [3., 2.], [300., 200.], x) if x < 2 else _two_level(method, [2., 3.], [200., 300.], x)
            assert (np.isnan(out) and np.isnan(w)) or abs(out - w) < 0.01, (method, x, out, w)
    # between two levels the pair is (level <= x, level > x): "nearest" takes the lower one however close the upper is
    assert _two_level(vr.NN, [2., 3.], [200., 300.], 2.9) == 200.
    assert _two_level(vr.NN, [3., 2.], [300., 200.], 2.9) == 200.
    assert _two_level(vr.NN, [2., 3.], [200., 300.], 3.5) == 300.  # extrapolating: the closest one


def _random_columns(seed, nt, nzi, nzo, ny, nx, order):
    rng = np.random.default_rng(seed)
    base = np.sort(rng.uniform(1., 1000., nzi)) if order != "dec" else np.sort(rng.uniform(1., 1000., nzi))[::-1]
    ilev = (base[None, :, None, None] * (1 + 0.3 * rng.uniform(-1, 1, (nt, 1, ny, nx)))).astype(np.float32)
    if order in ("shuf", "rep", "nan"):
        ilev = rng.permuted(ilev, axis=1)
    if order == "rep" and nzi > 2:
        ilev[:, nzi // 2] = ilev[:, 0]
        ilev[:, -1] = ilev[:, 1]
    if order == "nan":
        ilev[rng.uniform(size=ilev.shape) < 0.2] = np.nan
        ilev[:, :, 0, 0] = np.nan
    x = rng.uniform(-100., 1500., (nt, nzo, ny, nx))
    pick = rng.integers(0, nzi, (nt, nzo, ny, nx))
    onlevel = rng.uniform(size=x.shape) < 0.3  # targets exactly on an input level, the first one included
    x = np.where(onlevel, np.take_along_axis(ilev, pick, axis=1).astype(np.float64), x)
    data = cases.field(nt * nzi, ny, nx, seed=seed + 1, nan_frac=0.05).reshape(nt, nzi, ny, nx)
    return data, ilev, x


@pytest.mark.parametrize("order", ["inc", "dec", "shuf", "rep", "nan"])
@pytest.mark.parametrize("nzi", [1, 2, 7, 19])
def test_vectorised_search_equals_the_sequential_one(order, nzi):
    data, ilev, x = _random_columns(11 + nzi, 2, nzi, 5, 4, 9, order)
    first, second = vr.search_pairs(ilev, x)
    for idx in np.ndindex(x.shape):
        t, k, j, i = idx
        assert (first[idx], second[idx]) == vr.find_closest_neighbor_distinct_elements(ilev[t, :, j, i], x[idx]), idx


@pytest.mark.parametrize("method", vr.METHODS)
@pytest.mark.parametrize("order", ["inc", "shuf", "rep", "nan"])
def test_vectorised_interpolation_equals_the_per_cell_form(method, order):
    nt, nzi, nzo, ny, nx = 2, 7, 4, 3, 8
    data, ilev, x = _random_columns(100 + method, nt, nzi, nzo, ny, nx, order)
    rng = np.random.default_rng(5)
    vmin, vmax = rng.uniform(-50, 200, (ny, nx)), rng.uniform(600, 1400, (ny, nx))
    for bounds in ((None, None), (vmin, None), (None, vmax), (vmin, vmax)):
        got = vr.interpolate(method, data, ilev, x, bounds[0], bounds[1], clampMin=275., clampMax=290.)
        want = np.empty_like(got)
        for idx in np.ndindex(x.shape):
            t, k, j, i = idx
            want[idx] = vr.interpolate_cell(method, ilev[t, :, j, i], data[t, :, j, i], x[idx],
                                            None if bounds[0] is None else bounds[0][j, i], None if bounds[1] is None else bounds[1][j, i])
        want = vr.clamp(want, 275., 290.)
        assert cases.same(got, want), cases.describe_mismatch(got, want)


def test_clamp_keeps_nan_and_ignores_nan_bounds():
    v = np.array([1., 5., np.nan, 9.], np.float32)
    assert cases.same(vr.clamp(v, 2., 8.), np.array([2., 5., np.nan, 8.], np.float32))
    assert cases.same(vr.clamp(v, np.nan, 8.), np.array([1., 5., np.nan, 8.], np.float32))
    assert cases.same(vr.clamp(v, np.nan, np.nan), v)
