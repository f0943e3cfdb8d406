"""The CPU oracle against the reference's own C code, function by function.  CPU only.

oracle.ref() is oracle/_ref/libmifi_ref.so: the reference's src/interpolation.c and src/vertical_coordinate_transformations.c,
compiled unmodified (recipe: oracle/Makefile, oracle/ref_shim).  Every live test below calls the oracle's function and the
reference's on identical inputs and asks for identical bits: cases.same on floats (bit-identical defined values, the same NaN
positions), the same on the bit patterns of doubles, equal return codes, equal nChanged.  Both sides run on the host with the
same libm, so there is no tolerance anywhere; a differing bit is a misread operation order in the restatement.

Inputs the reference cannot take are kept from it by predicates computed from the inputs alone (never from an output).  They
are the oracle's documented divergences, each an out-of-bounds read or undefined behaviour in the reference:
  D1  bilinear, nearest/nearest corner with lround(y) == iy (src/interpolation.c:936 reads one row past the slice)
  D2  a position that is not finite or has |coordinate| >= 2^30 (cast to int)
  D5  a fill on a slice with nx < 2 or ny < 2 and something to fill
  D7  a rotation matrix on a mesh whose second delta probe, cell (ox/2 + 1, oy/2 + 1), is past the mesh: oy == 2, or ox == 2
      with oy <= 4 (src/interpolation.c:469 reads in_x_field beyond its end).  Found by this file.
For each the test asserts what the oracle returns instead.  Two more inputs are never built here because oracle and reference
alike read past the axis: mifi_points2position on an axis of one point.

The live tests skip when oracle/_ref/libmifi_ref.so is absent (no reference tree was at hand at build time), and for no other
reason.  test_recorded_answers never skips: it replays tests/golden/reference_answers.npz, answers recorded from the same
library by scripts/record_reference_answers.py, through the oracle.
"""
import functools
import os

import numpy as np
import pytest

import cases
import oracle
from oracle import proj_oracle as po

_REF_FILE = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), "_ref", "libmifi_ref.so")


@pytest.fixture(scope="module")
def ref():
    r = oracle.ref()
    if r is None:
        pytest.skip("%s is absent: build() found no reference tree to compile it from" % _REF_FILE)
    return r


def same64(a, b):
    """bit-identical defined doubles, identical NaN positions."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def describe64(a, b, limit=5):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    idx = np.nonzero((na != nb) | (~na & ~nb & (a.view(np.uint64) != b.view(np.uint64))))[0]
    return "%d of %d differ; first: %s" % (idx.size, a.size, [(int(i), float(a[i]), float(b[i])) for i in idx[:limit]])


# ---------------------------------------------------------------- the predicates of D1 and D2, from the positions alone
def lround(x):
    """C lround on finite doubles: half away from zero (x - trunc(x) is exact)."""
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0.0)


def d2_mask(px, py):
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(px) & np.isfinite(py) & (np.abs(px) < 2.0 ** 30) & (np.abs(py) < 2.0 ** 30))


def d1_mask(px, py, ix, iy):
    """x outside the linear range [0, ix-1) with 0 <= lround(x) < ix, y outside the linear range and lround(y) == iy."""
    ok = ~d2_mask(px, py)
    x, y = np.where(ok, px, 0.0), np.where(ok, py, 0.0)
    xlin = (0 <= np.floor(x)) & (np.floor(x) + 1 < ix)
    ylin = (0 <= np.floor(y)) & (np.floor(y) + 1 < iy)
    rx = lround(x)
    return ok & ~xlin & (0 <= rx) & (rx < ix) & ~ylin & (lround(y) == iy)


def skip_mask(method, px, py, ix, iy):
    m = d2_mask(px, py)
    return (m | d1_mask(px, py, ix, iy)) if method == oracle.BILINEAR else m


D1_CAP = 0.05

SOURCES = [(1, 1), (1, 29), (37, 1), (2, 2), (3, 2), (4, 4), (37, 29), (300, 200)]
OUT = (57, 43)


def _positions(inX, inY, method):
    """cases.backward_positions with the special coordinates.  The D1 zone is at most two strips of half a cell in x times
    one cell in y, whatever the source's size, while the list spans (n - 1 + 2 * overshoot) * 1.05 cells per side: around a
    source of one to three cells the default overshoot of 2 leaves a square of 4.2 cells, of which that zone is 1 / 17.6, above
    the cap by geometry alone.  Such sources get an overshoot of 4 (the zone is then 1 / 70 of the list at most)."""
    overshoot = 4.0 if min(inX, inY) < 4 else 2.0
    return cases.backward_positions(inX, inY, OUT[0], OUT[1], seed=100 * inX + inY + method, overshoot=overshoot, special=True)


# ---------------------------------------------------------------- mifi_get_values_f / _bilinear_f / _bicubic_f
@pytest.mark.parametrize("nz", [1, 3])
@pytest.mark.parametrize("source", SOURCES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR, oracle.BICUBIC], ids=["nearest", "bilinear", "bicubic"])
def test_point_functions(ref, capsys, method, source, nz):
    inX, inY = source
    outX, outY = OUT
    px, py = _positions(inX, inY, method)
    f = cases.field(nz, inY, inX, seed=7 + method + inX, extremes=True)
    d1 = d1_mask(px, py, inX, inY) if method == oracle.BILINEAR else np.zeros(px.size, bool)
    skip = skip_mask(method, px, py, inX, inY)
    if method == oracle.BILINEAR:
        with capsys.disabled():  # shown on every run, also when the test passes
            print("\nbilinear %dx%d nz %d: %.2f %% of %d points excluded as D1 (cap %.0f %%), %.2f %% as D2 " % (
                inX, inY, nz, 100.0 * d1.mean(), px.size, 100.0 * D1_CAP, 100.0 * d2_mask(px, py).mean()), end="")
        assert d1.mean() <= D1_CAP
    assert d2_mask(px, py).sum() >= 9  # the special coordinates are in the case
    got = oracle.interpolate_values(method, px, py, f, inX, inY, outX, outY).reshape(nz, -1)
    want, rc = ref.interpolate_values(method, px, py, f, inX, inY, skip)
    assert rc == oracle.OK
    assert np.all(np.isnan(got[:, skip]))  # what the oracle returns where the reference cannot be asked
    assert cases.same(got[:, ~skip], want[:, ~skip]), cases.describe_mismatch(got[:, ~skip], want[:, ~skip])
    # the per-point entry, its return code included
    for i in np.nonzero(~skip)[0][:: max(1, px.size // 40)]:
        w, wrc = ref.get_values(method, f, px[i], py[i], inX, inY, nz)
        g = np.empty(nz, np.float32)
        grc = getattr(oracle.lib(), oracle._POINT[method])(oracle._f(oracle._c32(f).ravel()), oracle._f(g), px[i], py[i], inX, inY, nz)
        assert grc == wrc and cases.same(g, w)


def test_skip_mask_removes_exactly_d1_and_d2():
    """The mask over the full special position list is the union of the two predicates, written out here a second time in
    scalar form, and nothing else: it cannot grow silently."""
    import math
    for method in (oracle.NEAREST, oracle.BILINEAR, oracle.BICUBIC):
        for inX, inY in SOURCES:
            px, py = _positions(inX, inY, method)
            mask = skip_mask(method, px, py, inX, inY)
            expect = np.zeros(px.size, bool)
            for i, (x, y) in enumerate(zip(px.tolist(), py.tolist())):
                if not (math.isfinite(x) and math.isfinite(y) and abs(x) < 2 ** 30 and abs(y) < 2 ** 30):
                    expect[i] = True  # D2
                    continue
                if method != oracle.BILINEAR:
                    continue
                c_lround = lambda v: int(math.floor(abs(v) + 0.5) * (1 if v >= 0 else -1)) if abs(v) < 2 ** 30 else 0
                xlin = 0 <= math.floor(x) and math.floor(x) + 1 < inX
                ylin = 0 <= math.floor(y) and math.floor(y) + 1 < inY
                expect[i] = (not xlin) and 0 <= c_lround(x) < inX and (not ylin) and c_lround(y) == inY  # D1
            assert np.array_equal(mask, expect), (method, inX, inY)
            assert not np.any(d1_mask(px, py, inX, inY) & d2_mask(px, py))
            n_special = int(np.sum(~np.isfinite(px) | ~np.isfinite(py) | (np.abs(np.nan_to_num(px)) >= 2.0 ** 30) | (np.abs(np.nan_to_num(py)) >= 2.0 ** 30)))
            assert d2_mask(px, py).sum() == n_special <= 2 * len(cases.SPECIAL)


# ---------------------------------------------------------------- fills
FILL_SHAPES = [(40, 30, 3), (97, 61, 2), (2, 2, 1), (3, 17, 1), (130, 5, 2), (4, 4, 1), (5, 70, 1), (300, 200, 2),
               (64, 66, 1), (33, 1200, 1), (1000, 131, 1), (5000, 1100, 1)]  # test_gpu_parity.test_fill2d_matches_oracle
FILL_PARAMS = [(4.0, 1.6, 100), (0.5, 1.0, 23), (4.0, 1.9, 3), (1e-9, 1.6, 41)]


@functools.lru_cache(maxsize=4)
def _holes(nz, ny, nx, seed):
    return cases.holes(nz, ny, nx, seed=seed)


def _same_fill(got, want, label):
    (ga, gn, grc), (wa, wn, wrc) = got, want
    assert grc == wrc, label
    assert gn == wn, label
    assert cases.same(ga, wa), "%s: %s" % (label, cases.describe_mismatch(ga, wa))


@pytest.mark.parametrize("params", FILL_PARAMS)
@pytest.mark.parametrize("shape", FILL_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_fill2d(ref, shape, params):
    nx, ny, nz = shape
    f = _holes(nz, ny, nx, nx * 31 + ny)
    for z in range(nz):
        _same_fill(oracle.fill2d(f[z], *params), ref.fill2d(f[z], *params), "slice %d" % z)


def _fill_edge_fields():
    """name -> [ny][nx] slice: no NaN, all NaN, one defined cell, NaN only on the rim, nx / ny of 2 and 3."""
    base = cases.holes(1, 23, 31, seed=77)[0]
    out = {"holes": base}
    full = cases.field(1, 23, 31, seed=78, nan_frac=0.0, extremes=False)[0]
    out["no_nan"] = full
    out["all_nan"] = np.full((23, 31), np.nan, np.float32)
    one = np.full((23, 31), np.nan, np.float32)
    one[11, 17] = 281.5
    out["one_defined"] = one
    rim = full.copy()
    rim[0, :] = rim[-1, :] = np.nan
    rim[:, 0] = rim[:, -1] = np.nan
    out["nan_rim"] = rim
    for ny, nx in ((2, 2), (2, 3), (3, 2), (3, 3), (2, 40), (40, 2), (3, 40), (40, 3)):
        g = cases.field(1, ny, nx, seed=80 + nx * 50 + ny, nan_frac=0.0, extremes=False)[0]
        g.reshape(-1)[:: 3] = np.nan
        out["%dx%d" % (nx, ny)] = g
    return out


# relaxCrit never met (maxLoop ends the loop) / met in the first sweep; maxLoop 0 and 1
FILL_EDGE_PARAMS = [(4.0, 1.6, 0), (4.0, 1.6, 1), (0.0, 1.6, 37), (-1.0, 1.9, 12), (1e30, 1.6, 100), (4.0, 1.6, 100)]


@pytest.mark.parametrize("params", FILL_EDGE_PARAMS)
def test_fill2d_edges(ref, params):
    for name, f in _fill_edge_fields().items():
        _same_fill(oracle.fill2d(f, *params), ref.fill2d(f, *params), name)


CREEP_PARAMS = [(20, 2), (1, 1), (5, 2), (3, 0), (2, 7), (0, 2), (0, 0), (1, 0), (2, -1), (1, -3)]  # (repeat, setWeight)


@pytest.mark.parametrize("params", CREEP_PARAMS)
@pytest.mark.parametrize("shape", FILL_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_creepfills(ref, shape, params):
    """Shapes and parameters of test_gpu_parity.test_creepfill_matches_oracle, plus repeat 0, weight 0 and negative weights
    (the char argument: it wraps in the reference's size_t sum, src/interpolation.c:1445)."""
    nx, ny, nz = shape
    repeat, weight = params
    f = _holes(nz, ny, nx, nx * 17 + ny)
    for z in range(nz):
        _same_fill(oracle.creepfill2d(f[z], repeat, weight), ref.creepfill2d(f[z], repeat, weight), "slice %d" % z)
        _same_fill(oracle.creepfillval2d(f[z], 271.25, repeat, weight), ref.creepfillval2d(f[z], 271.25, repeat, weight), "val, slice %d" % z)


@pytest.mark.parametrize("default", [np.nan, np.inf, -np.inf, 0.0, -0.0])
@pytest.mark.parametrize("params", [(20, 2), (0, 1), (1, 0), (3, 7), (2, -1)])
def test_creepfillval_default_values_and_edges(ref, params, default):
    repeat, weight = params
    for name, f in _fill_edge_fields().items():
        _same_fill(oracle.creepfillval2d(f, default, repeat, weight), ref.creepfillval2d(f, default, repeat, weight), name)
        _same_fill(oracle.creepfill2d(f, repeat, weight), ref.creepfill2d(f, repeat, weight), name)


def d5(f):
    """D5 from the slice alone: thinner than two cells, and both defined and undefined cells in it."""
    ny, nx = f.shape
    n = int(np.isnan(f).sum())
    return (nx < 2 or ny < 2) and 0 < n < f.size


def _thin_slices():
    out = []
    for ny, nx in ((1, 1), (1, 7), (7, 1)):
        full = cases.field(1, ny, nx, seed=3, nan_frac=0.0, extremes=False)[0]
        some = full.copy()
        some.reshape(-1)[::3] = np.nan
        out += [full, some, np.full((ny, nx), np.nan, np.float32)]
    return out


def test_fills_on_slices_thinner_than_two_d5():
    """D5: with nx < 2 or ny < 2 and something to fill the reference reads out of bounds; it is never called.  The oracle
    returns ORC_ERROR and leaves the slice alone.  (Needs no reference.)"""
    hit = [f for f in _thin_slices() if d5(f)]
    assert len(hit) == 2  # 1x1 has either nothing defined or nothing undefined
    for f in hit:
        for a, n, rc in (oracle.fill2d(f, 4.0, 1.6, 10), oracle.creepfill2d(f, 3, 2), oracle.creepfillval2d(f, 1.0, 3, 2)):
            assert rc == oracle.ERROR and cases.same(a, f) and n == int(np.isnan(f).sum())


def test_fills_on_thin_slices_with_nothing_to_fill(ref):
    """Complete or empty thin slices return before the reference touches a neighbour: those are compared."""
    safe = [f for f in _thin_slices() if not d5(f)]
    assert len(safe) == 7
    for f in safe:
        _same_fill(oracle.fill2d(f, 4.0, 1.6, 10), ref.fill2d(f, 4.0, 1.6, 10), str(f.shape))
        _same_fill(oracle.creepfill2d(f, 3, 2), ref.creepfill2d(f, 3, 2), str(f.shape))
        _same_fill(oracle.creepfillval2d(f, 1.0, 3, 2), ref.creepfillval2d(f, 1.0, 3, 2), str(f.shape))


# ---------------------------------------------------------------- rotations by a known matrix
@pytest.mark.parametrize("shape", [(64, 48, 4), (101, 37, 1), (7, 5, 4), (2000, 3, 1), (1, 1, 1)])
def test_rotation_by_matrix(ref, shape):
    ox, oy, oz = shape
    m = cases.rotation_matrix(ox, oy, seed=ox)
    assert ox * oy < 17 or np.abs(m.reshape(-1, 4)[:, 3]).max() > np.pi  # angles beyond +-pi
    u = cases.field(oz, oy, ox, seed=1, extremes=True)
    v = cases.field(oz, oy, ox, seed=2, extremes=True) - 280
    if u.size >= 6:
        u.reshape(-1)[[1, 3]] = np.nan, np.inf
        v.reshape(-1)[[2, 3, 5]] = np.nan, -np.inf, np.inf
    mm, uu, vv = oracle._c64(m), oracle._c32(u).copy().ravel(), oracle._c32(v).copy().ravel()
    grc = oracle.lib().orc_vector_reproject_values_by_matrix_f(oracle._d(mm), oracle._f(uu), oracle._f(vv), ox, oy, oz)
    wu, wv, wrc = ref.vector_reproject_values(m, u, v, ox, oy)
    assert grc == wrc
    assert cases.same(uu, wu.ravel()), cases.describe_mismatch(uu, wu)
    assert cases.same(vv, wv.ravel()), cases.describe_mismatch(vv, wv)
    gu, gv = oracle.vector_reproject_values(m, u, v, ox, oy)
    assert cases.same(gu, wu) and cases.same(gv, wv)
    ang = (np.random.default_rng(3).uniform(-400, 800, (oz, oy, ox))).astype(np.float32)
    if ang.size >= 6:
        ang.reshape(-1)[[0, 2, 4, 5]] = np.nan, np.inf, 0.0, 360.0
    aa = ang.copy().ravel()
    grc = oracle.lib().orc_vector_reproject_direction_by_matrix_f(oracle._d(mm), oracle._f(aa), ox, oy, oz)
    wa, wrc = ref.vector_reproject_direction(m, ang, ox, oy)
    assert grc == wrc
    assert cases.same(aa, wa.ravel()), cases.describe_mismatch(aa, wa)
    assert cases.same(oracle.vector_reproject_direction(m, ang, ox, oy), wa)


# ---------------------------------------------------------------- mifi_points2position
def _axes():
    r = np.radians
    return [("asc", np.linspace(-5, 5, 41), oracle.PROJ_AXIS), ("desc", np.linspace(9, -3, 25), oracle.PROJ_AXIS),
            ("one_cell", np.array([2.0, 3.5]), oracle.PROJ_AXIS), ("one_cell_desc", np.array([1.0, -1.0]), oracle.PROJ_AXIS),
            ("uneven", np.array([1., 2., 4., 8., 16., 17.]), oracle.PROJ_AXIS),
            ("lon_-180_180", r(np.arange(-180, 180, 1.0)), oracle.LONGITUDE), ("lon_0_360", r(np.arange(0, 360, 0.5)), oracle.LONGITUDE),
            ("lon_desc", r(np.arange(180, -180, -1.0)), oracle.LONGITUDE), ("lon_0_360_desc", r(np.arange(359.5, -0.25, -0.5)), oracle.LONGITUDE),
            ("lon_regional", r(np.linspace(-30, 45, 76)), oracle.LONGITUDE), ("lon_regional_east", r(np.linspace(150, 200, 51)), oracle.LONGITUDE),
            ("lon_one_cell", r(np.array([10.0, 11.0])), oracle.LONGITUDE), ("lon_two_halves", r(np.array([0.0, 180.0])), oracle.LONGITUDE),
            ("lat_desc", r(np.linspace(80, -80, 321)), oracle.LATITUDE), ("lat_asc", r(np.linspace(-90, 90, 181)), oracle.LATITUDE),
            ("lat_one_cell", r(np.array([60.0, 59.0])), oracle.LATITUDE)]


@pytest.mark.parametrize("case", _axes(), ids=lambda c: c[0])
def test_points2position(ref, case):
    _, axis, typ = case
    rng = np.random.default_rng(axis.size)
    p = rng.uniform(-8, 8, 3000)
    p[::97] = axis[rng.integers(0, axis.size, p[::97].size)]  # exact hits
    mid = 0.5 * (axis[:-1] + axis[1:])
    p[1:1 + min(mid.size, 50)] = mid[:50]
    ends = np.array([axis[0], axis[-1], np.nextafter(axis[0], 9), np.nextafter(axis[0], -9), np.nextafter(axis[-1], 9), np.nextafter(axis[-1], -9),
                     np.pi, -np.pi, np.nextafter(np.pi, 9), np.nextafter(-np.pi, -9), 2 * np.pi, -2 * np.pi, 0.0, -0.0, 3 * np.pi, -3 * np.pi,
                     axis[0] + 2 * np.pi, axis[-1] - 2 * np.pi, axis[0] - 2 * np.pi, axis[-1] + 2 * np.pi,
                     np.nan, np.inf, -np.inf, 1e300, -1e300])
    p[100:100 + ends.size] = ends
    got = oracle.points2position(p, axis, typ)
    grc = oracle.lib().orc_points2position(oracle._d(p.copy()), p.size, oracle._d(oracle._c64(axis)), axis.size, typ)
    want, wrc = ref.points2position(p, axis, typ)
    assert grc == wrc
    assert same64(got, want), describe64(got, want)
    assert np.all(got[100 + ends.size - 5:100 + ends.size - 2] == -999.0)


# ---------------------------------------------------------------- the 1-D blends between two fields
ABX = [(1., 2., 1.5), (1., 1., .5), (0., 1., 2.), (0., 1., 1.), (0., 1., 0.), (0., 1., -.5), (0., 1., -1.5), (0., 1., 2.5),
       (1000., 100., 500.), (1000., 100., 1500.), (1000., 100., 100.), (3., 7., 3.0000001),  # test_blends_between_two_fields_match_oracle
       (2., 2., 2.), (2., 2., 3.), (5., 5., 1.), (0., 0., 0.), (-3., -3., 1.),  # a == b
       (0., 1., 2.), (1., 0., 2.), (1., 2., 0.), (-1., 2., 3.), (1., -2., 3.), (1., 2., -3.), (-1., -2., -3.), (1., 1., 1.),  # log: non-positive
       (np.e, 1., 2.), (1., np.e, .5), (1e-300, 1e300, 1.), (2., 3., np.nan), (np.nan, 3., 2.), (2., np.inf, 3.)]


@pytest.mark.parametrize("abx", ABX, ids=lambda t: "a%g_b%g_x%g" % t)
@pytest.mark.parametrize("kind", range(7), ids=[n[len("mifi_get_values_"):-2] for n in __import__("oracle.reference", fromlist=["BLENDS"]).BLENDS])
def test_blends(ref, kind, abx):
    """Return code and, where the function refuses (log of a non-positive coordinate), an untouched output: both fronts
    prefill the output with the same sentinel."""
    a, b, x = abx
    A = cases.field(1, 37, 53, seed=kind + 1, nan_frac=0.05)[0]
    B = cases.field(1, 37, 53, seed=kind + 50, nan_frac=0.05)[0]
    got, grc = oracle.get_values_1d(kind, A, B, a, b, x)
    want, wrc = ref.get_values_1d(kind, A, B, a, b, x)
    assert grc == wrc
    assert cases.same(got, want), cases.describe_mismatch(got, want)
    if grc != oracle.OK:
        assert np.all(got == np.float32(-12345.0))


@pytest.mark.parametrize("abx", ABX, ids=lambda t: "a%g_b%g_x%g" % t)
def test_linear_blend_of_doubles(ref, abx):
    a, b, x = abx
    rng = np.random.default_rng(11)
    A, B = rng.normal(0, 5, 2001), rng.normal(3, 5, 2001)
    A[[1, 5, 9]] = np.nan, np.inf, -0.0
    B[[2, 5, 10]] = np.nan, -np.inf, 5e-324
    out = np.full(A.shape, -12345.0)
    grc = oracle.lib().orc_get_values_linear_d(oracle._d(A), oracle._d(B), oracle._d(out), A.size, a, b, x)
    want, wrc = ref.get_values_linear_d(A, B, a, b, x)
    assert grc == wrc
    assert same64(out, want), describe64(out, want)


# ---------------------------------------------------------------- fill value <-> NaN
@pytest.mark.parametrize("bad", [np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-42, 9.96921e36, -32767.0, 1e-45])
def test_bad2nan_nan2bad(ref, bad):
    rng = np.random.default_rng(0)
    a = rng.normal(0, 1, 10007).astype(np.float32)
    for k, v in enumerate((9.96921e36, -32767.0, np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-42, -1e-42, 1e-45)):
        a[rng.choice(a.size, 50, replace=False)] = np.float32(v)
    b = np.float32(bad)
    for n in (a.size, 1, 0):
        g, (w, wret) = oracle.bad2nan(a[:n], b), ref.bad2nan(a[:n], b)
        tmp = a[:1].copy()
        gret = oracle.lib().orc_bad2nanf(oracle._f(tmp), oracle._f(tmp), b)  # an empty range: only the return value
        assert gret == wret == 0
        assert cases.same(g, w), cases.describe_mismatch(g, w)
        g2, (w2, wret) = oracle.nan2bad(a[:n], b), ref.nan2bad(a[:n], b)
        assert wret == 0
        # the written fill value is compared by its bits as well: -0.0 and a denormal must arrive as they are
        assert cases.same(g2, w2) and np.array_equal(np.isnan(g2) | (g2.view(np.uint32) == w2.view(np.uint32)), np.ones(g2.shape, bool))


# ---------------------------------------------------------------- functions around the five PROJ.4 calls
GEO = "+proj=latlong +R=6371000"
STERE = "+proj=stere +lat_0=90 +lon_0=0 +lat_ts=60 +a=6371000 +e=0"
STERE_OBL = "+proj=stere +lat_0=52 +lon_0=10 +R=6371000 +x_0=1000 +y_0=-2000"
LCC = "+proj=lcc +lat_0=63 +lon_0=15 +lat_1=63 +lat_2=63 +no_defs +R=6.371e+06"
ROT = "+proj=ob_tran +o_proj=longlat +lon_0=-40 +o_lat_p=22 +R=6.371e+06 +no_defs"
POLAR0 = "+ellps=sphere +a=127.4 +e=0 +proj=stere +lat_0=90 +lon_0=0 +lat_ts=60"
POLAR90 = "+ellps=sphere +a=127.4 +e=0 +proj=stere +lat_0=90 +lon_0=90 +lat_ts=60"

# the pairs and axis types of test_gpu_projection.test_vector_reproject_matrix_on_the_gpu, plus axes in degrees
MATRIX_CASES = [
    (STERE, GEO, np.linspace(-25, 25, 60), np.linspace(52, 78, 40), (1, 2)),
    (GEO, LCC, (np.arange(40) - 19.5) * 25000.0, (np.arange(30) - 14.5) * 25000.0, (0, 0)),
    (ROT, STERE_OBL, np.linspace(-8e5, 8e5, 33), np.linspace(-6e5, 6e5, 21), (0, 0)),
    (POLAR0, POLAR90, np.arange(5) - 2., np.arange(5) - 2., (0, 0)),
    (LCC, GEO, np.linspace(0, 30, 31), np.linspace(70, 55, 16), (1, 2)),        # LONGITUDE / LATITUDE axes in degrees, descending y
    (STERE_OBL, ROT, np.linspace(-12, 14, 27), np.linspace(-9, 9, 19), (1, 2)),  # rotated lat/lon: degrees, but not "latlong" (:408)
]


@pytest.fixture
def hooked(ref):
    ref.set_transform(po.transform)
    yield ref
    ref.set_transform(None)


def test_projection_calls_fail_without_a_hook(ref):
    ref.set_transform(None)
    assert ref.project_values(GEO, STERE, [0.1], [1.0])[2] == oracle.ERROR
    assert ref.project_axes(GEO, STERE, [0.1, 0.2], [1.0])[2] == oracle.ERROR
    assert ref.get_vector_reproject_matrix(STERE, GEO, [0., 1.], [60., 61.], 1, 2)[1] == oracle.ERROR


@pytest.mark.parametrize("case", MATRIX_CASES, ids=lambda c: "%dx%d_types%d%d" % (len(c[2]), len(c[3]), c[4][0], c[4][1]))
def test_vector_reproject_matrix(hooked, case):
    """mifi_get_vector_reproject_matrix and _field with the five PROJ.4 calls answered by oracle.proj_oracle.transform on both
    sides.  This pins the reference's mesh loops, degree conversion, finite-difference deltas, atan2 / bearing and the
    normalisation (src/interpolation.c:330-521, 667-788), NOT the projections: those stay pinned by Snyder / EPSG."""
    from test_oracle_kats import _rotation_matrix, _rotation_matrix_field
    pin, pout, xa, ya, types = case
    want, rc = hooked.get_vector_reproject_matrix(pin, pout, xa, ya, types[0], types[1])
    assert rc == oracle.OK
    got = _rotation_matrix(pin, pout, xa, ya, types[0], types[1])
    assert same64(got, want), describe64(got, want)
    # _field: the mesh of the output axes taken back to the input projection is the field in the input projection
    r = lambda a, t: np.radians(a) if t != oracle.PROJ_AXIS else np.asarray(a, float)
    xx, yy = np.meshgrid(r(xa, types[0]), r(ya, types[1]))
    in_x, in_y = po.transform(pout, pin, xx.ravel(), yy.ravel())
    want, rc = hooked.get_vector_reproject_matrix_field(pin, pout, in_x, in_y, len(xa), len(ya))
    assert rc == oracle.OK
    out_x, out_y = po.transform(pin, pout, in_x, in_y)
    got = _rotation_matrix_field(pin, pout, in_x, in_y, out_x, out_y, len(xa), len(ya))
    assert same64(got, want), describe64(got, want)


SMALL_MESHES = [(1, 1), (1, 2), (2, 1), (1, 9), (9, 1), (2, 2), (3, 2), (40, 2), (2, 3), (2, 4), (2, 5), (3, 3), (3, 4), (4, 3), (5, 5)]


@pytest.mark.parametrize("mesh", SMALL_MESHES, ids=lambda m: "%dx%d" % m)
def test_vector_reproject_matrix_small_meshes(hooked, mesh):
    """Every branch of the delta (:463-508): one column, one row, one point, and the meshes around divergence D7.  Where the
    predicate holds the reference is not called; the restatement then takes the first probe alone, and the matrix is a
    rotation all the same."""
    from test_oracle_kats import _rotation_matrix, second_probe_outside
    ox, oy = mesh
    assert second_probe_outside(ox, oy) == (mesh in [(2, 2), (3, 2), (40, 2), (2, 3), (2, 4)])
    for pin, pout, xa, ya, types in ((STERE, GEO, np.linspace(-3, 3, ox), np.linspace(60, 62, oy), (1, 2)),
                                     (GEO, LCC, (np.arange(ox) - 1.5) * 25000.0, (np.arange(oy) + 2.5) * 25000.0, (0, 0)),
                                     (ROT, STERE_OBL, np.linspace(8e5, -8e5, ox), np.linspace(-6e5, 6e5, oy), (0, 0))):
        got = _rotation_matrix(pin, pout, xa, ya, types[0], types[1])
        if second_probe_outside(ox, oy):
            g = got.reshape(-1, 4)
            assert np.all(np.abs(np.hypot(g[:, 0], g[:, 1]) - 1) < 1e-14) and np.array_equal(g[:, 2], -g[:, 1])
            continue
        want, rc = hooked.get_vector_reproject_matrix(pin, pout, xa, ya, types[0], types[1])
        assert rc == oracle.OK
        assert same64(got, want), (pin, describe64(got, want))


@pytest.mark.parametrize("pin,pout,metric", [(STERE, GEO, True), (GEO, STERE_OBL, False), (ROT, LCC, False), (LCC, ROT, True)])
def test_vector_reproject_matrix_points(hooked, pin, pout, metric):
    """mifi_get_vector_reproject_matrix_points: fixed differences of 100 m or 1e-5 (src/interpolation.c:649)."""
    rng = np.random.default_rng(8)
    if po.is_latlong(po.parse(pout)) or pout == ROT:
        ox, oy = np.radians(rng.uniform(-20, 40, 500)), np.radians(rng.uniform(45, 80, 500))
    else:
        ox, oy = rng.uniform(-8e5, 8e5, 500), rng.uniform(-6e5, 6e5, 500)
    want, rc = hooked.get_vector_reproject_matrix_points(pin, pout, metric, ox, oy)
    assert rc == oracle.OK
    delta = 100.0 if metric else 0.00001
    ix, iy = po.transform(pout, pin, ox, oy)
    xdx = po.transform(pin, pout, ix + delta, iy)
    ydy = po.transform(pin, pout, ix, iy + delta)
    got = oracle.vector_matrix_from_deltas(ox, oy, xdx, ydy, delta, delta, po.is_latlong(po.parse(pout)))
    assert same64(got, want), describe64(got, want)


def test_matrix_from_deltas_of_either_sign(hooked):
    """Negative deltas (a descending x axis in the input projection) take the `sign < 0` branches."""
    xa, ya = np.linspace(8e5, -8e5, 33), np.linspace(6e5, -6e5, 21)
    from test_oracle_kats import _rotation_matrix
    for pin, pout in ((ROT, STERE_OBL), (GEO, LCC)):
        want, rc = hooked.get_vector_reproject_matrix(pin, pout, xa, ya, 0, 0)
        assert rc == oracle.OK
        got = _rotation_matrix(pin, pout, xa, ya, 0, 0)
        assert same64(got, want), describe64(got, want)


@pytest.mark.parametrize("case", MATRIX_CASES[:6], ids=lambda c: "%dx%d" % (len(c[2]), len(c[3])))
def test_project_axes_and_values(hooked, case):
    """mifi_project_axes: the reference's (y, x) mesh loop; mifi_project_values: the plain pass-through.  Projections by the hook."""
    pin, pout, xa, ya, types = case
    r = lambda a, t: np.radians(a) if t != oracle.PROJ_AXIS else np.asarray(a, float)
    xa, ya = r(xa, types[0]), r(ya, types[1])
    wx, wy, rc = hooked.project_axes(pout, pin, xa, ya)
    assert rc == oracle.OK
    gx, gy = po.project_axes(pout, pin, xa, ya)
    assert same64(gx, wx) and same64(gy, wy)
    vx, vy, rc = hooked.project_values(pout, pin, gx[:17] * 1.0, gy[:17] * 1.0)
    assert rc == oracle.OK
    tx, ty = po.transform(pout, pin, gx[:17], gy[:17])
    assert same64(tx, vx) and same64(ty, vy)


def test_shim_is_latlong_is_proj4s(ref):
    """interpolation.c:366/408 rely on pj_is_latlong being false for ob_tran; the stand-in and proj_oracle agree."""
    import ctypes
    L = ref.lib
    L.pj_init_plus.restype = ctypes.c_void_p
    L.pj_init_plus.argtypes = [ctypes.c_char_p]
    L.pj_is_latlong.argtypes = [ctypes.c_void_p]
    L.pj_free.argtypes = [ctypes.c_void_p]
    for s in (GEO, STERE, ROT, LCC, "+proj=longlat +datum=WGS84", "+proj=latlon +R=1", "+proj=lonlat +R=1", "+R=1 +proj=latlong",
              "+proj=ob_tran +o_proj=latlong +o_lat_p=30 +R=1"):
        pj = L.pj_init_plus(s.encode())
        assert bool(L.pj_is_latlong(pj)) == po.is_latlong(po.parse(s)), s
        L.pj_free(pj)


# ---------------------------------------------------------------- vertical_coordinate_transformations.c
def _kat_inputs(golden_dir, name):
    from test_vertical_levels_ref import _load
    return _load(name)


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_vertical_transformations_live(ref, golden_dir):
    """The seeded inputs of tests/golden/vertical_transform_kats.json through the live library instead of the recorded column,
    with the bounds tests/test_vertical_levels_ref.py states: bit-identical where only + - * / are involved or the C
    library's log is used, one float32 step where numpy's log / exp stand in for the C library's.  The live answers also
    equal the recorded ones."""
    import vertical_levels_ref as vl
    from test_vertical_levels_ref import _ulps_f32
    (q, T), rec = _kat_inputs(golden_dir, "mifi_virtual_temperature")
    live = np.array([ref.lib.mifi_virtual_temperature(float(a), float(b)) for a, b in zip(q, T)], np.float32)
    assert np.array_equal(_bits(live), _bits(rec))
    assert np.array_equal(_bits(vl.virtual_temperature(q, T)), _bits(live))
    (pl, ph, T), rec = _kat_inputs(golden_dir, "mifi_barometric_layer_thickness")
    live = np.array([ref.lib.mifi_barometric_layer_thickness(float(a), float(b), float(c)) for a, b, c in zip(pl, ph, T)], np.float32)
    assert np.array_equal(_bits(live), _bits(rec))
    assert np.array_equal(_bits(vl.layer_thickness(pl, ph, T, log=vl.c_log)), _bits(live))
    assert np.all(_ulps_f32(vl.layer_thickness(pl, ph, T), live) <= 1)
    for name, fn in (("mifi_barometric_standard_altitude", vl.standard_altitude), ("mifi_barometric_standard_pressure", vl.standard_pressure)):
        (x,), rec = _kat_inputs(golden_dir, name)
        live, rc = ref.level_pressure(name, x)
        assert rc == oracle.OK and np.array_equal(_bits(live), _bits(rec)), name
        assert np.all(_ulps_f32(fn(x).astype(np.float32), live.astype(np.float32)) <= 1), name
    for name, fn in (("mifi_ocean_s_g1_z", vl.ocean_s_g1_z), ("mifi_ocean_s_g2_z", vl.ocean_s_g2_z)):
        (h, hc, zeta, sigma, C), rec = _kat_inputs(golden_dir, name)
        live = np.array([ref.level_pressure(name, float(a), float(b), float(c), np.array([d]), np.array([e]))[0][0]
                         for a, b, c, d, e in zip(h, hc, zeta, sigma, C)])
        assert np.array_equal(_bits(live), _bits(rec)), name
        assert np.array_equal(_bits(fn(h, hc, zeta, sigma, C)), _bits(live)), name


def _level_cases():
    """(kind, Levels keywords) on a 5x4x2 surface pressure field with 9 levels."""
    import vertical_ref as vr
    rng = np.random.default_rng(20)
    nx, ny, nt, nz = 5, 4, 2, 9
    ps = rng.uniform(600, 1040, (nt, ny, nx)).astype(np.float32)
    ps[0, 1, 2] = np.nan
    c = rng.uniform(0, 1, nz)
    return nx, ny, nt, nz, ps, [(vr.SIGMA, dict(sigma=c, ptop=5.0, ps=ps)), (vr.HYBRID_SIGMA, dict(a=0.3 * c, b=c * c, p0=1000.0, ps=ps)),
                                (vr.HYBRID_SIGMA_AP, dict(ap=300 * c, b=c * c, ps=ps))]


def test_level_pressure_formulas(ref):
    """mifi_atmosphere_sigma_pressure, _hybrid_sigma_pressure, _hybrid_sigma_ap_pressure per cell against
    vertical_levels_ref.level_field_double (the doubles) and vertical_ref.level_field (their float32 rounding)."""
    import vertical_levels_ref as vl
    import vertical_ref as vr
    nx, ny, nt, nz, ps, kinds = _level_cases()
    for kind, kw in kinds:
        lv = vr.Levels(kind, nz, **kw)
        d, f = vl.level_field_double(lv, nt, ny, nx), vr.level_field(lv, nt, ny, nx)
        for t in range(nt):
            for j in range(ny):
                for i in range(nx):
                    p = float(ps[t, j, i])
                    if kind == vr.SIGMA:
                        want, rc = ref.level_pressure("mifi_atmosphere_sigma_pressure", kw["ptop"], p, kw["sigma"])
                    elif kind == vr.HYBRID_SIGMA:
                        want, rc = ref.level_pressure("mifi_atmosphere_hybrid_sigma_pressure", kw["p0"], p, kw["a"], kw["b"])
                    else:
                        want, rc = ref.level_pressure("mifi_atmosphere_hybrid_sigma_ap_pressure", p, kw["ap"], kw["b"])
                    assert rc == oracle.OK
                    assert same64(d[t, :, j, i], want), (kind, t, j, i, describe64(d[t, :, j, i], want))
                    assert cases.same(f[t, :, j, i], want.astype(np.float32)), (kind, t, j, i)


# ---------------------------------------------------------------- recorded answers: needs no reference, never skips
def test_recorded_answers(golden_dir):
    """tests/golden/reference_answers.npz (answers of oracle/_ref/libmifi_ref.so, recorded by scripts/record_reference_answers.py)
    replayed through the oracle: the same comparisons as the live tests, on a machine that has neither the reference nor
    oracle/_ref."""
    import reference_answers as ra
    fx = ra.load(golden_dir)
    n = 0
    for name in fx.names("regrid"):
        c = fx.case(name)
        inX, inY, nz = int(c["shape"][0]), int(c["shape"][1]), int(c["shape"][2])
        for method in (oracle.NEAREST, oracle.BILINEAR, oracle.BICUBIC):
            skip = c["skip%d" % method].astype(bool)
            assert np.array_equal(skip, skip_mask(method, c["px"], c["py"], inX, inY))
            got = oracle.interpolate_values(method, c["px"], c["py"], c["in"], inX, inY, c["px"].size, 1).reshape(nz, -1)
            want = c["out%d" % method].view(np.float32)
            assert np.all(np.isnan(got[:, skip]))
            assert cases.same(got[:, ~skip], want[:, ~skip]), (name, method, cases.describe_mismatch(got[:, ~skip], want[:, ~skip]))
            assert int(c["rc%d" % method]) == oracle.OK
            n += 1
    for name in fx.names("fill2d"):
        c = fx.case(name)
        for z in range(c["in"].shape[0]):
            a, nch, rc = oracle.fill2d(c["in"][z], float(c["params"][0]), float(c["params"][1]), int(c["params"][2]))
            assert rc == int(c["rc"][z]) and nch == int(c["nChanged"][z]), name
            assert cases.same(a, c["out"][z].view(np.float32)), (name, z, cases.describe_mismatch(a, c["out"][z].view(np.float32)))
            n += 1
    for name in fx.names("creepfill2d") + fx.names("creepfillval2d"):
        c = fx.case(name)
        for z in range(c["in"].shape[0]):
            if name.startswith("creepfillval2d"):
                a, nch, rc = oracle.creepfillval2d(c["in"][z], np.float32(c["params"][2]), int(c["params"][0]), int(c["params"][1]))
            else:
                a, nch, rc = oracle.creepfill2d(c["in"][z], int(c["params"][0]), int(c["params"][1]))
            assert rc == int(c["rc"][z]) and nch == int(c["nChanged"][z]), name
            assert cases.same(a, c["out"][z].view(np.float32)), (name, z, cases.describe_mismatch(a, c["out"][z].view(np.float32)))
            n += 1
    for name in fx.names("rotation"):
        c = fx.case(name)
        ox, oy = int(c["shape"][0]), int(c["shape"][1])
        gu, gv = oracle.vector_reproject_values(c["matrix"], c["u"], c["v"], ox, oy)
        assert cases.same(gu, c["u_out"].view(np.float32)) and cases.same(gv, c["v_out"].view(np.float32)), name
        assert cases.same(oracle.vector_reproject_direction(c["matrix"], c["angles"], ox, oy), c["angles_out"].view(np.float32)), name
        n += 1
    for name in fx.names("points2position"):
        c = fx.case(name)
        got = oracle.points2position(c["points"], c["axis"], int(c["axis_type"]))
        assert same64(got, c["out"].view(np.float64)), (name, describe64(got, c["out"].view(np.float64)))
        n += 1
    for name in fx.names("blend"):
        c = fx.case(name)
        for k, (kind, a, b, x) in enumerate(c["kabx"]):
            got, rc = oracle.get_values_1d(int(kind), c["A"], c["B"], a, b, x)
            assert rc == int(c["rc"][k]), (name, k)
            assert cases.same(got, c["out"][k].view(np.float32)), (name, k, cases.describe_mismatch(got, c["out"][k].view(np.float32)))
            n += 1
        for k, (a, b, x) in enumerate(c["abx_d"]):
            got = oracle.get_values_linear_d(c["A"].astype(np.float64), c["B"].astype(np.float64), a, b, x)
            assert same64(got, c["out_d"][k].view(np.float64)), (name, k)
    for name in fx.names("badvalue"):
        c = fx.case(name)
        for k, bad in enumerate(c["bad"].view(np.float32)):
            assert cases.same(oracle.bad2nan(c["in"], bad), c["bad2nan"][k].view(np.float32)), (name, k)
            g = oracle.nan2bad(c["in"], bad)
            w = c["nan2bad"][k].view(np.float32)
            assert cases.same(g, w) and np.all(np.isnan(g) | (g.view(np.uint32) == w.view(np.uint32))), (name, k)
            n += 1
    import vertical_ref as vr
    for name in fx.names("levels"):
        c = fx.case(name)
        lv, (nt, ny, nx) = ra.levels_of(vr.Levels, c), c["ps"].shape
        got = vr.level_field(lv, nt, ny, nx)
        assert cases.same(got, c["out"].view(np.float64).astype(np.float32)), name
        n += 1
    assert n >= 40
