"""The PROJ.4 string parser (fimex_amd/csrc/projection_parse.hip) and the point math the projection kernels compile
(fimex_amd/csrc/proj_math.hpp) run here on the CPU: tests/projection_host.hip calls them point by point the way the kernels do, and
fimex_amd/build.py compiles it for the host only.  Against oracle/proj_oracle.py with the tolerances tests/test_gpu_projection.py
applies to the same comparisons on the GPU; the refusals against the wording of each message.  No GPU is involved."""
import ctypes

import numpy as np
import pytest

import oracle
from fimex_amd import build as fb
from oracle import proj_oracle as po
from projection_cases import (ALL, DATUM_PAIRS, ELLIPSOIDAL, GEO, GEO_W, LCC, NADGRIDS, OMERC_TWO_POINT, ROT, STERE, STERE_OBL, TMERC_S, UNIT_EXTRAS,
                              UNSUPPORTED, UTM33, close, ellipsoidal_points, spherical_points)
from test_oracle_kats import second_probe_outside

N = 2000
_P, _D, _I64 = ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int64


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(fb.build_projection_host())
    err = [ctypes.c_char_p, ctypes.c_size_t]
    lib.projection_host_transform.argtypes = [_P, _P, _D, _D, _I64] + err
    lib.projection_host_matrix.argtypes = [_P, _P, _D, _D, _D, _D, _I64, ctypes.c_double, ctypes.c_double, _D] + err
    lib.projection_host_bounding_box.argtypes = [_P, _P, _D, _D, _I64] + [ctypes.c_double] * 4 + [_D] + err
    lib.projection_host_mesh_delta.argtypes = [_D, _I64, _I64, ctypes.POINTER(ctypes.c_int)]
    lib.projection_host_mesh_delta.restype = ctypes.c_double
    return lib


class Refused(Exception):
    pass


def _checked(rc, buf):
    if rc != 0:
        raise Refused(buf.value.decode())


def transform(shim, src, dst, x, y):
    x, y = np.array(x, dtype=np.float64).ravel(), np.array(y, dtype=np.float64).ravel()   # copies: the shim works in place
    buf = ctypes.create_string_buffer(1024)
    _checked(shim.projection_host_transform(src.encode(), dst.encode(), x.ctypes.data, y.ctypes.data, x.size, buf, len(buf)), buf)
    return x, y


@pytest.mark.parametrize("dst", ALL)
def test_project_values_from_geographic_and_back(shim, dst):
    lon, lat = spherical_points(dst, N)
    x, y = transform(shim, GEO, dst, lon, lat)
    wx, wy = po.transform(GEO, dst, lon, lat)
    close(x, wx, dst); close(y, wy, dst)
    bx, by = transform(shim, dst, GEO, x, y)  # round trip through the inverse
    np.testing.assert_allclose(bx, lon, atol=1e-11); np.testing.assert_allclose(by, lat, atol=1e-11)


@pytest.mark.parametrize("dst", ELLIPSOIDAL)
def test_ellipsoidal_projections_from_geographic_and_back(shim, dst):
    series = "proj=tmerc" in dst   # Gauss-Krueger truncated; utm and etmerc carry the series to n^6 and hold far out
    lon, lat = ellipsoidal_points(dst, N)
    x, y = transform(shim, GEO_W, dst, lon, lat)
    wx, wy = po.transform(GEO_W, dst, lon, lat)
    atol = 2e-6 if dst == TMERC_S else 2e-8   # metres; the spherical form takes acos of nearly 1 at the equator
    np.testing.assert_allclose(x, wx, rtol=2e-12, atol=atol); np.testing.assert_allclose(y, wy, rtol=2e-12, atol=atol)
    bx, by = transform(shim, dst, GEO_W, x, y)
    wbx, wby = po.transform(dst, GEO_W, x, y)
    np.testing.assert_allclose(bx, wbx, atol=2e-13); np.testing.assert_allclose(by, wby, atol=2e-13)
    tol = 2e-7 if series else (1e-9 if "laea" in dst or "cea" in dst else 2e-10)  # truncated series do not invert themselves exactly
    np.testing.assert_allclose(bx, lon, atol=tol); np.testing.assert_allclose(by, lat, atol=tol)


@pytest.mark.parametrize("pair", DATUM_PAIRS, ids=range(len(DATUM_PAIRS)))
def test_datum_shifts_between_sides_that_both_name_a_datum(shim, pair):
    src, dst = pair
    rng = np.random.default_rng(3)
    lon, lat = np.radians(rng.uniform(-10, 30, N)), np.radians(rng.uniform(35, 70, N))
    x, y = transform(shim, src, dst, lon, lat)
    wx, wy = po.transform(src, dst, lon, lat)
    scale = 1.0 if "latlong" in dst else 6.4e6
    np.testing.assert_allclose(x, wx, rtol=0, atol=2e-12 * scale); np.testing.assert_allclose(y, wy, rtol=0, atol=2e-12 * scale)
    bx, by = transform(shim, dst, src, x, y)
    np.testing.assert_allclose(bx, lon, atol=2e-9); np.testing.assert_allclose(by, lat, atol=2e-9)


def test_no_datum_shift_when_one_side_names_no_datum(shim):
    rng = np.random.default_rng(3)
    lon, lat = np.radians(rng.uniform(-10, 30, N)), np.radians(rng.uniform(35, 70, N))
    moved = transform(shim, "+proj=latlong +datum=WGS84", "+proj=latlong +datum=potsdam", lon, lat)
    assert 1e-5 < np.abs(moved[0] - lon).max() < 3e-4
    same = transform(shim, "+proj=latlong +datum=WGS84", "+proj=latlong +ellps=bessel", lon, lat)
    assert np.array_equal(same[0], lon) and np.array_equal(same[1], lat)


@pytest.mark.parametrize("proj", [STERE, UTM33])
@pytest.mark.parametrize("extra", UNIT_EXTRAS)
def test_units_and_prime_meridians(shim, proj, extra):
    """+units / +to_meter (pj_fwd.c, pj_inv.c) and +pm (pj_transform.c) on either side of a transformation"""
    rng = np.random.default_rng(len(proj) + len(extra))
    lon = np.radians(rng.uniform(2, 28, N))
    lat = np.radians(rng.uniform(45, 80, N))
    geo = GEO_W if "ellps" in proj or "datum" in proj else GEO
    dst = proj + " " + extra
    x, y = transform(shim, geo, dst, lon, lat)
    wx, wy = po.transform(geo, dst, lon, lat)
    close(x, wx, dst); close(y, wy, dst)
    bx, by = transform(shim, dst, geo, x, y)
    np.testing.assert_allclose(bx, lon, atol=1e-11); np.testing.assert_allclose(by, lat, atol=1e-11)
    if "pm" in extra:  # the meridian on the geographic side
        gx, gy = transform(shim, geo + " +pm=lisbon", proj, lon, lat)
        vx, vy = po.transform(geo + " +pm=lisbon", proj, lon, lat)
        close(gx, vx, proj); close(gy, vy, proj)
    if proj == UTM33:  # the mesh of two axes in the scaled unit, back to geographic
        ax, ay = np.linspace(2e5, 6e5, 40) / po.to_meter_of(po.parse(dst)), np.linspace(5.5e6, 6.5e6, 30) / po.to_meter_of(po.parse(dst))
        xx, yy = np.meshgrid(ax, ay)
        gx, gy = transform(shim, dst, geo, xx, yy)
        vx, vy = po.project_axes(dst, geo, ax, ay)
        np.testing.assert_allclose(gx, vx, atol=1e-12); np.testing.assert_allclose(gy, vy, atol=1e-12)


def test_transverse_mercator_refuses_the_far_side(shim):
    lon, lat = np.radians([15., 120., -100., 15.]), np.radians([60., 60., 10., -30.])
    tm33 = "+proj=tmerc +lon_0=15 +k=0.9996 +x_0=500000 +ellps=WGS84"
    x, y = transform(shim, GEO_W, tm33, lon, lat)
    wx, wy = po.transform(GEO_W, tm33, lon, lat)
    assert np.array_equal(np.isnan(x), [False, True, True, False]) and np.array_equal(np.isnan(x), np.isnan(wx))
    assert np.array_equal(np.isnan(y), np.isnan(wy))
    assert abs(x[0] - 500000.) < 1e-6 and abs(y[0] - wy[0]) < 1e-7


# (string, what its refusal says): every string test_gpu_projection.py expects the library to refuse, and one more for each other
# refusal of the parser that a string can reach.  The fragments are the parser's wording before it was split into set-up functions.
REFUSALS = [
    (UNSUPPORTED[0], "utm needs an ellipsoid: "),
    (UNSUPPORTED[1], "invalid UTM zone: "),
    (UNSUPPORTED[2], "the equatorial stereographic projection is implemented on the sphere only: "),
    (UNSUPPORTED[3], "projection string without +proj: "),
    (UNSUPPORTED[4], "ob_tran is implemented for +o_proj=longlat +o_lat_p only: "),
    (UNSUPPORTED[5], "ob_tran is implemented on the sphere only: "),
    (UNSUPPORTED[6], "unknown +units: "),
    (UNSUPPORTED[7], "invalid +to_meter: "),
    (UNSUPPORTED[8], "projection +axis other than enu is not implemented: "),
    (UNSUPPORTED[9], "+units / +to_meter with ob_tran are not implemented: "),
    (UNSUPPORTED[10], "+pm is neither a known meridian nor decimal degrees: "),
    (UNSUPPORTED[11], "datum not implemented: "),
    (UNSUPPORTED[12], "ellipsoid not implemented: "),
    (UNSUPPORTED[13], "projection string without an ellipsoid (+R, +a or +ellps): "),
    (UNSUPPORTED[14], "lcc: lat_1 = -lat_2: "),
    (UNSUPPORTED[15], "omerc is implemented by central point and azimuth (+lonc +alpha / +gamma) only: "),
    (UNSUPPORTED[16], "ortho is implemented on the sphere only: "),
    (UNSUPPORTED[17], "nsper needs +h > 0: "),
    (UNSUPPORTED[18], "projection not implemented: moll"),
    (NADGRIDS, "projection parameter +nadgrids is not implemented: "),
    (OMERC_TWO_POINT, "omerc is implemented by central point and azimuth (+lonc +alpha / +gamma) only: "),
    ("+proj=merc +R=abc", "projection parameter +R is not a number: "),
    ("+proj=merc +R=6371000 +lon_0=east", "projection parameter +lon_0 is not a number: "),
    ("+proj=merc +R=6371000 +geoc", "projection parameter +geoc is not implemented: "),
    ("+proj=merc +R=6371000 +over", "projection parameter +over is not implemented: "),
    ("+proj=merc +R=6371000 +to_meter=abc", "+to_meter is not a number: "),
    ("+proj=merc +R=6371000 +to_meter=1/x", "+to_meter is not a number: "),
    ("+proj=merc +R=6371000 +units=km +to_meter=-2", "invalid +to_meter: "),
    ("+proj=merc +datum=NAD27 +towgs84=1,2,3", "datum not implemented: "),   # the ellipsoid a datum implies
    ("+proj=merc +R=1 +towgs84=a,b,c", "+towgs84 is not a list of numbers: "),
    ("+proj=merc +a=6378137 +es=1.5", "invalid ellipsoid: "),
    ("+proj=merc +a=-1 +b=1", "invalid ellipsoid: "),
    ("+proj=merc +R=6371000 +lat_ts=90", "merc: lat_ts >= 90: "),
    ("+proj=etmerc +lon_0=9 +R=6371000", "etmerc needs an ellipsoid: "),
    ("+proj=utm +zone=61 +ellps=WGS84", "invalid UTM zone: "),
    ("+proj=cea +R=6371000 +lat_ts=100", "cea: |lat_ts| > 90: "),
    ("+proj=aeqd +lat_0=40 +ellps=WGS84", "aeqd is implemented on the sphere only: "),
    ("+proj=nsper +h=2e7 +lat_0=40 +ellps=WGS84", "nsper is implemented on the sphere only: "),
    ("+proj=omerc +lat_0=40 +lonc=10 +alpha=0 +ellps=WGS84", "omerc: alpha of 0 or 180 degrees, or lat_0 at a pole: "),
    ("+proj=omerc +lat_0=90 +lonc=10 +alpha=30 +ellps=WGS84", "omerc: alpha of 0 or 180 degrees, or lat_0 at a pole: "),
    ("+proj=geos +lon_0=0 +R=6371000", "geos needs +h > 0: "),
    ("+proj=geos +h=3.5e7 +lat_0=10 +R=6371000", "geos: lat_0 must be 0: "),
    ("+proj=geos +h=3.5e7 +sweep=z +R=6371000", "geos: +sweep must be x or y: "),
    ("+proj=aea +lat_1=30 +lat_2=-30 +R=6371000", "aea: lat_1 = -lat_2: "),
    ("+proj=ob_tran +o_proj=longlat +R=6371000", "ob_tran is implemented for +o_proj=longlat +o_lat_p only: "),
]


@pytest.mark.parametrize("bad,says", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_strings_say_why(shim, bad, says):
    for pair in ((GEO_W, bad), (bad, GEO_W)):   # on either side of a pair
        with pytest.raises(Refused) as e:
            transform(shim, pair[0], pair[1], np.zeros(3), np.zeros(3))
        message = str(e.value)
        assert message == (says + bad if says.endswith(": ") else says), message


@pytest.mark.parametrize("pin,pout,metric", [(STERE, GEO, True), (LCC, STERE_OBL, True), (ROT, GEO, False)], ids=["into_latlong", "between_projected", "from_rotated"])
def test_matrix_entries_at_points(shim, pin, pout, metric):
    """The per-point body of vector_matrix_kernel: fixed 100 m / 1e-5 rad differences, as mifi_get_vector_reproject_matrix_points"""
    rng = np.random.default_rng(8)
    lon, lat = np.radians(rng.uniform(-20, 40, 500)), np.radians(rng.uniform(45, 80, 500))
    ox, oy = po.transform(GEO, pout, lon, lat)
    ix, iy = po.transform(pout, pin, ox, oy)
    delta = 100. if metric else 0.00001
    got = np.empty((ox.size, 4))
    buf = ctypes.create_string_buffer(1024)
    _checked(shim.projection_host_matrix(pin.encode(), pout.encode(), ix.ctypes.data, iy.ctypes.data, ox.ctypes.data, oy.ctypes.data, ox.size,
                                         delta, delta, got.ctypes.data, buf, len(buf)), buf)
    xdx = po.transform(pin, pout, ix + delta, iy)
    ydy = po.transform(pin, pout, ix, iy + delta)
    want = oracle.vector_matrix_from_deltas(ox, oy, xdx, ydy, delta, delta, po.is_latlong(po.parse(pout))).reshape(-1, 4)
    np.testing.assert_allclose(got[:, :3], want[:, :3], atol=1e-7)
    np.testing.assert_allclose(np.hypot(got[:, 0], got[:, 1]), 1.0, atol=1e-14)
    np.testing.assert_array_equal(got[:, 2], -got[:, 1])
    np.testing.assert_allclose(np.cos(got[:, 3]), got[:, 0], atol=1e-15)


@pytest.mark.parametrize("box", [(55., 70., 0., 30.), (60., 80., 170., -170.)], ids=["plain", "across_180"])
def test_bounding_box_keep_flags(shim, box):
    """A lane of bounding_box_kernel: the point in degrees inside the box; west > east wraps at 180; a failed transformation is outside"""
    south, north, west, east = box
    rng = np.random.default_rng(11)
    x, y = rng.uniform(-3e6, 3e6, N), rng.uniform(-3e6, 3e6, N)
    x[:3], y[:3] = np.nan, (0., np.nan, 1e5)
    keep = np.full(N, 7, dtype=np.uint8)
    buf = ctypes.create_string_buffer(1024)
    _checked(shim.projection_host_bounding_box(STERE.encode(), GEO.encode(), x.ctypes.data, y.ctypes.data, N, south, north, west, east,
                                               keep.ctypes.data, buf, len(buf)), buf)
    lon, lat = (np.degrees(a) for a in po.transform(STERE, GEO, x, y))
    with np.errstate(invalid="ignore"):
        inside_lon = ~((lon > east) & (lon < west)) if west > east else ~((lon < west) | (lon > east))
        want = np.isfinite(lon) & np.isfinite(lat) & ~((lat < south) | (lat > north)) & inside_lon
        edge = np.minimum.reduce([np.abs(lat - south), np.abs(lat - north), np.abs(lon - west), np.abs(lon - east)]) < 1e-9
    assert not keep[:3].any() and set(np.unique(keep)) == {0, 1}
    assert np.array_equal(keep[~edge].astype(bool), want[~edge])


def _delta(f, ox, oy):
    """the delta of mifi_get_vector_reproject_matrix_proj (src/interpolation.c:458-518) with divergence D7"""
    d = 1e-3
    if ox > 1 and oy > 1:
        delta = d * (f[ox + 1] - f[0])
        if not second_probe_outside(ox, oy):
            delta = (delta + d * (f[(oy // 2 + 1) * ox + ox // 2 + 1] - f[(oy // 2) * ox + ox // 2])) / 2
    elif ox > 1:
        delta = d * (f[1] - f[0])
    elif oy > 1:
        delta = d * (f[ox] - f[0])
    else:
        delta = f[0] * d if f[0] > 1 else d
    return d if abs(delta) < 1e-9 else delta


@pytest.mark.parametrize("mesh", [(1, 1), (1, 9), (9, 1), (2, 2), (3, 2), (40, 2), (2, 3), (2, 4), (2, 5), (3, 3), (7, 6)], ids=lambda m: "%dx%d" % m)
def test_mesh_delta(shim, mesh):
    """Every branch of the delta, and the meshes of divergence D7 (oy == 2, or ox == 2 with oy <= 4), where the reference's second
    probe is past the mesh: the first probe stands alone and nothing beyond the mesh is read."""
    ox, oy = mesh
    assert second_probe_outside(ox, oy) == (ox > 1 and (oy == 2 or (ox == 2 and 1 < oy <= 4)))
    rng = np.random.default_rng(ox * 100 + oy)
    beyond = ctypes.c_int(-1)
    for scale in (25000., 0.5, 1e-8):   # metres, radians, and a mesh so fine that the floor of 1e-9 applies
        f = np.cumsum(rng.uniform(0.5, 1.5, ox * oy)) * scale + (3. if scale > 1 else 0.)
        got = shim.projection_host_mesh_delta(f.ctypes.data, ox, oy, ctypes.byref(beyond))
        assert beyond.value == 0
        assert got == _delta(f, ox, oy), (got, _delta(f, ox, oy))
        if scale == 1e-8:
            assert got == 1e-3
