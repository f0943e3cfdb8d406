"""The streaming kernels that launch a capped grid and cover the rest with a grid-stride loop, beyond one pass of that grid.

Three families launch at most 256 * 8 workgroups of 256 lanes -- L lanes -- and stride from there:
  convert.hip      capped_blocks(): launch_replace and stream_blocks want ceil(n / 1024) workgroups (a lane takes a 16-byte group
                   of four), launch_points2position ceil(n / 256)
  projection.hip   point_blocks(n): ceil(n / 256); the bounding box hands it 64 lanes per wave of ceil(nx / 64) * ny waves
  coordsearch.hip  blocks_for(n): ceil(n / 256), for the source cells (keys, points) and for the queries
Every production call strides.  Part (a) lowers the cap to 2 workgroups (FIMEX_AMD_{CONVERT,PROJECT,COORD}_MAX_BLOCKS on the tuning
build: a stride of 512 lanes) so that small shapes take every loop more than once; part (b) runs the product library, whose launch
rule cannot be changed, at the smallest sizes that stride; part (c) is the coordinate search where cubes of unit vectors and the
reference's walk along sorted latitudes could disagree.  Every comparison is with the CPU oracle under the bounds the other files
use: cases.same / bit equality for convert.hip, _close of test_gpu_projection.py, _same_cells_or_ties with its 2 % cap and 1e-12 on
the grid distance for the search.  Outputs of convert.hip lie between guard bands that must survive.

What the older files already reach (found by leaving each striding loop after its first iteration and running them): blend_kernel,
undefined_kernel and replace_scalar_kernel take one element per lane but are launched with one workgroup per 1024, so they make four
passes at any size; points2position is compared with the oracle on 4 M points in test_gpu_fullsize.py; project_axes_kernel and
vector_matrix_kernel run a 1201 x 1201 mesh in test_wind_to_a_projection_and_back, checked by the round trip only.  Nothing older
notices the same mutation in replace_kernel, the VEC bodies of to_float_kernel / from_float_kernel, project_values_kernel,
bounding_box_kernel, source_points_kernel or nearest_kernel; the tests below do.

CPU oracle times at the sizes of part (b), one call each, on 8 cores: numpy projection of 2 L + 77 points 0.11 s (sphere), 0.58 s
(UTM on the ellipsoid); the 1031 x 1021 mesh 0.11 s; the rotation matrix on 1031 x 521 0.15 s; grid distance of 1031 x 521 cells
0.74 s, the latitude walk for 1000 queries on them 0.83 s (it holds the grid distance), the exhaustive kd search 0.15 s;
L + L / 2 + 77 queries on 30 x 20 cells 0.08 s and 0.11 s.  None needed shrinking, and the matrix is compared on the whole mesh."""
import numpy as np
import pytest

import cases
import extract_ref
import oracle
from oracle import proj_oracle as po
from test_gpu_parity import _float_field, _same_cells_or_ties, _typed_field
from test_gpu_projection import GEO, GEO_W, LCC, ROT, STERE, STERE_OBL, UTM33, _close
from test_oracle_kats import _rotation_matrix
from test_oracle_props import _curvilinear_grid, _great_circle_cos, _xyz, coord_search_inputs

pytestmark = pytest.mark.gpu

L = 2048 * 256   # lanes of a capped grid
S = 2 * 256      # the same with the cap lowered to 2 workgroups
GUARD = 64       # bytes of 0xAB on either side of an output, a multiple of 16
FILL = 9.96921e36


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1
    return capi


@pytest.fixture
def capped(monkeypatch, tuning_build):
    for family in ("CONVERT", "PROJECT", "COORD"):
        monkeypatch.setenv("FIMEX_AMD_%s_MAX_BLOCKS" % family, "2")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, want):
    """cases.same for any element type: bit for bit on everything but NaN, whose positions must agree."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    ng, nw = np.isnan(got), np.isnan(want)
    return np.array_equal(ng, nw) and np.array_equal(_bits(got[~ng]), _bits(want[~nw]))


class _Guarded:
    """A device buffer for n elements of dt that starts `shift` elements behind a 16-byte boundary, between guard bands."""

    def __init__(self, dt, n, shift, init=None):
        import torch
        self.dt, self.n, self.size = np.dtype(dt), n, np.dtype(dt).itemsize
        self.first = GUARD + shift * self.size
        self.buf = torch.full((2 * GUARD + (n + 4) * self.size,), 0xAB, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        if init is not None:
            assert init.dtype == self.dt and init.size == n
            self.buf[self.first:self.first + n * self.size] = torch.from_numpy(_bits(init).view(np.uint8).copy()).cuda()
        self.ptr = self.buf.data_ptr() + self.first

    def result(self):
        import torch
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        end = self.first + self.n * self.size
        assert np.all(raw[:self.first] == 0xAB) and np.all(raw[end:] == 0xAB), "wrote outside the output"
        return raw[self.first:end].copy().view(self.dt)


# ---------------------------------------------------------------- convert.hip: fill value <-> NaN
def _replace_field(n, seed):
    """Mostly plain values, so that most 16-byte groups hold no hit and are not written back; the fill value, NaN, +-0, +-inf and
    denormals in about one element of thirty, spread over the whole length."""
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 1, n).astype(np.float32)
    special = np.array([FILL, FILL, np.nan, np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-42], np.float32)
    k = rng.choice(n, n // 30, replace=False)
    a[k] = special[rng.integers(0, special.size, k.size)]
    a[-1], a[-2] = FILL, np.nan   # the scalar tail holds both
    return a


def _check_replace(fa, n, shift, seed):
    a = _replace_field(n, seed)
    groups = a[:n - n % 4].reshape(-1, 4)
    assert ((groups == np.float32(FILL)) | np.isnan(groups)).any(axis=1).mean() < 0.5   # groups without a hit are the common case
    for name, bad, ref in (("bad2nan", FILL, oracle.bad2nan), ("nan2bad", -32767.0, oracle.nan2bad)):
        g = _Guarded(np.float32, n, shift, a)
        getattr(fa, name + "_device")(g.ptr, n, bad, _stream())
        got, want = g.result(), ref(a, bad)
        assert cases.same(got, want), (name, n, shift, cases.describe_mismatch(got, want))


# launch_replace: ceil(n / 1024) workgroups, capped; the kernel's main loop runs while i + 3 * stride < n / 4
@pytest.mark.parametrize("n", [4 * (4 * S + S // 2) + 3,   # main loop once, remainder loop for half the lanes, tail
                               4 * (2 * S + S // 2) + 1,   # remainder loop only
                               4 * (8 * S + 100) + 2],     # main loop twice
                         ids=["main_once", "remainder_only", "main_twice"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one_float_off"])
def test_replace_strides_under_a_lowered_cap(fa, capped, n, shift):
    _check_replace(fa, n, shift, seed=n + shift)


@pytest.mark.parametrize("n,shift", [(4 * (4 * L + L // 2) + 3, 0), (4 * (2 * L + L // 2) + 1, 0), (2 * L + 77, 1)],
                         ids=["main_once", "remainder_only", "scalar_kernel"])
def test_replace_strides_under_the_product_launch_rule(fa, n, shift):
    """9 437 187 floats are the smallest aligned array on which the product's bad2nan enters its four-way unrolled main loop."""
    _check_replace(fa, n, shift, seed=shift + 5)


# ---------------------------------------------------------------- convert.hip: typed edges of a slice
def _check_data2interpolation(fa, code, n, shifts):
    dt = oracle.CDM_DTYPES[code]
    a = _typed_field(dt, n, seed=code + n)
    bad = float(a[10])
    want = oracle.data2interpolation_array(a, bad)
    for s_in, s_out in shifts:
        src = _Guarded(dt, n, s_in, a)
        dst = _Guarded(np.float32, n, s_out)
        fa.data2interpolation_device(src.ptr, code, n, bad, dst.ptr, _stream())
        got = dst.result()
        assert cases.same(got, want), (code, s_in, s_out, cases.describe_mismatch(got, want))


def _check_interpolation2data(fa, code, n, shifts):
    dt = oracle.CDM_DTYPES[code]
    f = _float_field(n, 0, seed=code * 7 + n)
    want = oracle.interpolation_array2data(f, code, 77.0)
    for s_in, s_out in shifts:
        src = _Guarded(np.float32, n, s_in, f)
        dst = _Guarded(dt, n, s_out)
        fa.interpolation2data_device(src.ptr, n, code, 77.0, dst.ptr, _stream())
        got = dst.result()
        assert np.array_equal(_bits(got), _bits(want)), (code, s_in, s_out, int((_bits(got) != _bits(want)).sum()))


ALL_SHIFTS = [(0, 0), (0, 1), (1, 0), (1, 1)]   # (source, destination): the VEC body needs both on their boundaries


# stream_blocks: ceil(n / 1024) workgroups, capped: three passes of whole groups, a fourth for 100 lanes, a tail of 3
@pytest.mark.parametrize("code", sorted(oracle.CDM_DTYPES))
def test_typed_edges_stride_under_a_lowered_cap(fa, capped, code):
    n = 4 * (3 * S) + 4 * 100 + 3
    _check_data2interpolation(fa, code, n, ALL_SHIFTS)
    _check_interpolation2data(fa, code, n, ALL_SHIFTS)


@pytest.mark.parametrize("code", [oracle.CDM_UCHAR, oracle.CDM_SHORT, oracle.CDM_FLOAT, oracle.CDM_DOUBLE], ids=["uchar", "short", "float", "double"])
def test_typed_edges_stride_under_the_product_launch_rule(fa, code):
    """One type per element size; the second pass of the VEC bodies starts at n > 4 L."""
    n = 4 * (2 * L) + 4 * 777 + 3
    _check_data2interpolation(fa, code, n, [(0, 0)])
    _check_interpolation2data(fa, code, n, [(0, 0)])


# ---------------------------------------------------------------- convert.hip: blends and points2position
@pytest.mark.parametrize("alias", [False, True], ids=["apart", "out_is_A"])
def test_blends_stride_under_a_lowered_cap(fa, capped, alias):
    """blend_kernel for float and double and undefined_kernel (BLEND_LINEAR_NO_EXTRAPOL outside [a, b]): stream_blocks wants 13
    workgroups for these n, gets 2."""
    n = 4 * 1024 * 3 + 5
    A32, B32 = cases.field(1, 1, n, seed=1, nan_frac=0.02)[0, 0], cases.field(1, 1, n, seed=2, nan_frac=0.02)[0, 0]
    rng = np.random.default_rng(3)
    A64, B64 = rng.normal(0, 5, n), rng.normal(3, 5, n)
    A64[::501] = np.nan
    runs = [(A32, B32, lambda a, b, o: fa.get_values_1d_device(fa.BLEND_LINEAR, a, b, o, n, 2., 5., 3., _stream()),
             oracle.get_values_1d(oracle.BLEND_LINEAR, A32, B32, 2., 5., 3.)[0]),
            (A64, B64, lambda a, b, o: fa.get_values_linear_d_device(a, b, o, n, 2., 5., 3., _stream()),
             oracle.get_values_linear_d(A64, B64, 2., 5., 3.)),
            (A32, B32, lambda a, b, o: fa.get_values_1d_device(fa.BLEND_LINEAR_NO_EXTRAPOL, a, b, o, n, 2., 5., 6., _stream()),
             oracle.get_values_1d(oracle.BLEND_LINEAR_NO_EXTRAPOL, A32, B32, 2., 5., 6.)[0])]
    assert np.isnan(runs[2][3]).all() and not np.isnan(runs[0][3]).all()
    for A, B, call, want in runs:
        dA, dB = _Guarded(A.dtype, n, 0, A), _Guarded(B.dtype, n, 0, B)
        out = dA if alias else _Guarded(A.dtype, n, 0)
        call(dA.ptr, dB.ptr, out.ptr)
        got = out.result()
        assert _same_bits(got, want), int((_bits(got) != _bits(want)).sum())
        assert _same_bits(dB.result(), B)


def _p2p_cases(n, seed):
    rng = np.random.default_rng(seed)
    for axis, typ, lo, hi in ((np.linspace(-5, 5, 41), oracle.PROJ_AXIS, -8, 8),
                              (np.radians(np.arange(-180, 180, 1.0)), oracle.LONGITUDE, -8, 8)):   # ascending; circular
        p = rng.uniform(lo, hi, n)
        hits = np.arange(0, n, 97)
        p[hits] = axis[rng.integers(0, axis.size, hits.size)]
        p[5], p[6], p[7] = np.nan, np.inf, -np.inf
        p[-3:] = [np.nan, axis[3], hi]   # the last pass holds every kind as well
        yield p, axis, typ


def _check_points2position(fa, n, cases_):
    for p, axis, typ in cases_:
        g = _Guarded(np.float64, n, 0, p)
        fa.points2position_device(g.ptr, n, axis, typ, _stream())
        got, want = g.result(), oracle.points2position(p, axis, typ)
        assert _same_bits(got, want), (typ, int((_bits(got) != _bits(want)).sum()))
        assert (want == -999.).any() and (want == np.round(want)).sum() > n // 200


# launch_points2position: ceil(n / 256) workgroups, capped
def test_points2position_strides_under_a_lowered_cap(fa, capped):
    n = 3 * S + 5
    _check_points2position(fa, n, _p2p_cases(n, 4))


def test_points2position_strides_under_the_product_launch_rule(fa):
    n = 2 * L + 77
    _check_points2position(fa, n, list(_p2p_cases(n, 5))[1:])


# ---------------------------------------------------------------- projection.hip
def _values_input(src, n, seed):
    rng = np.random.default_rng(seed)
    lon0 = 15.0 if src == GEO_W else 10.0   # UTM 33: within 12 degrees of its meridian
    return np.radians(rng.uniform(lon0 - 12, lon0 + 12, n)), np.radians(rng.uniform(40, 80, n))


PAIRS = [(GEO, STERE_OBL), (GEO_W, UTM33)]   # one spherical and one ellipsoidal pair of test_gpu_projection.py


def _check_project_values(fa, src, dst, n, first):
    lon, lat = _values_input(src, n, seed=n)
    x, y = fa.project_values_host(src, dst, lon, lat)
    wx, wy = po.transform(src, dst, lon, lat)
    _close(x, wx, dst); _close(y, wy, dst)
    tx, ty = fa.project_values_host(src, dst, lon[first:], lat[first:])   # the same points as the first lanes of a call
    bad = np.flatnonzero((_bits(x[first:]) != _bits(tx)) | (_bits(y[first:]) != _bits(ty)))
    assert bad.size == 0, "index %d and %d more differ from a call on the points from %d on" % (first + bad[0], bad.size - 1, first)


def _check_project_axes(fa, src, dst, ax, ay, first):
    gx, gy = fa.project_axes_host(src, dst, ax, ay)
    wx, wy = po.project_axes(src, dst, ax, ay)
    assert gx.shape == (ay.size, ax.size)
    _close(gx.ravel(), wx, dst); _close(gy.ravel(), wy, dst)
    row = -(-first // ax.size)   # the rows that lie wholly at flat indices >= first, as a mesh of their own
    tx, ty = fa.project_axes_host(src, dst, ax, ay[row:])
    bad = np.flatnonzero((_bits(gx[row:]) != _bits(tx)).ravel() | (_bits(gy[row:]) != _bits(ty)).ravel())
    assert bad.size == 0, "index %d and %d more differ from a call on the rows from %d on" % (row * ax.size + bad[0], bad.size - 1, row)


def _check_matrix(fa, ox, oy):
    xa, ya = np.linspace(-25, 25, ox), np.linspace(52, 78, oy)
    got = fa.get_vector_reproject_matrix_host(STERE, GEO, xa, ya, 1, 2).reshape(-1, 4)
    want = _rotation_matrix(STERE, GEO, xa, ya, 1, 2).reshape(-1, 4)
    np.testing.assert_allclose(got[:, :3], want[:, :3], atol=2e-6)   # the bounds of test_vector_reproject_matrix_on_the_gpu
    np.testing.assert_allclose(np.hypot(got[:, 0], got[:, 1]), 1.0, atol=1e-14)
    np.testing.assert_array_equal(got[:, 2], -got[:, 1])
    np.testing.assert_allclose(np.cos(got[:, 3]), got[:, 0], atol=1e-15)


BOX_STERE = "+proj=stere +lat_0=90 +lon_0=0 +lat_ts=60 +a=6.371e+06 +e=0"
BOX_LONLAT = "+proj=latlong +R=6.371e6"


def _check_bounding_box(fa, nx, ny, rows_of_first_pass):
    """A box that keeps part of the columns and the rows at the far end of the y axis, which only later passes reach."""
    x, y = np.linspace(-1.6e6, 1.4e6, nx), np.linspace(-0.5e6, -1.72e6, ny)   # away from the pole: the last rows are the widest
    lon, lat = po.project_axes(BOX_STERE, BOX_LONLAT, x, y)
    lon, lat = np.degrees(lon).reshape(ny, nx), np.degrees(lat).reshape(ny, nx)
    box = (70.03, 83.01, -20.02, 35.01)
    assert extract_ref.bound_distance(lon, lat, *box) > 1e-9   # no point within rounding of a bound
    wantX, wantY = extract_ref.bounding_box(lon, lat, *box)
    firstX, firstY = extract_ref.bounding_box(lon[:rows_of_first_pass], lat[:rows_of_first_pass], *box)
    assert 0 < wantX.size < nx and 0 < wantY.size < ny and wantY[-1] == ny - 1
    assert firstX.size < wantX.size and firstY.size < wantY.size   # columns and rows that only the later passes find
    gx, gy = fa.extract_bounding_box_host(BOX_STERE, BOX_LONLAT, x, y, *box)
    assert np.array_equal(gx, wantX) and np.array_equal(gy, wantY)


# point_blocks(n): ceil(n / 256) workgroups, capped
@pytest.mark.parametrize("src,dst", PAIRS, ids=["sphere", "ellipsoid"])
def test_project_values_strides_under_a_lowered_cap(fa, capped, src, dst):
    _check_project_values(fa, src, dst, 3 * S + 5, first=S)


@pytest.mark.parametrize("src,dst", PAIRS, ids=["sphere", "ellipsoid"])
def test_project_values_strides_under_the_product_launch_rule(fa, src, dst):
    _check_project_values(fa, src, dst, 2 * L + 77, first=L)


def test_project_axes_strides_under_a_lowered_cap(fa, capped):
    """37 x 43 = 1591 mesh points: i % ix and i / ix in a fourth pass."""
    _check_project_axes(fa, LCC, ROT, np.linspace(-9e5, 9e5, 37), np.linspace(-7e5, 8e5, 43), first=S)


def test_project_axes_strides_under_the_product_launch_rule(fa):
    """1031 x 1021: both lengths odd, ix * iy > 2 L."""
    _check_project_axes(fa, LCC, ROT, np.linspace(-9e5, 9e5, 1031), np.linspace(-7e5, 8e5, 1021), first=L)


def test_vector_matrix_strides_under_a_lowered_cap(fa, capped):
    _check_matrix(fa, 37, 43)


def test_vector_matrix_strides_under_the_product_launch_rule(fa):
    """1031 x 521 > L: project_axes_kernel and vector_matrix_kernel (outX[i % ox], outY[i / ox]) in a second pass.  The delta of the
    finite differences comes from cells at the origin and in the middle of the whole mesh, so a call on the later rows alone is
    another operation: the oracle on the whole mesh is the check here."""
    _check_matrix(fa, 1031, 521)


def test_bounding_box_strides_under_a_lowered_cap(fa, capped):
    """nx = 70: two wave tiles per row, the second of 6 lanes; 82 waves against the 8 of two workgroups."""
    _check_bounding_box(fa, 70, 41, rows_of_first_pass=4)


def test_bounding_box_strides_under_the_product_launch_rule(fa):
    """17 * 521 = 8857 waves against the 8192 of a capped grid: the last 40 rows belong to the second pass."""
    _check_bounding_box(fa, 1031, 521, rows_of_first_pass=8192 // 17)


# ---------------------------------------------------------------- coordsearch.hip
def _check_nearest(fa, qlon, qlat, lon, lat, some_unmatched=True):
    nx = lon.shape[1]
    assert abs(fa.grid_distance_host(lon, lat) - oracle.grid_distance(lon, lat)) < 1e-12
    gx, gy = fa.coord_nearest_host(qlon, qlat, lon, lat)
    wx, wy = oracle.fast_translate_points(qlon, qlat, lon, lat)

    def metric(i, x, y):
        k = (y * nx + x).astype(int)
        return _great_circle_cos(qlon[i], qlat[i], lon.ravel()[k], lat.ravel()[k])
    assert _same_cells_or_ties(gx, gy, wx, wy, metric, -1) < 0.02
    assert (gx >= 0).any() and (gx == -1).any() == some_unmatched
    return gx, gy


def _check_kdtree(fa, maxDist, qlon, qlat, lon, lat, some_unmatched=True):
    nx = lon.shape[1]
    gx, gy = fa.coord_kdtree_host(maxDist, qlon, qlat, lon, lat)
    wx, wy = oracle.flann_translate_points(maxDist, qlon, qlat, lon, lat)

    def metric(i, x, y):
        k = (y * nx + x).astype(int)
        return ((_xyz(qlon[i], qlat[i]) - _xyz(lon.ravel()[k], lat.ravel()[k])) ** 2).sum(-1)
    assert _same_cells_or_ties(gx, gy, wx, wy, metric, -1000) < 0.02
    assert (gx >= 0).any() and (gx == -1000).any() == some_unmatched
    return gx, gy


def _queries_around(lon, lat, n, seed, margin=0.004):
    rng = np.random.default_rng(seed)
    qlon = rng.uniform(np.nanmin(lon) - margin, np.nanmax(lon) + margin, n)
    qlat = rng.uniform(np.nanmin(lat) - margin, np.nanmax(lat) + margin, n)
    qlon[:3] = [np.nan, 0.1, 0.2]; qlat[:3] = [1.0, np.nan, 3.0]
    return qlon, qlat


def _fine_grid(nx, ny, seed, jitter=0.3):
    """_curvilinear_grid with a spacing at which 1031 x 521 cells stay between 50 and 63 degrees north."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    u = (i + jitter * rng.uniform(-1, 1, i.shape)) * 0.012
    v = (j + jitter * rng.uniform(-1, 1, i.shape)) * 0.02
    lon, lat = np.radians(5 + 0.9 * u - 0.3 * v), np.radians(50 + 0.35 * u + 0.8 * v)
    lon.reshape(-1)[rng.choice(lon.size, 5, replace=False)] = np.nan
    return lon, lat


# blocks_for(n): ceil(n / 256) workgroups, capped, for the source cells and for the queries
def test_coordinate_search_strides_under_a_lowered_cap(fa, capped):
    """2700 source cells and 3000 queries on two workgroups: source_keys_kernel, source_points_kernel and nearest_kernel all stride."""
    lon, lat = _curvilinear_grid(60, 45, seed=9, nan=5)
    qlon, qlat = _queries_around(lon, lat, 3000, seed=10)
    _check_nearest(fa, qlon, qlat, lon, lat)
    _check_kdtree(fa, 3000.0, qlon, qlat, lon, lat)


def test_coordinate_search_with_a_source_beyond_one_pass(fa):
    """1031 x 521 = 537 151 cells > L: keys and points of the cells past L come from a second pass; a cell that pass left out
    would be missing from the answers of the queries around it."""
    lon, lat = _fine_grid(1031, 521, seed=1)
    assert np.degrees(lat.min()) > 49.9 and np.degrees(lat.max()) < 63
    rng = np.random.default_rng(2)
    near = np.concatenate([rng.integers(L, lon.size, 450), rng.integers(0, lon.size, 450)])   # half of them around cells past L
    qlon, qlat = _queries_around(lon, lat, 1000, seed=3, margin=0.01)
    qlon[100:] = lon.ravel()[near] + rng.normal(0, 1e-4, near.size) / np.cos(lat.ravel()[near])
    qlat[100:] = lat.ravel()[near] + rng.normal(0, 1e-4, near.size)
    for gx, gy in (_check_nearest(fa, qlon, qlat, lon, lat), _check_kdtree(fa, 1200.0, qlon, qlat, lon, lat)):
        assert (gy[gx >= 0] * lon.shape[1] + gx[gx >= 0] >= L).sum() > 100   # answers among the cells of the second pass


def test_coordinate_search_with_queries_beyond_one_pass(fa):
    """L + L / 2 + 77 queries on 30 x 20 cells: the second pass of nearest_kernel ends inside the grid."""
    lon, lat = _curvilinear_grid(30, 20, seed=7, nan=5)
    qlon, qlat = _queries_around(lon, lat, L + L // 2 + 77, seed=8)
    for gx, gy in (_check_nearest(fa, qlon, qlat, lon, lat), _check_kdtree(fa, 3000.0, qlon, qlat, lon, lat)):
        assert (gx[L:] >= 0).any() and (gx[L:] < 0).any()


@pytest.mark.parametrize("case", coord_search_inputs(), ids=lambda c: c[0])
def test_coordinate_search_where_cubes_and_a_latitude_walk_could_disagree(fa, case):
    """The date line with queries on either branch of the longitude, both polar caps with a cell at the pole, a global grid with its
    pole rows, 1000 and 1001 cells (the sampling rule of the grid distance), and the kd search with 2^20 cubes per axis and matches
    present.  tests/test_oracle_props.py checks on the CPU that each input holds this and that the oracle alone stays within the 2 %."""
    name, lon, lat, qlon, qlat, maxDist, nn = case
    some_unmatched = not name.startswith("global")   # no point of the sphere is out of reach of the global grid
    _check_kdtree(fa, maxDist, qlon, qlat, lon, lat, some_unmatched)
    if nn:
        _check_nearest(fa, qlon, qlat, lon, lat, some_unmatched)


def test_coordinate_search_on_one_cell(fa):
    """src/CDMInterpolator.cc:1121-1123: acos(-2) as the region of influence, so COORD_NN finds nothing, not even the cell itself;
    library and oracle both follow the reference.  The kd-tree method finds the cell."""
    lon, lat = np.array([[0.2]]), np.array([[1.0]])
    qlon, qlat = np.array([0.2, 0.2001, 3.0]), np.array([1.0, 1.0001, -1.0])
    assert np.isnan(fa.grid_distance_host(lon, lat)) and np.isnan(oracle.grid_distance(lon, lat))
    for px, py in (fa.coord_nearest_host(qlon, qlat, lon, lat), oracle.fast_translate_points(qlon, qlat, lon, lat)):
        assert np.all(px == -1) and np.all(py == -1)
    for kx, ky in (fa.coord_kdtree_host(5000.0, qlon, qlat, lon, lat), oracle.flann_translate_points(5000.0, qlon, qlat, lon, lat)):
        assert kx.tolist() == [0, 0, -1000] and ky.tolist() == [0, 0, -1000]
