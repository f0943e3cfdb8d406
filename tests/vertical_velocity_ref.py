"""CPU restatement of the reference's vertical velocity on model levels, the yardstick of tests/test_gpu_vertical_velocity.py.
Not a test.

  griddistance            mifi_griddistance, src/interpolation.c:1539-1595 (numpy's sin / cos / arccos: compared with a tolerance)
  vertical_velocity       mifi_compute_vertical_velocity, :1597-1773, float64 throughout in the reference's operation order, the C
                          library's log (vertical_levels_ref.c_log), rounded to float32 where the reference stores a float
  omega_to_vertical_wind  mifi_omega_to_vertical_wind_f, src/vertical_coordinate_transformations.c:195-209, all in float32
tests/test_vertical_velocity_ref.py pins the three to the reference's object code (oracle/_ref/libmifi_ref.so, bound here with ctypes
by reference_lib) and to tests/golden/vertical_velocity_answers.npz.
"""
import ctypes
import os

import numpy as np

import vertical_levels_ref as vl

f32, f64 = np.float32, np.float64

DEG_TO_RAD = .017453292519943296                 # oracle/ref_shim/proj_api.h
EARTH_RADIUS_M = 6371000.0                       # MIFI_EARTH_RADIUS_M
R_DRY_AIR = 8.31432 / 0.0289644                  # MIFI_GAS_CONSTANT / MIFI_MOLAR_MASS_DRY_AIR
G = 9.80665                                      # MIFI_EARTH_GRAVITY
MR_G = f32(-(8.31432 / (9.80665 * 0.0289644)))   # (float)-BAROMETRIC_FACTOR
OK, ERROR = 1, -1

FIXTURE = "vertical_velocity_answers.npz"


# ------------------------------------------------------------------ grid distance
def _great_circle_m(lon, lat, p, q):
    la0, lo0, la1, lo1 = DEG_TO_RAD * lat[p], DEG_TO_RAD * lon[p], DEG_TO_RAD * lat[q], DEG_TO_RAD * lon[q]
    with np.errstate(invalid="ignore"):
        return (EARTH_RADIUS_M * np.arccos(np.sin(la0) * np.sin(la1) + np.cos(la0) * np.cos(la1) * np.cos(lo1 - lo0))).astype(f32)


def griddistance(lon, lat):
    """lon, lat float64 [ny][nx] in degrees -> (gridDistX, gridDistY float32 [ny][nx], return code).  The copies into the last column
    and the last row run in the reference's order, one element after the other."""
    lon, lat = np.ascontiguousarray(lon, f64), np.ascontiguousarray(lat, f64)
    ny, nx = lon.shape
    n = nx * ny
    lo, la = lon.reshape(-1), lat.reshape(-1)
    gx, gy = np.zeros(n, f32), np.zeros(n, f32)
    if n == 1:
        return gx.reshape(ny, nx), gy.reshape(ny, nx), ERROR
    if nx == 1 or ny == 1:
        p = np.arange(n - 1)
        gx[:-1] = _great_circle_m(lo, la, p, p + 1)
        gy[:-1] = gx[:-1]
        gx[n - 1], gy[n - 1] = gx[n - 2], gy[n - 2]
        return gx.reshape(ny, nx), gy.reshape(ny, nx), OK
    jj, ii = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    p = (ii + nx * jj).reshape(-1)
    gx[p] = _great_circle_m(lo, la, p, p + 1)
    gy[p] = _great_circle_m(lo, la, p, p + nx)
    for j in range(ny):  # last column
        p = j * nx + (nx - 1)
        gx[p], gy[p] = gx[p - 1], gy[p - 1]
    for i in range(nx):  # last row, overwriting the corner: p - ny, not p - nx
        p = (ny - 1) * nx + i
        gx[p], gy[p] = gx[p - ny], gy[p - ny]
    return gx.reshape(ny, nx), gy.reshape(ny, nx), OK


def griddistance_tolerance(want):
    """|got - want| <= 2^-23 |want| + 6371000 * 2^-49 / sin(want / 6371000): one float step, and the conditioning of acos near 1 for an
    argument that carries a few units in the last place from sin and cos."""
    w = np.asarray(want, f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2.0 ** -23 * np.abs(w) + EARTH_RADIUS_M * 2.0 ** -49 / np.sin(w / EARTH_RADIUS_M)


# ------------------------------------------------------------------ vertical velocity
def half_levels(ap, b):
    """:1653-1663."""
    nz = len(ap)
    ah, bh = np.zeros(nz + 1), np.zeros(nz + 1)
    bh[nz] = 1.0
    for k in range(nz - 1, 0, -1):
        ah[k] = 2.0 * ap[k] - ah[k + 1]
        bh[k] = 2.0 * b[k] - bh[k + 1]
    return ah, bh


def _borders(a):
    """:1747-1758 on one level [ny][nx]: the rows first, then the columns over every j."""
    a[0, 1:-1] = a[1, 1:-1]
    a[-1, 1:-1] = a[-2, 1:-1]
    a[:, 0] = a[:, 1]
    a[:, -1] = a[:, -2]


def vertical_velocity(dx, dy, gridDistX, gridDistY, ap, b, zs, ps, u, v, t, log=vl.c_log):
    """gridDistX, gridDistY, zs float32 [ny][nx]; ap, b float64 [nz]; ps float32 [nt][ny][nx]; u, v, t float32 [nt][nz][ny][nx] ->
    (w float32 [nt][nz][ny][nx], M float64 of the same shape): M is the magnitude of the terms that cancel in w,
    (|R t dlnp sum / dp| + |R t alfa div / dp| + |rhx rdx_2| (|z+| + |z-|) + |rhy rdy_2| (|z+| + |z-|)) / g, with the border copies."""
    u, v, t = (np.ascontiguousarray(a, f32) for a in (u, v, t))
    nt, nz, ny, nx = t.shape
    assert nx >= 3 and ny >= 3 and nz >= 1, "the reference reads outside its arrays"
    ap, b = np.ascontiguousarray(ap, f64), np.ascontiguousarray(b, f64)
    ps = np.ascontiguousarray(ps, f32).reshape(nt, ny, nx)
    zs = np.ascontiguousarray(zs, f32).reshape(ny, nx).astype(f64)
    w = np.zeros((nt, nz, ny, nx), f32)
    M = np.zeros((nt, nz, ny, nx), f64)
    I = (slice(1, -1), slice(1, -1))
    xm, xp = (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None))
    ym, yp = (slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1))
    with np.errstate(all="ignore"):
        rdx_2, rdy_2 = 1 / (2 * dx), 1 / (2 * dy)
        mapRatioX = np.ascontiguousarray(gridDistX, f32).reshape(ny, nx).astype(f64) / dx
        mapRatioY = np.ascontiguousarray(gridDistY, f32).reshape(ny, nx).astype(f64) / dy
        rhx, rhy = 1 / mapRatioX, 1 / mapRatioY
        rhxy = rhx * rhy
        ah, bh = half_levels(ap, b)
        for it in range(nt):
            p = ps[it].astype(f64)
            dp, dlnp, alfa = np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx))
            dp[0] = (ah[1] - ah[0]) + (bh[1] - bh[0]) * p
            alfa[0] = np.log(2.)
            for k in range(1, nz):
                pm = ah[k] + bh[k] * p
                pp = ah[k + 1] + bh[k + 1] * p
                dp[k] = pp - pm
                dlnp[k] = log(pp / pm)
                alfa[k] = 1. - pm * dlnp[k] / dp[k]
            z = np.zeros((nz, ny, nx))
            total = zs * G
            for k in range(nz - 1, -1, -1):
                rt = R_DRY_AIR * t[it, k].astype(f64)
                z[k] = total + rt * alfa[k]
                total = total + rt * dlnp[k]
            total = np.zeros((ny, nx))
            for k in range(1, nz):
                uu = mapRatioY * u[it, k].astype(f64) * dp[k]
                vv = mapRatioX * v[it, k].astype(f64) * dp[k]
                div = rhxy[I] * (rdx_2 * (uu[xp] - uu[xm]) + rdy_2 * (vv[yp] - vv[ym]))
                rt = R_DRY_AIR * t[it, k][I].astype(f64)
                w1 = rt * (dlnp[k][I] * total[I] + alfa[k][I] * div) / dp[k][I]
                w2 = rhx[I] * rdx_2 * (z[k][xp] - z[k][xm]) + rhy[I] * rdy_2 * (z[k][yp] - z[k][ym])
                w[it, k][I] = ((w1 + w2) / G).astype(f32)
                M[it, k][I] = (np.abs(rt * dlnp[k][I] * total[I] / dp[k][I]) + np.abs(rt * alfa[k][I] * div / dp[k][I])
                               + np.abs(rhx[I] * rdx_2) * (np.abs(z[k][xp]) + np.abs(z[k][xm]))
                               + np.abs(rhy[I] * rdy_2) * (np.abs(z[k][yp]) + np.abs(z[k][ym]))) / G
                total[I] = total[I] + div
                _borders(w[it, k])
                _borders(M[it, k])
    return w, M


def velocity_tolerance(want, M, nz):
    """|got - want| <= 2^-23 |want| + nz * 2^-50 * M: the device's log differs from the host's by a couple of units in the last
    place (2^-51 relative); the error enters z once per level below the cell and w multiplied by what M collects; the rounding to
    float adds one float step."""
    with np.errstate(invalid="ignore"):
        return 2.0 ** -23 * np.abs(np.asarray(want, f64)) + nz * 2.0 ** -50 * M


# ------------------------------------------------------------------ omega
def omega_to_vertical_wind(omega, p, t):
    """float32 arrays of one shape: ((mR_g * omega) * t) / p in float32."""
    with np.errstate(all="ignore"):
        return (((MR_G * np.asarray(omega, f32)).astype(f32) * np.asarray(t, f32)).astype(f32) / np.asarray(p, f32)).astype(f32)


# ------------------------------------------------------------------ the reference's object code
_F = ctypes.POINTER(ctypes.c_float)
_D = ctypes.POINTER(ctypes.c_double)
_Z = ctypes.c_size_t


class ReferenceLib:
    """mifi_griddistance, mifi_compute_vertical_velocity and mifi_omega_to_vertical_wind_f of oracle/_ref/libmifi_ref.so."""

    def __init__(self, path):
        L = self.lib = ctypes.CDLL(path)
        L.mifi_griddistance.argtypes = [_Z, _Z, _D, _D, _F, _F]
        L.mifi_griddistance.restype = ctypes.c_int
        L.mifi_compute_vertical_velocity.argtypes = [_Z, _Z, _Z, ctypes.c_double, ctypes.c_double, _F, _F, _D, _D, _F, _F, _F, _F, _F, _F]
        L.mifi_compute_vertical_velocity.restype = _Z
        L.mifi_omega_to_vertical_wind_f.argtypes = [_Z, _F, _F, _F, _F]
        L.mifi_omega_to_vertical_wind_f.restype = ctypes.c_int

    def griddistance(self, lon, lat):
        lon, lat = np.ascontiguousarray(lon, f64), np.ascontiguousarray(lat, f64)
        ny, nx = lon.shape
        gx, gy = np.full((ny, nx), -1.0, f32), np.full((ny, nx), -1.0, f32)
        rc = self.lib.mifi_griddistance(nx, ny, lon.ctypes.data_as(_D), lat.ctypes.data_as(_D), gx.ctypes.data_as(_F), gy.ctypes.data_as(_F))
        return gx, gy, rc

    def vertical_velocity(self, dx, dy, gridDistX, gridDistY, ap, b, zs, ps, u, v, t):
        """One call per time step, as CDMProcessor::getDataSlice makes them."""
        a32 = lambda a: np.ascontiguousarray(a, f32)
        gridDistX, gridDistY, zs, ps, u, v, t = (a32(a) for a in (gridDistX, gridDistY, zs, ps, u, v, t))
        ap, b = np.ascontiguousarray(ap, f64), np.ascontiguousarray(b, f64)
        nt, nz, ny, nx = t.shape
        assert nx >= 3 and ny >= 3 and nz >= 1, "the reference reads outside its arrays"
        ps = ps.reshape(nt, ny, nx)
        w = np.full((nt, nz, ny, nx), -12345.0, f32)
        fp = lambda a: a.ctypes.data_as(_F)
        for it in range(nt):
            rc = self.lib.mifi_compute_vertical_velocity(nx, ny, nz, dx, dy, fp(gridDistX), fp(gridDistY), ap.ctypes.data_as(_D),
                                                         b.ctypes.data_as(_D), fp(zs), fp(ps[it]), fp(u[it]), fp(v[it]), fp(t[it]), fp(w[it]))
            assert rc == OK
        return w

    def omega_to_vertical_wind(self, omega, p, t):
        omega, p, t = (np.ascontiguousarray(a, f32) for a in (omega, p, t))
        w = omega.copy()  # in place, as OmegaVerticalConverter::getDataSlice
        fp = lambda a: a.ctypes.data_as(_F)
        rc = self.lib.mifi_omega_to_vertical_wind_f(w.size, fp(w), fp(p), fp(t), fp(w))
        assert rc == OK
        return w


def reference_lib():
    """The ReferenceLib of oracle/_ref/libmifi_ref.so, or None where build() found no reference tree to compile it from."""
    import oracle
    return ReferenceLib(oracle.ref().path) if oracle.ref() is not None else None


# ------------------------------------------------------------------ cases
def make_grid(seed, nx, ny, lat0=60.0, spacing=0.025):
    """A perturbed curvilinear lon / lat grid in degrees: spacing of at least 0.01 degrees between neighbours, no duplicate points."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(ny, dtype=f64), np.arange(nx, dtype=f64), indexing="ij")
    wob = 0.2 * spacing
    lon = 10.0 + spacing * i + wob * np.sin(0.7 * j + 0.3 * i) + 0.1 * spacing * rng.uniform(-1, 1, (ny, nx))
    lat = lat0 + spacing * j + wob * np.cos(0.5 * i - 0.2 * j) + 0.1 * spacing * rng.uniform(-1, 1, (ny, nx))
    return lon, lat


def hybrid_coefficients(nz):
    """Full-level ap (Pa) and b, index 0 at the top, as means of half levels that start at p = 0 and end at ps."""
    eh = np.arange(nz + 1, dtype=f64) / nz
    ahh, bhh = 40000.0 * eh * (1 - eh), eh ** 2
    return 0.5 * (ahh[:-1] + ahh[1:]), 0.5 * (bhh[:-1] + bhh[1:])


def make_case(seed, nx, ny, nz, nt=1, nan_frac=0.0, spacing=0.025):
    """Smooth terrain, surface pressure, wind and temperature on a perturbed grid, so that w1 and w2 cancel as they do in real data.
    Returns a dict of the arguments of vertical_velocity (plus lon, lat).  nan_frac: share of NaN in t and u."""
    rng = np.random.default_rng(seed)
    lon, lat = make_grid(seed, nx, ny, spacing=spacing)
    gx, gy, _ = griddistance(lon, lat)
    dx = dy = float(np.median(gy[:-1]))
    j, i = np.meshgrid(np.arange(ny, dtype=f64), np.arange(nx, dtype=f64), indexing="ij")
    ph = rng.uniform(0, 2 * np.pi, 8)
    hill = lambda a, b_, c: np.sin(a * i + ph[c]) * np.cos(b_ * j + ph[c + 1])
    zs = 600.0 + 500.0 * hill(0.11, 0.17, 0) + 80.0 * hill(0.45, 0.38, 2)
    tt = np.arange(nt, dtype=f64)[:, None, None]
    ps = 101325.0 * np.exp(-zs[None] / 8000.0) + 300.0 * np.sin(0.05 * i + 0.08 * j + 0.6 * tt + ph[4])[...]
    eta = ((np.arange(nz) + 0.5) / nz)[None, :, None, None]
    wave = np.sin(0.06 * i + 0.09 * j + ph[5])[None, None] + 0.0 * eta
    t = 215.0 + 70.0 * eta + 3.0 * wave + 0.5 * np.cos(0.21 * i - 0.13 * j + tt + ph[6])[:, None]
    u = 25.0 * (1.2 - eta) * np.cos(0.07 * j + ph[7])[None, None] + 2.0 * np.sin(0.19 * i + 0.4 * tt)[:, None] * (1 + eta)
    v = 10.0 * (1.2 - eta) * np.sin(0.05 * i + ph[3])[None, None] + 1.5 * np.cos(0.23 * j - 0.3 * tt)[:, None] * (1 + eta)
    ap, b = hybrid_coefficients(nz)
    t, u, v = (np.ascontiguousarray(np.broadcast_to(a, (nt, nz, ny, nx)), f32) for a in (t, u, v))
    if nan_frac:
        t[rng.uniform(size=t.shape) < nan_frac] = np.nan
        u[rng.uniform(size=u.shape) < nan_frac] = np.nan
    return dict(lon=lon, lat=lat, dx=dx, dy=dy, gridDistX=gx, gridDistY=gy, ap=ap, b=b, zs=zs.astype(f32), ps=ps.astype(f32), u=u, v=v, t=t)


VELOCITY_ARGS = ("dx", "dy", "gridDistX", "gridDistY", "ap", "b", "zs", "ps", "u", "v", "t")


def velocity_args(case):
    return [case[k] for k in VELOCITY_ARGS]


def make_omega_case(seed, kind, nx, ny, nz, nt):
    """(vertical_ref.Levels in hPa of `kind`, omega in hPa/s, t) with a NaN and a zero pressure among the cells."""
    lv, T, _, _, _ = vl.make_atmosphere(seed, kind, nx, ny, nt, nz, False)
    rng = np.random.default_rng(seed + 1000)
    omega = rng.normal(0.0, 0.02, T.shape).astype(f32)
    omega[0, 0, 0, 1] = np.nan
    T[0, nz - 1, 1, 0] = np.nan
    omega[0, 0, 1, 1] = 0.0
    if lv.field is not None:
        lv.field[0, 0, 1, 1:3] = 0.0
    elif lv.axis is not None:
        lv.axis[0] = 0.0
    else:  # ps = 0 in two columns and a coefficient that makes one of their levels zero
        lv.ps[0, 1, 1:3] = 0.0
        lv.ps[0, 2, 2] = np.nan
        if lv.sigma is not None:
            lv.sigma[0] = 1.0  # ptop + 1 * (0 - ptop)
        else:
            (lv.a if lv.a is not None else lv.ap)[0] = 0.0
    return lv, omega, T


# ------------------------------------------------------------------ the recorded fixture
# (name, nx, ny, nz, nan_frac) of the recorded vertical-velocity cases, (name, nx, ny) of the grids, nt = 1 throughout
RECORDED_VELOCITY = (("s7x5x4", 7, 5, 4, 0.0), ("s5x7x4", 5, 7, 4, 0.0), ("s3x3x2", 3, 3, 2, 0.0), ("s3x9x1", 3, 9, 1, 0.0),
                     ("s37x19x6", 37, 19, 6, 0.0), ("s37x19x6nan", 37, 19, 6, 0.01))
RECORDED_GRIDS = (("g13x4", 13, 4), ("g5x7", 5, 7), ("g7x5", 7, 5), ("g3x3", 3, 3), ("g1x9", 1, 9), ("g9x1", 9, 1), ("g1x1", 1, 1))
RECORDED_OMEGA = (7, 5, 6, 2)  # nx, ny, nz, nt of the omega case of every level kind


def recorded_velocity_case(name):
    i, (_, nx, ny, nz, nan_frac) = next((i, c) for i, c in enumerate(RECORDED_VELOCITY) if c[0] == name)
    return make_case(500 + i, nx, ny, nz, 1, nan_frac)


def load_fixture(golden_dir):
    with np.load(os.path.join(golden_dir, FIXTURE), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
