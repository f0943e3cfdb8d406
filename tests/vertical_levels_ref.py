"""CPU restatement of the reference's vertical level converters, the yardstick of tests/test_gpu_vertical_levels.py.  Not a test.

The functions of src/vertical_coordinate_transformations.c (virtual temperature :108-111, layer thickness :154-157, standard
altitude :94-106, standard pressure :79-91, ocean s-coordinates :159-176) with their operand types and rounding points, and the
loops around them: PressureIntegrationToAltitudeConverter.cc:185-208 (`integrate_cell` per column in plain Python with math.log,
`integrate` vectorised over columns, one numpy step per level), AltitudeHeightConverter.cc:87-105 (the topography term),
PressureToStandardAltitudeConverter / AltitudeStandardToPressureConverter (:33-41 each, on the inner converter's doubles) and
OceanSCoordinateGToDepthConverter.cc:66-107.  tests/test_vertical_levels_ref.py pins the functions to the reference's known
answers in tests/golden/vertical_transform_kats.json and the vectorised loop to the per-cell one.

Logarithms: `integrate` takes the C library's log (math.log) element by element, as the reference does and as `integrate_cell`
does, so that the two agree bit for bit; `layer_thickness`, `standard_altitude` and `standard_pressure` take numpy's.
"""
import math

import numpy as np

from vertical_ref import AXIS, FIELD, HYBRID_SIGMA, HYBRID_SIGMA_AP, SIGMA, level_field

EARTH_GRAVITY = 9.80665                                    # MIFI_EARTH_GRAVITY, include/fimex/mifi_constants.h:235
BAROMETRIC_FACTOR = 8.31432 / (EARTH_GRAVITY * 0.0289644)  # vertical_coordinate_transformations.c:73-74
Z_MOL_WEIGHT_RATIO = .60771704180064308681                 # :77
STANDARD_P, STANDARD_T = 1013.25, 288.15

AUTO = -1  # surfaceFirst: the reference's own rule

f32, f64 = np.float32, np.float64


def _c_log(x):
    """log() of the C library with its IEEE results where Python raises."""
    if x > 0.0:
        return math.log(x)  # +inf included
    if x == 0.0:
        return -math.inf
    return math.nan  # negative or NaN


_c_log_array = np.frompyfunc(_c_log, 1, 1)


def c_log(x):
    """math.log element by element on a float64 array."""
    x = np.asarray(x, f64)
    return np.array(_c_log_array(x), dtype=f64).reshape(x.shape)


# ------------------------------------------------------------------ the functions
def virtual_temperature(q, T):
    """mifi_virtual_temperature: float (1 + Z * q) * T with the product in double."""
    with np.errstate(all="ignore"):
        return ((1 + Z_MOL_WEIGHT_RATIO * np.asarray(q, f32).astype(f64)) * np.asarray(T, f32).astype(f64)).astype(f32)


def layer_thickness(p_low, p_high, T, log=np.log):
    """mifi_barometric_layer_thickness: the quotient in float, the rest in double, rounded to float once."""
    with np.errstate(all="ignore"):
        ratio = (np.asarray(p_low, f32) / np.asarray(p_high, f32)).astype(f32)
        return (log(ratio.astype(f64)) * np.asarray(T, f32).astype(f64) * BAROMETRIC_FACTOR).astype(f32)


def standard_altitude(p, log=np.log):
    """mifi_barometric_standard_altitude on doubles."""
    K = -BAROMETRIC_FACTOR * STANDARD_T
    with np.errstate(all="ignore"):
        return K * log(np.asarray(p, f64) / STANDARD_P)


def standard_pressure(h, exp=np.exp):
    """mifi_barometric_standard_pressure on doubles."""
    C = -1 / (BAROMETRIC_FACTOR * STANDARD_T)
    with np.errstate(all="ignore"):
        return STANDARD_P * exp(C * np.asarray(h, f64))


def ocean_s_g1_z(h, h_c, zeta, sigma, C):
    with np.errstate(all="ignore"):
        h_inv = 1 / np.asarray(h, f64)
        S = h_c * sigma + (h - h_c) * C
        return S + zeta * (1 + S * h_inv)


def ocean_s_g2_z(h, h_c, zeta, sigma, C):
    with np.errstate(all="ignore"):
        hph_c_inv = 1 / (np.asarray(h, f64) + h_c)
        S = hph_c_inv * (h_c * sigma + h * C)
        return zeta + (zeta + h) * S


# ------------------------------------------------------------------ level descriptions as the inner converter's doubles
def level_field_double(lv, nt, ny, nx):
    """What the inner converter's getDataSlice(...)->asDouble() holds: the formulas unrounded, a FIELD's floats or an AXIS's
    doubles as they are."""
    if lv.kind == FIELD:
        return lv.field.reshape(nt, lv.nz, ny, nx).astype(f64)
    if lv.kind == AXIS:
        return np.broadcast_to(lv.axis[None, :, None, None], (nt, lv.nz, ny, nx)).copy()
    ps = lv.ps.reshape(nt, 1, ny, nx).astype(f64)
    col = lambda c: c[None, :, None, None]
    with np.errstate(all="ignore"):
        if lv.kind == SIGMA:
            return lv.ptop + col(lv.sigma) * (ps - lv.ptop)
        if lv.kind == HYBRID_SIGMA:
            return (col(lv.a) * lv.p0) + (col(lv.b) * ps)
        if lv.kind == HYBRID_SIGMA_AP:
            return col(lv.ap) + (col(lv.b) * ps)
    raise ValueError("unknown level kind %r" % (lv.kind,))


def add_topography(values, topo, topoFactor):
    """AltitudeHeightConverter::getDataSlice on doubles [nt][nz][ny][nx]; topo float64 [ny][nx] or None."""
    if topo is None:
        return values
    with np.errstate(all="ignore"):
        return values + topoFactor * np.asarray(topo, f64)[None, None]


# ------------------------------------------------------------------ the integration
def surface_first(p, flag=AUTO):
    """start_high_p of PressureIntegrationToAltitudeConverter.cc:105-122 on the float pressure field [nt][nz][ny][nx]."""
    if flag != AUTO:
        return bool(flag)
    return bool(p[0, 0, 0, 0] > p[0, -1, 0, 0])


def integrate_cell(p, T, q, sap, sgp, up):
    """One column, :187-207: p, T, q (or None) are its nz float32 values.  Returns (altitudes as Python floats (doubles),
    the running sum of |layer thickness|)."""
    nz = len(p)
    a = float(f32(sgp)) / EARTH_GRAVITY
    p_low = f32(sap)
    alt, spread = [0.0] * nz, [0.0] * nz
    total = 0.0
    for i in range(nz):
        k = i if up else nz - 1 - i
        p_high = f32(p[k])
        Tv = f32(T[k])
        if q is not None:
            Tv = f32((1 + Z_MOL_WEIGHT_RATIO * float(f32(q[k]))) * float(Tv))
        with np.errstate(all="ignore"):
            ratio = f32(p_low / p_high)
        lt = f32(_c_log(float(ratio)) * float(Tv) * BAROMETRIC_FACTOR)
        a += float(lt)
        total += abs(float(lt))
        alt[k], spread[k] = a, total
        p_low = p_high
    return alt, spread


def integrate(p, T, q, sap, sgp, flag=AUTO):
    """The same for every column: p, T, q (or None) float32 [nt][nz][ny][nx]; sap, sgp float32 [nt][ny][nx].
    Returns (a float64 [nt][nz][ny][nx], the running sum of |layer thickness| float64, of the same shape)."""
    p, T = np.ascontiguousarray(p, f32), np.ascontiguousarray(T, f32)
    nt, nz, ny, nx = p.shape
    up = surface_first(p, flag)
    a = np.asarray(sgp, f32).reshape(nt, ny, nx).astype(f64) / EARTH_GRAVITY
    p_low = np.asarray(sap, f32).reshape(nt, ny, nx).copy()
    alt = np.empty(p.shape, f64)
    spread = np.empty(p.shape, f64)
    total = np.zeros((nt, ny, nx), f64)
    for i in range(nz):
        k = i if up else nz - 1 - i
        Tv = T[:, k] if q is None else virtual_temperature(q[:, k], T[:, k])
        lt = layer_thickness(p_low, p[:, k], Tv, log=c_log).astype(f64)
        with np.errstate(all="ignore"):
            a = a + lt
            total = total + np.abs(lt)
        alt[:, k], spread[:, k] = a, total
        p_low = p[:, k]
    return alt, spread


def altitude_field(lv, nt, ny, nx, T, q, sap, sgp, flag=AUTO, topo=None, topoFactor=-1.0):
    """fimex_amd_vertical_altitude_integrate_*: (float32 result, a, spread) for a vertical_ref.Levels pressure description."""
    a, spread = integrate(level_field(lv, nt, ny, nx), T, q, sap, sgp, flag)
    with np.errstate(all="ignore"):
        return add_topography(a, topo, topoFactor).astype(f32), a, spread


def standard_altitude_field(lv, nt, ny, nx, topo=None, topoFactor=-1.0):
    """(float32 result, the altitude before the topography term)."""
    alt = standard_altitude(level_field_double(lv, nt, ny, nx))
    with np.errstate(all="ignore"):
        return add_topography(alt, topo, topoFactor).astype(f32), alt


def standard_pressure_field(lv, nt, ny, nx, topo=None, topoFactor=1.0):
    """(float32 result, the level before the topography term): the topography joins the level (height -> altitude)."""
    h = level_field_double(lv, nt, ny, nx)
    with np.errstate(all="ignore"):
        return standard_pressure(add_topography(h, topo, topoFactor)).astype(f32), h


def ocean_depth_field(generation, s, C, depth_c, depth, eta, nt):
    """OceanSCoordinateGToDepthConverter::getDataSlice: float32 [nt][nz][ny][nx]; depth [ny][nx], eta [nt][ny][nx] or None."""
    depth = np.asarray(depth, f64)
    h = depth[None, None]
    zeta = np.asarray(eta, f64)[:, None] if eta is not None else np.zeros((nt, 1) + depth.shape)
    sig = np.asarray(s, f64)[None, :, None, None]
    cc = np.asarray(C, f64)[None, :, None, None]
    z = (ocean_s_g1_z if generation == 1 else ocean_s_g2_z)(h, depth_c, zeta, sig, cc)
    with np.errstate(all="ignore"):
        return (-1. * z).astype(f32)


# ------------------------------------------------------------------ test input
def make_atmosphere(seed, kind, nx, ny, nt, nz, surface_first, nan_frac=0.0):
    """A plausible atmosphere for the integration: (pressure levels as vertical_ref.Levels of `kind`, T, q, sap, sgp) with every
    pressure positive and sap (600 ... 1040 hPa, also the ps of the formula kinds: the same array) above the lowest level's
    pressure.  Level index 0 is next to the surface when surface_first.  nan_frac: share of NaN in T."""
    from vertical_ref import Levels
    rng = np.random.default_rng(seed)
    eta = (np.arange(nz) + 0.5) / nz                    # 0 = top, 1 = surface
    sap = (600.0 + 440.0 * rng.uniform(size=(nt, ny, nx))).astype(f32)
    sgp = (EARTH_GRAVITY * 3000.0 * (1040.0 - sap.astype(f64)) / 440.0 * rng.uniform(0.9, 1.1, (nt, ny, nx))).astype(f32)
    T = (210.0 + 80.0 * eta[None, :, None, None] + rng.normal(0, 2.0, (nt, nz, ny, nx))).astype(f32)
    q = (0.015 * eta[None, :, None, None] ** 3 * rng.uniform(0, 1, (nt, nz, ny, nx))).astype(f32)
    q[:, :, ::3, ::5] = 0.0
    if nan_frac:
        T[rng.uniform(size=T.shape) < nan_frac] = np.nan
    b = eta ** 2
    ap = 1000.0 * (eta - b) + 0.1                       # hPa; ap + b * ps < ps for every ps >= 600
    order = slice(None, None, -1) if surface_first else slice(None)
    T, q = T[:, order].copy(), q[:, order].copy()
    ap, b, eta = ap[order].copy(), b[order].copy(), eta[order].copy()
    if kind == HYBRID_SIGMA_AP:
        lv = Levels(kind, nz, ap=ap, b=b, ps=sap)
    elif kind == HYBRID_SIGMA:
        lv = Levels(kind, nz, a=ap / 1000.0, b=b, p0=1000.0, ps=sap)
    elif kind == SIGMA:
        lv = Levels(kind, nz, sigma=eta, ptop=0.1, ps=sap)
    elif kind == AXIS:
        lv = Levels(kind, nz, axis=5.0 + 585.0 * eta)  # below 590 hPa
    else:
        hybrid = level_field(Levels(HYBRID_SIGMA_AP, nz, ap=ap, b=b, ps=sap), nt, ny, nx).astype(f64)
        lv = Levels(FIELD, nz, field=hybrid * (1 - 1e-3 * rng.uniform(size=hybrid.shape)))
    return lv, T, q, sap, sgp
