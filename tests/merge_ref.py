"""CPU restatement of the reference's grid merging, line by line:

  linear_smoothing   CDMBorderSmoothing_Linear::operator()       src/CDMBorderSmoothing_Linear.cc:41-85
  border_smooth      CDMBorderSmoothing::getDataSlice, the loop  src/CDMBorderSmoothing.cc:129-139
  overlay            CDMOverlay::getDataSlice, the loop          src/CDMOverlay.cc:82-86
  extend_inner_axis  CDMMergerPrivate::extendInnerAxis           src/CDMMerger.cc:231-275
  merge              CDMMergerPrivate::makeCDM's reader chain    src/CDMMerger.cc:212-227

The size_t arithmetic of the smoothing is Python integers mod 2^64, the double arithmetic numpy float64 scalars (IEEE, one
operation per line of the reference), and every step rounds to float once, as the reference's float interpolation arrays and its
float / double variables with scale 1 and offset 0 do.  Test infrastructure: the product never imports it.
"""
import functools
import math
import os

import numpy as np

import oracle
from oracle import proj_oracle as po

M64 = (1 << 64) - 1
OUTER, INNER, EQUAL, BLEND = "outer", "inner", "equal", "blend"


def _dist(dx, dy):
    """:33-35, on doubles made from size_t differences"""
    dx, dy = np.float64(dx), np.float64(dy)
    return np.sqrt(dx * dx + dy * dy)


def linear_alpha(nx, ny, tw, bw, x, y):
    """-> (branch, alpha): the branch of :52-55 and, for the transition band, alpha of :59-83.  OUTER: valueO, INNER: valueI,
    BLEND: valueI + alpha * diff (or valueO where diff == 0)."""
    if nx == 0 or ny == 0:  # :43-44
        return OUTER, None
    xmin1 = bw & M64
    xmax1 = (xmin1 + tw) & M64  # :46
    ymin1 = bw & M64
    ymax1 = (ymin1 + tw) & M64  # :47
    xmax2 = (nx - bw) & M64
    xmin2 = (xmax2 - tw) & M64  # :48
    ymax2 = (ny - bw) & M64
    ymin2 = (ymax2 - tw) & M64  # :49
    if x < xmin1 or x >= xmax2 or y < ymin1 or y >= ymax2:  # :52
        return OUTER, None
    if x >= xmax1 and x < xmin2 and y >= ymax1 and y < ymin2:  # :54
        return INNER, None
    alpha = np.float64(0)  # :59
    if x < xmax1:  # :60
        if y < ymax1:
            alpha = _dist((xmax1 - x) & M64, (ymax1 - y) & M64)
        elif y >= ymin2:
            alpha = _dist((xmax1 - x) & M64, (y - ymin2) & M64)
        else:
            alpha = np.float64((xmax1 - x) & M64)
    elif x >= xmin2:  # :67
        if y < ymax1:
            alpha = _dist((x - xmin2) & M64, (ymax1 - y) & M64)
        elif y >= ymin2:
            alpha = _dist((x - xmin2) & M64, (y - ymin2) & M64)
        else:
            alpha = np.float64((x - xmin2) & M64)
    elif y < ymax1:  # :74
        alpha = np.float64((ymax1 - y) & M64)
    elif y >= ymin2:  # :76
        alpha = np.float64((y - ymin2) & M64)
    alpha = alpha / np.float64(tw)  # :79
    if alpha > 1:
        alpha = np.float64(1)
    elif alpha < 0:
        alpha = np.float64(0)
    return BLEND, alpha


def linear_smoothing(nx, ny, tw, bw, x, y, valueI, valueO):
    """operator()(curX, curY, valueI, valueO) on doubles -> (double, branch)"""
    valueI, valueO = np.float64(valueI), np.float64(valueO)
    branch, alpha = linear_alpha(nx, ny, tw, bw, x, y)
    if branch == OUTER:
        return valueO, OUTER
    if branch == INNER:
        return valueI, INNER
    with np.errstate(invalid="ignore"):
        diff = valueO - valueI  # :56
        if diff == 0:           # :57-58
            return valueO, EQUAL
        prod = alpha * diff     # :84, two operations
        return valueI + prod, BLEND


@functools.lru_cache(maxsize=64)
def _alpha_planes(nx, ny, tw, bw):
    """kind [ny][nx] (0 outer, 1 inner, 2 blend) and alpha [ny][nx] of every cell, from linear_alpha; shared, nobody writes to it"""
    kind = np.zeros((ny, nx), np.int8)
    alpha = np.zeros((ny, nx), np.float64)
    for y in range(ny):
        for x in range(nx):
            b, a = linear_alpha(nx, ny, tw, bw, x, y)
            kind[y, x] = 0 if b == OUTER else 1 if b == INNER else 2
            if b == BLEND:
                alpha[y, x] = a
    return kind, alpha


def border_smooth(inner, outer_on_inner, tw=5, bw=2, use_outer=True):
    """getDataSlice's loop on [nz][ny][nx] (or [ny][nx]) float fields -> float32, same shape.  Vectorised over the cells; the
    per-cell branch and alpha come from linear_alpha, the values follow :129-139 and Linear :52-58, :84 operation by operation
    (test_merge_ref.py checks the vectorised form against linear_smoothing cell by cell)."""
    if tw <= 0:
        raise ValueError("invalid parameter values for linear smoothing")  # Linear :93-94
    I = np.asarray(inner, np.float32)
    O = np.asarray(outer_on_inner, np.float32)
    assert I.shape == O.shape and I.ndim >= 2
    ny, nx = I.shape[-2:]
    kind, alpha = _alpha_planes(nx, ny, tw, bw)
    kind = np.broadcast_to(kind, I.shape)
    alpha = np.broadcast_to(alpha, I.shape)
    vi, vo = I.astype(np.float64), O.astype(np.float64)  # getDouble
    with np.errstate(invalid="ignore", over="ignore"):
        diff = vo - vi
        prod = alpha * diff
        blend = vi + prod
        blend = np.where(diff == 0, vo, blend)
        smoothed = np.where(kind == 0, vo, np.where(kind == 1, vi, blend))
        merged = np.where(np.isnan(vi), vo if use_outer else np.float64(np.nan), np.where(np.isnan(vo), vi, smoothed))
        out = merged.astype(np.float32)
    # the undefined value the reference writes is MIFI_UNDEFINED_D, the quiet NaN; an outer NaN taken over keeps its payload
    if not use_outer:
        out[np.isnan(vi)] = np.float32(np.nan)
    return out


def overlay(top, base):
    """:82-86: top where it is defined, else base"""
    t, b = np.asarray(top, np.float32), np.asarray(base, np.float32)
    assert t.shape == b.shape
    return np.where(np.isnan(t), b, t)


def _equal(a, b):
    """src/CDMMergeUtils.h:35-38"""
    return math.fabs(a - b) < 1e-6


def extend_inner_axis(valuesI, valuesO):
    """extendInnerAxis on the two axes' values (doubles, in one unit): the inner axis continued with its own step as far as the
    outer axis reaches"""
    vI, vO = [float(v) for v in valuesI], [float(v) for v in valuesO]
    if len(vI) < 2 or len(vO) < 2:
        raise ValueError("no data for axis")  # :245-248
    stepI, stepO = vI[1] - vI[0], vO[1] - vO[0]  # :251
    for i in range(2, len(vI)):
        if not _equal(vI[i] - vI[i - 1], stepI):
            raise ValueError("inner axis does not have constant step size, cannot merge")
    for i in range(2, len(vO)):
        if not _equal(vO[i] - vO[i - 1], stepO):
            raise ValueError("outer axis does not have constant step size, cannot merge")
    minI = vI[0] if stepI > 0 else vI[-1]  # :262-263
    minO = vO[0] if stepO > 0 else vO[-1]
    maxI = vI[0] if stepI < 0 else vI[-1]
    maxO = vO[0] if stepO < 0 else vO[-1]
    if minI < minO or maxI > maxO:
        raise ValueError("top not inside  bottom")
    reverse = []
    nO = vI[0] - stepI  # :268
    while minO <= nO <= maxO:
        reverse.append(nO)
        nO -= stepI
    extended = reverse[::-1] + vI
    nO = vI[-1] + stepI  # :272
    while minO <= nO <= maxO:
        extended.append(nO)
        nO += stepI
    return np.array(extended, np.float64)


class Grid:
    """a projection string, its two axes (degrees for a geographic projection) and whether they are degrees"""

    def __init__(self, proj, x, y, degree):
        self.proj, self.degree = proj, bool(degree)
        self.x, self.y = np.asarray(x, np.float64), np.asarray(y, np.float64)

    @property
    def shape(self):
        return self.y.size, self.x.size

    def axes(self):
        """what CDMInterpolator hands to the projection code: radians for degrees (src/CDMInterpolator.cc:1443-1451)"""
        return (np.radians(self.x), np.radians(self.y)) if self.degree else (self.x, self.y)


def positions(src, dst, project_axes=po.project_axes, points2position=oracle.points2position, types=(oracle.PROJ_AXIS, oracle.LONGITUDE, oracle.LATITUDE)):
    """Fractional positions of every cell of dst on the axes of src, as CDMInterpolator::changeProjection derives them:
    mifi_project_axes of the target mesh into the source projection, then mifi_points2position on the source axes."""
    dx, dy = dst.axes()
    sx, sy = src.axes()
    qx, qy = project_axes(dst.proj, src.proj, dx, dy)
    tx, ty = (types[1], types[2]) if src.degree else (types[0], types[0])
    px = points2position(np.array(qx, np.float64).ravel(), sx, tx)
    py = points2position(np.array(qy, np.float64).ravel(), sy, ty)
    return np.asarray(px, np.float64), np.asarray(py, np.float64)


def merge_positions(inner, outer, target, **kw):
    """the three position pairs of a merge: outer on the inner grid, inner on the target, outer on the target"""
    return positions(outer, inner, **kw), positions(inner, target, **kw), positions(outer, target, **kw)


def merge(I, O, pos, shapes, method=oracle.BILINEAR, smooth_method=oracle.BILINEAR, tw=5, bw=2, use_outer=True, outer_method=None):
    """CDMMerger::getDataSlice on float fields I [nz][iy][ix] and O [nz][oy][ox].  pos: merge_positions' three pairs; shapes:
    ((iy, ix), (oy, ox), (ty, tx)); outer_method: the method of the outer -> target regrid where it is not `method` (the reference
    gives both one, the library's merge plan takes any two backward plans).  -> (out [nz][ty][tx], the smoothed inner field S)"""
    (iy, ix), (oy, ox), (ty, tx) = shapes
    (oi_x, oi_y), (it_x, it_y), (ot_x, ot_y) = pos
    I = np.asarray(I, np.float32).reshape(-1, iy, ix)
    O = np.asarray(O, np.float32).reshape(-1, oy, ox)
    OI = oracle.interpolate_values(smooth_method, oi_x, oi_y, O, ox, oy, ix, iy)  # step 1 (CDMBorderSmoothing's interpolator)
    S = border_smooth(I, OI, tw, bw, use_outer)                                   # step 2
    ST = oracle.interpolate_values(method, it_x, it_y, S, ix, iy, tx, ty)         # step 3
    OT = oracle.interpolate_values(method if outer_method is None else outer_method, ot_x, ot_y, O, ox, oy, tx, ty)
    return overlay(ST, OT), S                                                     # step 4


# ---- the reference's own cases (test/testMerger.cc)
def _read(golden_dir, name):
    from scipy.io import netcdf_file
    return netcdf_file(os.path.join(golden_dir, name), "r", mmap=False)


def _field(f, var):
    """a variable as the interpolator's float array: the fill value becomes NaN (data2InterpolationArray)"""
    v = f.variables[var]
    a = np.array(v.data, np.float64)
    fill = getattr(v, "_FillValue", None)
    out = a.astype(np.float32)
    if fill is not None:
        out[a == np.float64(fill)] = np.nan
    return out.reshape((-1,) + out.shape[-2:])


# name -> (target shape (ny, nx), [(ix, iy, expected)], bound): test/testMerger.cc:54-60, :88-94
KNOWN = {
    "test_merger": ((113, 61), [(28, 56, 288.104), (24, 56, 288.467), (8, 56, 289.937)], 0.001),
    "test_merge_target": ((101, 101), [(19, 65, 275.62), (22, 21, 276.30)], 0.01),
}


def load_case(golden_dir, name):
    """-> dict(I, O, inner, outer, target): the two fields and the three grids of one of the reference's cases"""
    if name == "test_merger":  # :41-51: setTargetGridFromInner
        fi, fo = _read(golden_dir, "test_merge_inner.nc"), _read(golden_dir, "test_merge_outer.nc")
        proj = fi.variables["projection_regular_ll"].proj4.decode()
        inner = Grid(proj, fi.variables["longitude"].data, fi.variables["latitude"].data, True)
        outer = Grid(fo.variables["projection_regular_ll"].proj4.decode(), fo.variables["longitude"].data, fo.variables["latitude"].data, True)
        target = Grid(proj, extend_inner_axis(inner.x, outer.x), extend_inner_axis(inner.y, outer.y), True)
        return dict(I=_field(fi, "ga_2t_1"), O=_field(fo, "ga_2t_1"), inner=inner, outer=outer, target=target)
    if name == "test_merge_target":  # :74-85: CDMMerger(base, top), the base file is the inner
        fi, fo = _read(golden_dir, "merge_target_base.nc"), _read(golden_dir, "merge_target_top.nc")
        inner = Grid(fi.variables["projection_regular_ll"].proj4.decode(), fi.variables["longitude"].data, fi.variables["latitude"].data, True)
        outer = Grid(fo.variables["projection_6"].proj4.decode(), fo.variables["x"].data, fo.variables["y"].data, False)
        target = Grid("+proj=stere +lat_0=90 +lon_0=70 +lat_ts=60 +units=m +a=6.371e+06 +e=0 +no_defs",
                      -1192800. + 800. * np.arange(101), -1304000. + 800. * np.arange(101), False)
        return dict(I=_field(fi, "air_temperature_2m"), O=_field(fo, "air_temperature_2m"), inner=inner, outer=outer, target=target)
    raise KeyError(name)


def case_shapes(c):
    return c["inner"].shape, c["outer"].shape, c["target"].shape
