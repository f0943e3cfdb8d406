"""CPU restatement of the reference's vertical interpolation, the yardstick of tests/test_gpu_vertical.py.  Not a test.

Per column and output level (src/CDMVerticalInterpolator.cc:441-504): the target level x, the validity range, the search for the
bracketing input levels (include/fimex/Utils.h:204-290), the blend of the two data values (src/interpolation.c:1030-1156 through
the oracle's orc_get_values_1d_f with one-element arrays, so that the log kinds use the C library's log) and the output clamp.
The two searches are plain sequential Python over one column; `search_pairs` is the same walk vectorised over columns with numpy
(one step per input level, in index order) and `interpolate` uses it, with a vectorised blend for nearest and the linear family.
tests/test_vertical_ref.py checks the vectorised forms against the per-cell ones.
"""
import numpy as np

import oracle

# mifi_vertical_interpol_method, include/fimex/mifi_constants.h:202-231
LIN, LOG, LOGLOG, NN, LIN_WEAK_EXTRA, LIN_NO_EXTRA, LIN_CONST_EXTRA = range(7)
METHODS = (LIN, LOG, LOGLOG, NN, LIN_WEAK_EXTRA, LIN_NO_EXTRA, LIN_CONST_EXTRA)
LINEAR_FAMILY = (LIN, NN, LIN_WEAK_EXTRA, LIN_NO_EXTRA, LIN_CONST_EXTRA)
# intFunc of src/CDMVerticalInterpolator.cc:333-341 as the oracle's blend kind
BLEND_OF = {LIN: oracle.BLEND_LINEAR, LOG: oracle.BLEND_LOG, LOGLOG: oracle.BLEND_LOG_LOG, NN: oracle.BLEND_NEAREST,
            LIN_WEAK_EXTRA: oracle.BLEND_LINEAR_WEAK_EXTRAPOL, LIN_NO_EXTRA: oracle.BLEND_LINEAR_NO_EXTRAPOL,
            LIN_CONST_EXTRA: oracle.BLEND_LINEAR_CONST_EXTRAPOL}

FIELD, AXIS, SIGMA, HYBRID_SIGMA, HYBRID_SIGMA_AP = range(5)
KINDS = (FIELD, AXIS, SIGMA, HYBRID_SIGMA, HYBRID_SIGMA_AP)

DBL_MAX = np.finfo(np.float64).max


# ------------------------------------------------------------------ the two searches, one column
def find_closest_distinct_elements(levels, x):
    """include/fimex/Utils.h:204-236."""
    n = len(levels)
    r1 = r2 = 0
    if n == 0:
        return 0, 0
    x = float(x)
    v1 = float(levels[0])
    v1Diff = abs(x - v1)
    v2Diff = v1Diff
    for k in range(n):
        cur = float(levels[k])
        vDiff = abs(x - cur)
        if vDiff <= v2Diff:
            if vDiff < v1Diff:
                r2 = r1
                v2Diff = v1Diff
                v1 = cur
                r1 = k
                v1Diff = vDiff
            elif cur != v1:
                r2 = k
                v2Diff = vDiff
    return r1, r2


def find_closest_neighbor_distinct_elements(levels, x):
    """include/fimex/Utils.h:251-290."""
    n = len(levels)
    if n == 0:
        return 0, 0
    x = float(x)
    lowest = highest = 0
    cur = float(levels[0])
    lowDiff = x - cur
    highDiff = cur - x
    if lowDiff < 0:
        lowDiff = DBL_MAX
    if highDiff < 0:
        highDiff = DBL_MAX
    for k in range(1, n):
        cur = float(levels[k])
        if cur <= x:
            diff = x - cur
            if diff < lowDiff:
                lowDiff = diff
                lowest = k
        else:
            diff = cur - x
            if diff < highDiff:
                highDiff = diff
                highest = k
    if lowDiff == DBL_MAX or highDiff == DBL_MAX:
        return find_closest_distinct_elements(levels, x)
    return lowest, highest


# ------------------------------------------------------------------ level descriptions
class Levels:
    """The levels of every column of a [nt][nz][ny][nx] variable (fimex_amd_vertical_levels)."""

    def __init__(self, kind, nz, axis=None, sigma=None, a=None, ap=None, b=None, p0=0.0, ptop=0.0, ps=None, field=None):
        f64 = lambda v: None if v is None else np.ascontiguousarray(v, np.float64)
        f32 = lambda v: None if v is None else np.ascontiguousarray(v, np.float32)
        self.kind, self.nz = kind, nz
        self.axis, self.sigma, self.a, self.ap, self.b = f64(axis), f64(sigma), f64(a), f64(ap), f64(b)
        self.p0, self.ptop = float(p0), float(ptop)
        self.ps, self.field = f32(ps), f32(field)


def level_field(lv, nt, ny, nx):
    """verticalData4D(...)->asFloat(): float32 [nt][nz][ny][nx]; the formulas in float64 in the order of
    src/vertical_coordinate_transformations.c:37-71, then rounded to float32."""
    if lv.kind == FIELD:
        return lv.field.reshape(nt, lv.nz, ny, nx).copy()
    if lv.kind == AXIS:
        return np.broadcast_to(lv.axis.astype(np.float32)[None, :, None, None], (nt, lv.nz, ny, nx)).copy()
    ps = lv.ps.reshape(nt, 1, ny, nx).astype(np.float64)
    col = lambda c: c[None, :, None, None]
    with np.errstate(all="ignore"):
        if lv.kind == SIGMA:
            pDiff = ps - lv.ptop
            p = lv.ptop + col(lv.sigma) * pDiff
        elif lv.kind == HYBRID_SIGMA:
            p = (col(lv.a) * lv.p0) + (col(lv.b) * ps)
        elif lv.kind == HYBRID_SIGMA_AP:
            p = col(lv.ap) + (col(lv.b) * ps)
        else:
            raise ValueError("unknown level kind %r" % (lv.kind,))
        return p.astype(np.float32)


# ------------------------------------------------------------------ one cell
def blend_cell(method, v0, v1, lev0, lev1, x):
    """intFunc(&v0, &v1, out, 1, (double)lev0, (double)lev1, x), src/CDMVerticalInterpolator.cc:482.  Where the blend returns
    MIFI_ERROR the reference leaves the element unset; NaN here (the documented divergence)."""
    out, rc = oracle.get_values_1d(BLEND_OF[method], np.array([v0], np.float32), np.array([v1], np.float32),
                                   float(np.float32(lev0)), float(np.float32(lev1)), float(x))
    return out[0] if rc == oracle.OK else np.float32(np.nan)


def in_range(x, vmin, vmax):
    """src/CDMVerticalInterpolator.cc:454-471 (vmin / vmax: None when the array is absent)."""
    if vmin is not None and vmax is not None:
        return (x >= vmin) and (x <= vmax)
    if vmin is not None:
        return x >= vmin
    if vmax is not None:
        return x <= vmax
    return True


def clamp(v, clampMin, clampMax):
    """:494-504 on float32 arrays."""
    v = np.array(v, np.float32)
    with np.errstate(invalid="ignore"):
        if not np.isnan(clampMin):
            v = np.where(v < np.float32(clampMin), np.float32(clampMin), v)
        if not np.isnan(clampMax):
            v = np.where(v > np.float32(clampMax), np.float32(clampMax), v)
    return v.astype(np.float32)


def interpolate_cell(method, levels, data, x, vmin=None, vmax=None):
    """One output element before the clamp: levels / data are the column's nzi input levels (float32) and values."""
    if not in_range(x, vmin, vmax):
        return np.float32(np.nan)
    first, second = find_closest_neighbor_distinct_elements(levels, x)
    if first == second:
        return np.float32(np.nan)
    return blend_cell(method, data[first], data[second], levels[first], levels[second], x)


# ------------------------------------------------------------------ all columns at once
def search_pairs(ilev, x):
    """find_closest_neighbor_distinct_elements for every column and output level: ilev float32 [nt][nzi][ny][nx],
    x float64 [nt][nzo][ny][nx] -> (first, second) int arrays of x's shape.  One numpy step per input level, in index order."""
    nzi = ilev.shape[1]
    lev = lambda k: ilev[:, k][:, None].astype(np.float64)
    with np.errstate(all="ignore"):
        c0 = lev(0)
        lowDiff, highDiff = x - c0, c0 - x
        lowDiff = np.where(lowDiff < 0, DBL_MAX, lowDiff)
        highDiff = np.where(highDiff < 0, DBL_MAX, highDiff)
        lowest = np.zeros(x.shape, np.int64)
        highest = np.zeros(x.shape, np.int64)
        for k in range(1, nzi):
            c = lev(k)
            le = c <= x
            d = x - c
            upd = le & (d < lowDiff)
            lowDiff = np.where(upd, d, lowDiff)
            lowest = np.where(upd, k, lowest)
            d = c - x
            upd = ~le & (d < highDiff)
            highDiff = np.where(upd, d, highDiff)
            highest = np.where(upd, k, highest)
        need = (lowDiff == DBL_MAX) | (highDiff == DBL_MAX)
        # find_closest_distinct_elements
        v1 = np.broadcast_to(c0, x.shape).copy()
        v1Diff = np.abs(x - c0)
        v2Diff = v1Diff.copy()
        r1 = np.zeros(x.shape, np.int64)
        r2 = np.zeros(x.shape, np.int64)
        for k in range(nzi):
            c = np.broadcast_to(lev(k), x.shape)
            vDiff = np.abs(x - c)
            c1 = vDiff <= v2Diff
            c2 = c1 & (vDiff < v1Diff)
            c3 = c1 & ~c2 & (c != v1)
            r2 = np.where(c2, r1, np.where(c3, k, r2))
            v2Diff = np.where(c2, v1Diff, np.where(c3, vDiff, v2Diff))
            v1 = np.where(c2, c, v1)
            r1 = np.where(c2, k, r1)
            v1Diff = np.where(c2, vDiff, v1Diff)
    return np.where(need, r1, lowest), np.where(need, r2, highest)


def _linear_family(method, A, B, a, b, x):
    """src/interpolation.c:1030-1126 with n = 1, vectorised: f in float64 rounded to float32, the blend in float32."""
    if method == NN:
        return A.copy()
    with np.errstate(all="ignore"):
        f = np.where(a == b, 0.0, (x - a) / (b - a)).astype(np.float32)
        lin = (A + f * (B - A)).astype(np.float32)
        nan = np.float32(np.nan)
        if method == LIN:
            return np.where(f == 0, A, np.where(f == 1, B, lin))
        if method == LIN_CONST_EXTRA:
            return np.where(f >= 1, B, np.where(f <= 0, A, lin))
        left, right = (-1.0, 2.0) if method == LIN_WEAK_EXTRA else (0.0, 1.0)
        return np.where(f == 0, A, np.where(f == 1, B, np.where((f >= np.float32(left)) & (f <= np.float32(right)), lin, nan)))


def log_factor(method, a, b, x):
    """The f of the log blends in float64 (numpy's log): for the tolerance of the GPU comparison only, never for a result."""
    with np.errstate(all="ignore"):
        if method == LOGLOG:
            a, b, x = np.log(a + np.e), np.log(b + np.e), np.log(x + np.e)
        la, lb, lx = np.log(a), np.log(b), np.log(x)
        return np.where(la == lb, 0.0, (lx - la) / (lb - la))


def interpolate(method, data, ilev, x, validMin=None, validMax=None, clampMin=np.nan, clampMax=np.nan, columns=None, details=False):
    """getLevelDataSlice for a batch: data, ilev float32 [nt][nzi][ny][nx]; x float64 [nt][nzo][ny][nx] (fixed levels: broadcast
    level1 first); validMin / validMax float64 [ny][nx] or None -> float32 [nt][nzo][ny][nx].
    columns: boolean [ny][nx]; only those columns are computed (the others come back as NaN) -- the log kinds go cell by cell.
    details: also return (A, B, f) of the blend per cell (f in float64), for tolerances."""
    data = np.ascontiguousarray(data, np.float32)
    ilev = np.ascontiguousarray(ilev, np.float32)
    x = np.ascontiguousarray(np.broadcast_to(x, (data.shape[0], x.shape[1]) + data.shape[2:]), np.float64)
    first, second = search_pairs(ilev, x)
    take = lambda arr, idx: np.take_along_axis(arr, idx, axis=1)
    A, B = take(data, first), take(data, second)
    a, b = take(ilev, first).astype(np.float64), take(ilev, second).astype(np.float64)
    ok = first != second
    with np.errstate(invalid="ignore"):
        if validMin is not None:
            ok &= x >= np.asarray(validMin, np.float64)[None, None]
        if validMax is not None:
            ok &= x <= np.asarray(validMax, np.float64)[None, None]
    if columns is not None:
        ok &= np.asarray(columns, bool)[None, None]
    if method in LINEAR_FAMILY:
        out = _linear_family(method, A, B, a, b, x).astype(np.float32)
    else:
        out = np.full(x.shape, np.nan, np.float32)
        kind = BLEND_OF[method]
        for idx in zip(*np.nonzero(ok)):
            r, rc = oracle.get_values_1d(kind, A[idx].reshape(1), B[idx].reshape(1), float(a[idx]), float(b[idx]), float(x[idx]))
            if rc == oracle.OK:
                out[idx] = r[0]
    out = clamp(np.where(ok, out, np.float32(np.nan)), clampMin, clampMax)
    if details:
        f = log_factor(method, a, b, x) if method in (LOG, LOGLOG) else None
        return out, A, B, f
    return out
