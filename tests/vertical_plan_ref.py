"""CPU restatement of the vertical interpolation plan (include/fimex_amd.h, 8f n5b), the yardstick of tests/test_gpu_vertical_plan.py.
Not a test.

build() is the search of tests/vertical_ref.py (search_pairs) with the blend of src/interpolation.c:1030-1156 (n = 1) folded into
one factor per output cell; apply() is the one rule that then serves all seven methods, between numpy restatements of
data2InterpolationArray and interpolationArray2Data (src/CDMInterpolator.cc:115-124).  tests/test_vertical_plan_ref.py checks
apply(build()) against vertical_ref.interpolate.
"""
import math

import numpy as np

import vertical_ref as vr


def _logs(v):
    return np.array([math.log(t) for t in v], np.float64)


def build(method, ilev, x, validMin=None, validMax=None):
    """ilev float32 [nt][nzi][ny][nx], x float64 broadcastable to [nt][nzo][ny][nx], validMin / validMax float64 [ny][nx] or None
    -> (first, second, f, undefined), each [nt][nzo][ny][nx]; f float32."""
    ilev = np.ascontiguousarray(ilev, np.float32)
    nt, nzi, ny, nx = ilev.shape
    x = np.ascontiguousarray(np.broadcast_to(x, (nt, np.shape(x)[1], ny, nx)), np.float64)
    first, second = vr.search_pairs(ilev, x)
    undefined = first == second
    with np.errstate(invalid="ignore"):
        if validMin is not None:
            undefined |= ~(x >= np.asarray(validMin, np.float64)[None, None])
        if validMax is not None:
            undefined |= ~(x <= np.asarray(validMax, np.float64)[None, None])
    a = np.take_along_axis(ilev, first, axis=1).astype(np.float64)
    b = np.take_along_axis(ilev, second, axis=1).astype(np.float64)
    xx = x.copy()
    if method in (vr.LOG, vr.LOGLOG):
        with np.errstate(invalid="ignore"):
            undefined |= (a <= 0) | (b <= 0) | (x <= 0)  # :1133, :1146
        ok = ~undefined
        la, lb, lx = a[ok], b[ok], x[ok]
        if method == vr.LOGLOG:
            la, lb, lx = _logs(la + math.e), _logs(lb + math.e), _logs(lx + math.e)
            # :1150; unreachable for positive levels, kept as the reference states it
            assert not np.any((la <= 0) | (lb <= 0) | (lx <= 0))
        a, b, xx = a.copy(), b.copy(), xx
        a[ok], b[ok], xx[ok] = _logs(la), _logs(lb), _logs(lx)
    with np.errstate(all="ignore"):
        f0 = np.where(a == b, 0.0, (xx - a) / (b - a)).astype(np.float32)
        f = f0
        if method == vr.NN:
            f = np.zeros_like(f0)
        elif method == vr.LIN_CONST_EXTRA:
            f = np.where(f0 >= 1, np.float32(1), np.where(f0 <= 0, np.float32(0), f0))
        elif method in (vr.LIN_WEAK_EXTRA, vr.LIN_NO_EXTRA):
            left, right = (np.float32(-1), np.float32(2)) if method == vr.LIN_WEAK_EXTRA else (np.float32(0), np.float32(1))
            undefined = undefined | ~((f0 == 0) | (f0 == 1) | ((f0 >= left) & (f0 <= right)))
    return first, second, f.astype(np.float32), undefined


def as_float_nan(data, bad):
    """data2InterpolationArray: static_cast<float> per element, then the fill value, narrowed to float, as NaN."""
    with np.errstate(all="ignore"):
        f = np.asarray(data).astype(np.float32)
        bad32 = np.float32(bad)
    if not np.isnan(bad32):
        f = np.where(f == bad32, np.float32(np.nan), f)
    return f


def from_float_fill(v, dtype, fill):
    """interpolationArray2Data: NaN -> the fill value, integers through MetNoFimex::round (lround, then long -> int), floating
    types through 1.0 * v + 0.0 in double.  For values inside the range of int."""
    dtype = np.dtype(dtype)
    v = np.asarray(v, np.float32)
    nan = np.isnan(v)
    d = 1.0 * np.where(nan, 0.0, v).astype(np.float64) + 0.0
    if dtype.kind in "iu":
        t = np.trunc(d)
        r = t + np.where(np.abs(d - t) >= 0.5, np.copysign(1.0, d), 0.0)
        out = r.astype(np.int64).astype(np.int32).astype(dtype)
        return np.where(nan, np.array(fill, np.float64).astype(dtype), out).astype(dtype)
    out = d.astype(dtype)
    return np.where(nan, np.array(fill, np.float64).astype(dtype), out).astype(dtype)


def apply(entries, data, dtype=np.float32, bad=np.nan, clampMin=np.nan, clampMax=np.nan):
    """The apply rule of include/fimex_amd.h on data [nt][nzi][ny][nx] of dtype -> [nt][nzo][ny][nx] of dtype."""
    first, second, f, undefined = entries
    dtype = np.dtype(dtype)
    data = np.ascontiguousarray(data, dtype)
    A = as_float_nan(np.take_along_axis(data, first, axis=1), bad)
    B = as_float_nan(np.take_along_axis(data, second, axis=1), bad)
    with np.errstate(all="ignore"):
        v = np.where(f == 0, A, np.where(f == 1, B, (A + f * (B - A)).astype(np.float32))).astype(np.float32)
    v = vr.clamp(np.where(undefined, np.float32(np.nan), v), clampMin, clampMax)
    if dtype == np.float32 and np.isnan(bad):
        return v  # an interpolation array: stored as it is
    return from_float_fill(v, dtype, bad)
