"""numpy restatement of CDMExtractor (reference paths relative to its tree): the array a reduction describes, the order in which the
reference's joinSlices emits it, and the index computations of reduceAxes and reduceLatLonBoundingBox.

A reduction is a list of dimensions, fastest first as a CDM shape is: (length, positions, start, size).  positions is None for a
dimension that is not in dimSlices_, otherwise the strictly ascending source positions (src/CDMExtractor.cc:280-306); (start, size)
is the caller's SliceBuilder window in the reduced dimension.  Arrays are numpy arrays, slowest dimension first."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (south, north, west, east) -> x kept, y kept; values taken from the stored fields of coordTest.nc
BOXES = [
    ((29.5, 31.5, -13.5, -11.2), list(range(2, 9)), list(range(2, 8))),
    ((28.0, 33.0, -11.6, -14.2), [0, 1, 6, 7, 8, 9, 10], list(range(11))),  # west > east: only lon > east && lon < west is outside
    ((31.8, 32.2, -13.1, -12.9), [], []),
]


def coordtest():
    from scipy.io import netcdf_file
    with netcdf_file(os.path.join(GOLDEN, "coordTest.nc"), "r", mmap=False) as f:
        v = f.variables
        return {"x": v["x"].data.astype(np.float64), "y": v["y"].data.astype(np.float64),
                "lon": v["longitude"].data.astype(np.float64), "lat": v["latitude"].data.astype(np.float64),
                "sigma": v["sigma"].data.astype(np.float64) * np.float64(v["sigma"].scale_factor),
                "proj": v["projection_1"].proj4.decode(), "air_temperature": v["air_temperature"].data.astype(np.int16),
                "air_temperature_scale": float(v["air_temperature"].scale_factor), "air_temperature_fill": int(v["air_temperature"]._FillValue)}


def random_reduction(rng, nDims=None, maxLength=6, empty=0.03):
    """1-4 dimensions of length 1-6; a dimension now and then (probability `empty`) gets an empty list or a window of size 0."""
    dims = []
    for _ in range(nDims or rng.integers(1, 5)):
        length = int(rng.integers(1, maxLength + 1))
        hollow = rng.random() < empty
        positions = None
        if rng.random() < 0.6:
            positions = np.sort(rng.choice(length, int(rng.integers(0 if hollow else 1, length + 1)), replace=False))
        limit = length if positions is None else len(positions)
        start = int(rng.integers(0, limit + 1)) if hollow else int(rng.integers(0, limit))
        size = int(rng.integers(0 if hollow else 1, limit - start + 1))
        dims.append((length, positions, start, size))
    return dims


def full(dim):
    """(length, positions) stands for the whole reduced dimension: (length, positions, 0, its reduced length)."""
    if len(dim) == 4:
        return tuple(dim)
    return dim[0], dim[1], 0, dim[0] if dim[1] is None else len(dim[1])


def window_positions(dim):
    length, positions, start, size = full(dim)
    p = np.arange(length) if positions is None else np.asarray(positions, dtype=np.int64)
    return p[start:start + size]


def pick(a, dims):
    """The row-major array of the reduced shape: out[i_{n-1}]...[i_0] = in[p_{n-1}(i_{n-1})]...[p_0(i_0)]."""
    a = np.asarray(a).reshape([d[0] for d in dims][::-1])
    idx = [window_positions(d) for d in dims][::-1]
    return a[np.ix_(*idx)]


def _chunks(p):
    """src/CDMExtractor.cc:131-145: (start, size) of the runs of neighbouring positions."""
    out = []
    for v in p:
        if out and out[-1][0] + out[-1][1] == v:
            out[-1][1] += 1
        else:
            out.append([int(v), 1])
    return [tuple(c) for c in out]


def reference_rectangles(dims):
    """The SliceBuilder list of CDMExtractor::getDataSlice_ (src/CDMExtractor.cc:96-175): per rectangle a (start, size) per
    dimension, fastest first, in the order joinSlices concatenates them."""
    dims = [full(d) for d in dims]
    slices = [[(0, d[0]) for d in dims]]  # :102
    for k, (length, positions, start, size) in enumerate(dims):  # :107
        if positions is None:  # :113-118
            for s in slices:
                s[k] = (start, size)
        elif len(positions) == 0:  # :119-123
            for s in slices:
                s[k] = (start, 0)
        elif size == 0:  # the reference asserts positions.size() > sbStart (:127); an empty window gives an empty result
            for s in slices:
                s[k] = (0, 0)
        elif len(slices) <= 1:  # :129-159, chunks as large as possible
            slices = [s[:k] + [c] + s[k + 1:] for c in _chunks(window_positions(dims[k])) for s in slices]
        else:  # :160-172, position by position
            slices = [s[:k] + [(int(p), 1)] + s[k + 1:] for p in window_positions(dims[k]) for s in slices]
    return slices


def reference_join(a, dims):
    """joinSlices (src/CDMExtractor.cc:54-94): every rectangle read row-major, one after the other, as a flat array."""
    a = np.asarray(a).reshape([d[0] for d in dims][::-1])
    parts = [a[tuple(slice(st, st + n) for st, n in rect[::-1])].ravel() for rect in reference_rectangles(dims)]
    return np.concatenate(parts)


def order_differs(dims):
    """Divergence D9: the concatenation of reference_join is not the row-major array of pick.  The output holds an element, a
    reduced dimension's window holds more than one chunk (the fastest such dimension is the one cut into chunks), and a slower
    dimension that is not reduced has a window longer than 1: it stays whole inside each rectangle although it is slower."""
    dims = [full(d) for d in dims]
    if any(d[3] == 0 for d in dims):
        return False
    cut = next((k for k, d in enumerate(dims) if d[1] is not None and len(_chunks(window_positions(d))) > 1), None)
    if cut is None:
        return False
    return any(d[1] is None and d[3] > 1 for d in dims[cut + 1:])


def axis_range(axis, startVal, endVal):
    """src/CDMExtractor.cc:369-406 with the axis already in the unit of the bounds (slope 1, offset 0): (startPos, size)."""
    v = np.asarray(axis, dtype=np.float64).copy()
    n = v.size
    if n == 0:
        return 0, 0
    delta = 1e-5
    if n > 1 and v[0] != v[1]:
        delta = .01 * abs(v[0] - v[1])  # :370-373
    lo, hi = startVal - delta, endVal + delta
    reverse = n > 1 and v[0] > v[1]
    if reverse:
        v = v[::-1]
    startPos = int(np.searchsorted(v, lo, side="left"))  # lower_bound, :387
    endPos = int(np.searchsorted(v, hi, side="right"))   # upper_bound, :388
    size = max(endPos - startPos, 0)
    if reverse:
        startPos = n - size - startPos  # :402
    return startPos, size


def bounding_box(lon, lat, south, north, west, east):
    """src/CDMExtractor.cc:496-511 on degree fields [ny][nx]: the ascending x and y positions with a point inside the box.
    A point that is not finite lies outside (divergence D10; HUGE_VAL in the reference, which falls outside every box too)."""
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    wrap180 = west > east  # :449
    with np.errstate(invalid="ignore"):
        out = (lat < south) | (lat > north)
        out |= ((lon > east) & (lon < west)) if wrap180 else ((lon < west) | (lon > east))
    keep = ~out & np.isfinite(lon) & np.isfinite(lat)
    return np.flatnonzero(keep.any(axis=0)), np.flatnonzero(keep.any(axis=1))


def bound_distance(lon, lat, south, north, west, east):
    """Smallest distance (degrees) of any point to any of the four bounds: how far the box is from a rounding question."""
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    return min(np.abs(lat - south).min(), np.abs(lat - north).min(), np.abs(lon - west).min(), np.abs(lon - east).min())
