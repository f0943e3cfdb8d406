"""CPU restatement of the reference's time-axis interpolation and quality masking, the yardstick of tests/test_gpu_time_quality.py
(include/fimex_amd.h, 8f n10).  Not a test.

  time_mapping      the loop of CDMTimeInterpolator::changeTimeAxis, src/CDMTimeInterpolator.cc:161-188, on doubles
  blend_factor      f of mifi_get_values_linear_conf_extrapol_f, src/interpolation.c:1087, and the branch it selects, :1088-1102
  blend             mifi_get_values_linear_weak_extrapol_f, src/interpolation.c:1085-1109, on two float32 fields
  time_interpolate  CDMTimeInterpolator::getDataSlice, src/CDMTimeInterpolator.cc:109-125, for every position of the new axis:
                    Data::asFloat() of the two slices (include/fimex/Utils.h:94-116, a cast), then blend
  cast_fill         data_caster<C, double>, include/fimex/Utils.h:85-115, as DataImpl<C>::setValue uses it, src/DataImpl.h:140
  quality_mask      CDMQualityExtractor::getDataSlice, src/CDMQualityExtractor.cc:281-385; HIGHEST and LOWEST as
                    include/fimex/CDMQualityExtractor.h documents them, not as findDefinedExtreme (:219-237) behaves (divergence D8)
tests/test_time_quality_ref.py pins blend to the reference's object code (oracle/_ref/libmifi_ref.so) and everything to
tests/golden/time_quality_answers.npz.  The mapping and the mask are C++ behind boost and have no object code to be pinned to.
"""
import bisect
import ctypes
import os

import numpy as np

f32, f64 = np.float32, np.float64

FIXTURE = "time_quality_answers.npz"
UNDEFINED_F_BITS = 0x7FC00000  # MIFI_UNDEFINED_F as the library writes it

CDM_CHAR, CDM_SHORT, CDM_INT, CDM_FLOAT, CDM_DOUBLE, CDM_UCHAR, CDM_USHORT, CDM_UINT, CDM_INT64, CDM_UINT64 = 1, 2, 3, 4, 5, 7, 8, 9, 10, 11
DTYPES = {CDM_CHAR: np.int8, CDM_SHORT: np.int16, CDM_INT: np.int32, CDM_FLOAT: np.float32, CDM_DOUBLE: np.float64,
          CDM_UCHAR: np.uint8, CDM_USHORT: np.uint16, CDM_UINT: np.uint32, CDM_INT64: np.int64, CDM_UINT64: np.uint64}
TYPES = tuple(DTYPES)

COPY_A, COPY_B, BLEND, UNDEFINED = 0, 1, 2, 3
VALUES, ALL, MAX, MIN, HIGHEST, LOWEST = 0, 1, 2, 3, 4, 5
MODES = (VALUES, ALL, MAX, MIN, HIGHEST, LOWEST)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


# ------------------------------------------------------------------ time axis
def time_mapping(oldTimes, newTimes):
    """(t1, t2) per new time; raises ValueError where the library returns -1."""
    old = [float(v) for v in np.asarray(oldTimes, f64).reshape(-1)]
    if not old or any(not (a < b) for a, b in zip(old, old[1:])) or old[0] != old[0]:
        raise ValueError("the old times must be strictly ascending and not empty")
    t1, t2 = [], []
    lastPos = 0
    for x in np.asarray(newTimes, f64).reshape(-1):
        pos = bisect.bisect_left(old, float(x), lastPos)  # lower_bound(oldTimes.begin() + lastPos, ...), :167
        if pos == len(old):
            pos -= 1                                      # :170-173
        b = pos                                           # :174
        if pos != 0:
            a = pos - 1                                   # :176
        else:
            a = pos                                       # :178
            if pos + 1 != len(old):
                b = pos + 1                               # :180
        lastPos = pos                                     # :185
        t1.append(a)
        t2.append(b)
    return np.array(t1, np.uintp), np.array(t2, np.uintp)


def blend_factor(a, b, x):
    """(f, branch): f a float32, the double quotient rounded once."""
    with np.errstate(all="ignore"):
        f = f32(0) if a == b else f32((f64(x) - f64(a)) / (f64(b) - f64(a)))  # :1087
    if f == 0:
        return f, COPY_A
    if f == 1:
        return f, COPY_B
    if f >= f32(-1.0) and f <= f32(2.0):  # :1094, the limits of :1108
        return f, BLEND
    return f, UNDEFINED


def blend(A, B, a, b, x):
    """mifi_get_values_linear_weak_extrapol_f on float32 arrays."""
    A, B = np.asarray(A, f32), np.asarray(B, f32)
    f, branch = blend_factor(a, b, x)
    if branch == COPY_A:
        return A.copy()
    if branch == COPY_B:
        return B.copy()
    if branch == BLEND:
        with np.errstate(all="ignore"):
            return (A + (f * (B - A)).astype(f32)).astype(f32)  # :1045, every operation in float
    return np.full(A.shape, UNDEFINED_F_BITS, np.uint32).view(f32)


def time_interpolate(data, oldTimes, newTimes):
    """data[nOld, ...] of a stored type -> float32 [nNew, ...]."""
    x = np.asarray(data)
    old, new = np.asarray(oldTimes, f64).reshape(-1), np.asarray(newTimes, f64).reshape(-1)
    t1, t2 = time_mapping(old, new)
    if x.shape[0] != old.size:
        raise ValueError("one slice per old time")
    out = np.empty((new.size,) + x.shape[1:], f32)
    for i in range(new.size):
        a, b = int(t1[i]), int(t2[i])
        with np.errstate(all="ignore"):
            out[i] = blend(x[a].astype(f32), x[b].astype(f32), old[a], old[b], new[i])  # :112-124
    return out


def undefined_positions(oldTimes, newTimes):
    """bool per new time: the whole output slice is MIFI_UNDEFINED_F."""
    old, new = np.asarray(oldTimes, f64).reshape(-1), np.asarray(newTimes, f64).reshape(-1)
    t1, t2 = time_mapping(old, new)
    return np.array([blend_factor(old[int(a)], old[int(b)], x)[1] == UNDEFINED for a, b, x in zip(t1, t2, new)], bool)


# ------------------------------------------------------------------ quality mask
def _round_half_away(v):
    t = float(np.trunc(v))
    return t + (float(np.copysign(1.0, v)) if abs(v - t) >= 0.5 else 0.0)


def cast_fill(fillValue, dtype):
    """data_caster<C, double>(fillValue); raises ValueError for a fill the type cannot hold: one that the route through int does not
    give back as rounded, or one beyond the range of float."""
    dtype = np.dtype(dtype)
    v = float(fillValue)
    if dtype == np.float64:
        return f64(v)
    if dtype == np.float32:
        if np.isfinite(v) and abs(v) > float(np.finfo(f32).max):
            raise ValueError("fill beyond the range of float")
        return f32(v)
    if v != v or not abs(v) < 2.0 ** 63:
        raise ValueError("no integer fill")
    r = int(_round_half_away(v))                 # lround, Utils.h:72-75
    as_int = (r + 2 ** 31) % 2 ** 32 - 2 ** 31   # long -> int
    info = np.iinfo(dtype)
    c = as_int % 2 ** info.bits                  # int -> C, modulo 2^bits
    if info.min < 0 and c >= 2 ** (info.bits - 1):
        c -= 2 ** info.bits
    if c != r:
        raise ValueError("the type cannot hold the fill")
    return dtype.type(c)


def masked_status(status, mode, values=(), limit=np.nan, validMin=np.nan, validMax=np.nan, statusFill=np.nan):
    """bool per status cell: the cells of the data at this position get the fill value."""
    with np.errstate(all="ignore"):
        sd = np.asarray(status).reshape(-1).astype(f64)  # asDouble(), :283
    if mode == VALUES:
        use = sorted(float(v) for v in np.asarray(values, f64).reshape(-1))  # :286-287
        if not use or any(v != v for v in use):
            raise ValueError("an empty list or a NaN in it")
        return np.isnan(sd) | ~np.isin(sd, use)  # :370 (binary_search reports NaN as found), :380
    if mode not in MODES:
        raise ValueError("unknown mode")
    with np.errstate(invalid="ignore"):
        if validMin == validMin:
            sd[sd < validMin] = np.nan      # :304-312
        if validMax == validMax:
            sd[sd > validMax] = np.nan      # :313-321
        if statusFill == statusFill:
            sd[sd == statusFill] = np.nan   # :322-330
        if mode == MAX:
            sd[sd > limit] = np.nan         # :339
        elif mode == MIN:
            sd[sd < limit] = np.nan         # :349
        elif mode in (HIGHEST, LOWEST):     # CDMQualityExtractor.h: only the highest / lowest defined status is kept
            defined = sd[~np.isnan(sd)]
            if defined.size:
                sd[sd != (defined.max() if mode == HIGHEST else defined.min())] = np.nan
    return np.isnan(sd)                     # :380


def quality_mask(data, status, mode, fillValue, values=(), limit=np.nan, validMin=np.nan, validMax=np.nan, statusFill=np.nan):
    """A masked copy of data; status=None: the data is its own status.  Raises ValueError where the library returns -1."""
    out = np.array(data, copy=True)
    s = out if status is None else np.asarray(status)
    m = masked_status(s, mode, values, limit, validMin, validMax, statusFill)
    fill = cast_fill(fillValue, out.dtype)
    if out.size == 0:
        return out
    if s.size == 0 or out.size % s.size:
        raise ValueError("incompatible sizes")
    flat = out.reshape(out.size // s.size, s.size)  # :377-385
    flat[:, m] = fill
    return out


# ------------------------------------------------------------------ the reference's object code
class ReferenceLib:
    """mifi_get_values_linear_weak_extrapol_f of oracle/_ref/libmifi_ref.so."""

    def __init__(self, path):
        self.fn = ctypes.CDLL(path).mifi_get_values_linear_weak_extrapol_f
        fp = ctypes.POINTER(ctypes.c_float)
        self.fn.argtypes = [fp, fp, fp, ctypes.c_size_t, ctypes.c_double, ctypes.c_double, ctypes.c_double]
        self.fn.restype = ctypes.c_int

    def blend(self, A, B, a, b, x):
        A, B = np.ascontiguousarray(A, f32), np.ascontiguousarray(B, f32)
        out = np.empty(A.shape, f32)
        fp = ctypes.POINTER(ctypes.c_float)
        rc = self.fn(A.ctypes.data_as(fp), B.ctypes.data_as(fp), out.ctypes.data_as(fp), A.size, a, b, x)
        assert rc == 1  # MIFI_OK
        return out


def reference_lib():
    """The ReferenceLib of oracle/_ref/libmifi_ref.so, or None where build() found no reference tree to compile it from."""
    import oracle
    return ReferenceLib(oracle.ref().path) if oracle.ref() is not None else None


# ------------------------------------------------------------------ cases
OLD_TIMES = np.array([0.0, 6.0, 12.0, 18.0])
AXES = {
    "fine": (OLD_TIMES, np.arange(29) * 1.5 - 9.0),                              # -9, -7.5, ..., 33: every branch, both extrapolations
    "coarse": (np.arange(7) * 3.0, np.array([0.0, 1.0, 10.0, 10.5, 18.0, 30.0])),  # a pair's t1 is not the previous t2
    "backwards": (OLD_TIMES, np.array([13.0, 2.0, 7.0, 18.0, 3.0, 12.0, 6.0])),   # lower_bound starts at the previous position
    "single": (np.array([5.0]), np.array([4.0, 5.0, 6.0])),                       # one old time: (0, 0), f = 0
}


def series(seed, dtype, nOld, n):
    """[nOld][n] of a stored type; the floating ones carry NaN, both infinities and values past the range of float."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dtype.kind == "f":
        x = rng.uniform(-50.0, 50.0, (nOld, n)).astype(dtype)
        x[rng.uniform(size=x.shape) < 0.08] = np.nan
        x.reshape(-1)[::17] = np.inf
        if dtype == np.float64:
            x.reshape(-1)[5::19] = 1e300
    else:
        info = np.iinfo(dtype)
        x = rng.integers(info.min, info.max, (nOld, n), dtype=dtype, endpoint=True)
        small = rng.uniform(size=x.shape) < 0.5
        x[small] = rng.integers(max(info.min, -300), min(info.max, 300), np.count_nonzero(small), endpoint=True).astype(dtype)
    return x


def status_values(seed, dtype, n, nan_share=0.1):
    """n status values 0 .. 9 of a stored type; the floating ones carry NaN."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 10, n).astype(dtype)
    if dtype.kind == "f":
        s[rng.uniform(size=n) < nan_share] = np.nan
    return s


def mode_arguments(mode):
    """Keyword arguments of quality_mask for one mode on status_values: every rule takes some cells and leaves some."""
    if mode == VALUES:
        return {"values": (7.0, 2.0, 3.0)}
    kw = {"validMin": 1.0, "validMax": 8.0, "statusFill": 5.0}
    if mode in (MAX, MIN):
        kw["limit"] = 6.0 if mode == MAX else 3.0
    return kw


def data_values(seed, dtype, shape):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dtype.kind == "f":
        return rng.uniform(-50.0, 50.0, shape).astype(dtype)
    return rng.integers(1, 100, shape).astype(dtype)


RECORDED_BLEND_N = 64
RECORDED_MASK_DATA = (CDM_SHORT, CDM_FLOAT, CDM_UINT64)
RECORDED_MASK_STATUS = (CDM_UCHAR, CDM_DOUBLE)


def recorded_blend_fields():
    """(A, B): float32 with NaN on either side, infinities, zeros of both signs and large values."""
    rng = np.random.default_rng(800)
    A = rng.uniform(-300.0, 300.0, RECORDED_BLEND_N).astype(f32)
    B = rng.uniform(-300.0, 300.0, RECORDED_BLEND_N).astype(f32)
    A[[1, 9]], B[[2, 9]] = np.nan, np.nan
    A[3], B[4], A[5], B[5] = np.inf, -np.inf, np.inf, np.inf
    A[6], B[6], A[7], B[7] = 0.0, -0.0, -0.0, 0.0
    A[8], B[8] = 3e38, -3e38
    return A, B


def load_fixture(golden_dir):
    with np.load(os.path.join(golden_dir, FIXTURE)) as z:
        return {k: z[k] for k in z.files}
