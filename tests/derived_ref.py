"""CPU restatement of the reference's scaled conversion, theta2T, specific2relative and accumulate / deaccumulate, the yardstick of
tests/test_gpu_derived.py (include/fimex_amd.h, 8f n9).  Not a test.

  convert_scaled            ScaleValue<IN, OUT>, include/fimex/Utils.h:443-464 (data_caster :85-115, round :72-75), as
                            DataImpl<IN>::convertDataType drives it, src/DataImpl.h:316-349
  theta_to_temperature      ThetaTemperatureConverter::getDataSlice, src/CDMPressureConversions.cc:226-245, float32 throughout, the C
                            library's powf
  specific_to_relative      mifi_specific_to_relative_humidity, src/vertical_coordinate_transformations.c:114-141, the C library's exp
  pack_relative_humidity    the short of CDMPressureConversions.cc:330, with what the reference's x86-64 build yields outside short
  accumulate, deaccumulate  CDMProcessor::getDataSlice, src/CDMProcessor.cc:470-491, :534-578, position after position
tests/test_derived_ref.py pins specific_to_relative to the reference's object code (oracle/_ref/libmifi_ref.so) and all of them to
tests/golden/derived_answers.npz.  The other four are C++ behind boost and have no object code to be pinned to.
"""
import ctypes
import ctypes.util
import os

import numpy as np

f32, f64 = np.float32, np.float64

FIXTURE = "derived_answers.npz"

# fimex_amd_datatype (include/fimex_amd.h) -> numpy; char is signed on the reference's platforms
CDM_CHAR, CDM_SHORT, CDM_INT, CDM_FLOAT, CDM_DOUBLE, CDM_UCHAR, CDM_USHORT, CDM_UINT, CDM_INT64, CDM_UINT64 = 1, 2, 3, 4, 5, 7, 8, 9, 10, 11
CDM_NAT, CDM_STRING = 0, 6
DTYPES = {CDM_CHAR: np.int8, CDM_SHORT: np.int16, CDM_INT: np.int32, CDM_FLOAT: np.float32, CDM_DOUBLE: np.float64,
          CDM_UCHAR: np.uint8, CDM_USHORT: np.uint16, CDM_UINT: np.uint32, CDM_INT64: np.int64, CDM_UINT64: np.uint64}
TYPES = tuple(DTYPES)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.exp.argtypes, _libm.exp.restype = [ctypes.c_double], ctypes.c_double
_libm.powf.argtypes, _libm.powf.restype = [ctypes.c_float, ctypes.c_float], ctypes.c_float
_exp_array = np.frompyfunc(lambda x: _libm.exp(float(x)), 1, 1)
_powf_array = np.frompyfunc(lambda x, y: _libm.powf(float(x), float(y)), 2, 1)


def c_exp(x):
    """exp() of the C library element by element on a float64 array."""
    x = np.asarray(x, f64)
    return np.array(_exp_array(x), dtype=f64).reshape(x.shape)


def c_powf(x, y):
    """powf() of the C library element by element on a float32 array and a float32 exponent."""
    x = np.asarray(x, f32)
    return np.array(_powf_array(x, f32(y)), dtype=f32).reshape(x.shape)


# ------------------------------------------------------------------ scaled conversion
def representable(value, dtype):
    """static_cast<T>(value) of a double is defined: for an integer T when the truncated value is in range, for float when a finite
    value is within its range, always for double."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return not np.isfinite(value) or abs(value) <= float(np.finfo(f32).max)
    if dtype.kind == "f":
        return True
    if value != value:
        return False
    t = float(np.trunc(f64(value)))
    info = np.iinfo(dtype)
    return float(info.min) <= t < 2.0 ** (info.bits - (1 if info.min < 0 else 0))


def old_fill(oldFill, dtype):
    """(IN)oldFill, or None where it does not exist: then the data has no fill value (documented divergence)."""
    dtype = np.dtype(dtype)
    if not representable(oldFill, dtype):
        return None
    if dtype.kind == "f":
        return dtype.type(oldFill)
    return dtype.type(int(np.trunc(f64(oldFill))))


def mifi_round(d):
    """MetNoFimex::round(double) (Utils.h:72-75) on a float64 array: lround, half away from zero, then long -> int (the low 32 bits);
    beyond the range of long and for NaN what glibc / x86-64 yields, LONG_MIN, whose int is 0 (divergence D6).  Returns int32."""
    d = np.asarray(d, f64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(d) < 2.0 ** 63
        t = np.trunc(np.where(ok, d, 0.0))
        r = t + np.where(np.abs(np.where(ok, d, 0.0) - t) >= 0.5, np.copysign(1.0, d), 0.0)
    return r.astype(np.int64).astype(np.int32)  # |r| < 2^63: exact; then the wrap-around of (int)


def convert_scaled(data, oldFill, oldScale, oldOffset, outType, newFill, newScale=1.0, newOffset=0.0):
    """ScaleValue<IN, OUT> on a numpy array of a stored type; raises ValueError where the library returns -1."""
    x = np.asarray(data)
    if outType not in DTYPES or not any(np.dtype(t) == x.dtype for t in DTYPES.values()):
        raise ValueError("no numeric CDM type")
    out_t = np.dtype(DTYPES[outType])
    if not representable(newFill, out_t):
        raise ValueError("newFill is not representable in the output type")
    with np.errstate(all="ignore"):
        nf = out_t.type(newFill) if out_t.kind == "f" else out_t.type(int(np.trunc(f64(newFill))))
        a = f64(oldScale) / f64(newScale)                       # Utils.h:453
        b = (f64(oldOffset) - f64(newOffset)) / f64(newScale)   # :454
        fill = old_fill(oldFill, x.dtype)
        hit = np.zeros(x.shape, bool) if fill is None else (x == fill)
        if x.dtype.kind == "f":
            hit |= np.isnan(x)
        d = a * x.astype(f64) + b                               # :459, two roundings
        r = mifi_round(d).astype(out_t) if out_t.kind in "iu" else d.astype(out_t)
    r[hit] = nf
    return r


# ------------------------------------------------------------------ theta2T
RCP = f32(f32(8.31432 / 0.0289644) / f32(1004.0))  # CDMPressureConversions.cc:235-239
PSX1 = f32(f32(1) / f32(1000.0))                   # :237-238


def theta_factor(p):
    """pow(p * psX1, Rcp) of :242, float32."""
    p = np.asarray(p, f32)
    with np.errstate(all="ignore"):
        return c_powf((p * PSX1).astype(f32), RCP)


def theta_to_temperature(theta, p, add_offset=0.0):
    """float32 arrays of one shape -> ((theta + add_offset) * pow(p * psX1, Rcp)) - add_offset in float32."""
    theta, off = np.asarray(theta, f32), f32(add_offset)
    with np.errstate(all="ignore"):
        return (((theta + off).astype(f32) * theta_factor(p)).astype(f32) - off).astype(f32)


# ------------------------------------------------------------------ specific2relative
C1, C2, C3, C4 = f32(610.78), f32(17.269), f32(273.16), f32(35.86)
MOL_WEIGHT_RATIO = 0.622
RH_SCALE = f32(25000)  # relative_humidity_scale_factor, CDMPressureConversions.cc:86


def humidity_es(t):
    """mifi_humidity_es, :114-121: the argument of exp in float32, exp and the product with c1 in float64, the result float32."""
    t = np.asarray(t, f32)
    with np.errstate(all="ignore"):
        x = ((C2 * (t - C3).astype(f32)).astype(f32) / (t - C4).astype(f32)).astype(f32)
        return (f64(C1) * c_exp(x.astype(f64))).astype(f32)


def specific_to_relative(q, t, p):
    """mifi_specific_to_relative_humidity, :132-141: float32 arrays of one shape -> float32 in [0, 100] or NaN."""
    q, t, p = (np.asarray(a, f32) for a in (q, t, p))
    with np.errstate(all="ignore"):
        es = humidity_es(t)
        rh = (100. * q.astype(f64) * p.astype(f64) / (es.astype(f64) * MOL_WEIGHT_RATIO)).astype(f32)
        rh = np.where(rh < 0, f32(0), np.where(rh > 100, f32(100), rh)).astype(f32)
    return rh


def pack_relative_humidity(rh):
    """(short)(25000.f * rh + 0.5), CDMPressureConversions.cc:330: a float32 product, + 0.5 in float64, truncation.  Outside short (undefined
    in the reference) what its x86-64 build yields: truncation to int32, of which the low 16 bits are kept; NaN and |x| >= 2^31 give 0."""
    rh = np.asarray(rh, f32)
    with np.errstate(all="ignore"):
        x = (RH_SCALE * rh).astype(f32).astype(f64) + 0.5
        bad = np.isnan(x) | (np.abs(x) >= 2.0 ** 31)
        i32 = np.trunc(np.where(bad, 0.0, x)).astype(np.int64)
    return (i32 & 0xffff).astype(np.uint16).view(np.int16)


def relative_humidity_short(q, t, p):
    return pack_relative_humidity(specific_to_relative(q, t, p))


# ------------------------------------------------------------------ accumulate / deaccumulate
def _nan0(a):
    return np.where(np.isnan(a), 0.0, a)


def accumulate(data, firstPos=0, prev=None):
    """data [nt][...] of a stored type = positions firstPos .. -> float64 of the same shape.  prev: acc[firstPos - 1] as float64."""
    x = np.asarray(data)
    out = np.empty(x.shape, f64)
    if firstPos > 0 and prev is None:
        raise ValueError("prev is required behind position 0")
    with np.errstate(all="ignore"):
        acc = None if firstPos == 0 else np.asarray(prev, f64).reshape(x.shape[1:])
        for t in range(x.shape[0]):
            pos = firstPos + t
            cur = x[t].astype(f64)  # Data::asDouble()
            if pos == 0:
                acc = cur           # cannot accumulate first, :537
            else:
                acc = cur + (_nan0(acc) if pos == 1 else acc)  # addDataP2Data, :476-491
            out[t] = acc
    return out


def deaccumulate(data, firstPos=0, prev=None):
    """prev: the position in front of the batch, in the type of data."""
    x = np.asarray(data)
    out = np.empty(x.shape, f64)
    if firstPos > 0 and prev is None:
        raise ValueError("prev is required behind position 0")
    with np.errstate(all="ignore"):
        before = None if firstPos == 0 else np.asarray(prev, x.dtype).reshape(x.shape[1:]).astype(f64)
        for t in range(x.shape[0]):
            pos = firstPos + t
            cur = x[t].astype(f64)
            out[t] = cur if pos == 0 else cur - (_nan0(before) if pos == 1 else before)  # :563-575
            before = cur
    return out


# ------------------------------------------------------------------ the reference's object code
class ReferenceLib:
    """mifi_specific_to_relative_humidity of oracle/_ref/libmifi_ref.so."""

    def __init__(self, path):
        self.fn = ctypes.CDLL(path).mifi_specific_to_relative_humidity
        self.fn.argtypes = [ctypes.c_float] * 3
        self.fn.restype = ctypes.c_float

    def specific_to_relative(self, q, t, p):
        q, t, p = (np.ascontiguousarray(a, f32) for a in (q, t, p))
        return np.array([self.fn(a, b, c) for a, b, c in zip(q.ravel().tolist(), t.ravel().tolist(), p.ravel().tolist())], f32).reshape(q.shape)


def reference_lib():
    """The ReferenceLib of oracle/_ref/libmifi_ref.so, or None where build() found no reference tree to compile it from."""
    import oracle
    return ReferenceLib(oracle.ref().path) if oracle.ref() is not None else None


# ------------------------------------------------------------------ cases
def scaled_values(dtype, n, seed, fill):
    """n values of a stored type: random ones over the type's useful range and, from the front, the fill, +-0, halves and extremes."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    fill = old_fill(fill, dtype)  # None where the type cannot hold it
    if dtype.kind == "f":
        v = (np.round(rng.uniform(-300.0, 300.0, n) * 2) / 2).astype(dtype)  # multiples of 0.5: halves both sides of zero
        big = rng.uniform(size=n) < 0.2
        v[big] = rng.uniform(-7e4, 7e4, np.count_nonzero(big)).astype(dtype)
        special = [fill, np.nan, 0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3e9, -3e9, 1e19, -1e19, np.inf, -np.inf, 1e-30]
    else:
        info = np.iinfo(dtype)
        v = rng.integers(max(info.min, -2 ** 40), min(info.max, 2 ** 40), n, dtype=np.int64, endpoint=True).astype(dtype)
        small = rng.uniform(size=n) < 0.5
        v[small] = rng.integers(max(info.min, -300), min(info.max, 300), np.count_nonzero(small), endpoint=True).astype(dtype)
        special = [fill, 0, 1, info.max, info.min, info.max - 1, 3, 5, 7]
        if info.min < 0:
            special += [-1, -3, -5]
    with np.errstate(all="ignore"):
        for i, s in enumerate(special):
            if s is None:
                continue
            v[(i * 3 + 1) % n] = dtype.type(s) if dtype.kind == "f" else dtype.type(int(s))
    return v


def scaled_parameters(inType, outType, variant):
    """(oldFill, oldScale, oldOffset, newFill, newScale, newOffset) of a (IN, OUT) pair.  Variant 0 unpacks / repacks with newScale != 1
    and produces halves; variant 1 has an oldFill that IN cannot hold (no fill value) and results beyond the range of a narrow OUT."""
    i, o = np.dtype(DTYPES[inType]), np.dtype(DTYPES[outType])
    if i.kind == "f":
        oldFill = -32767.0 if variant == 0 else 1e300 if i == np.float32 else np.nan
    else:
        oldFill = float(min(np.iinfo(i).max, 127) - 2) if variant == 0 else (np.nan if inType % 2 else float(np.iinfo(i).max) * 4.0 + 1e3)
    newFill = np.nan if o.kind == "f" else float(min(np.iinfo(o).max, 32767) - 1)
    if variant == 0:
        return oldFill, 0.5, 1.0, newFill, 2.0, 0.5     # a = 0.25, b = 0.25: x.5 and x.25 results from integers
    return oldFill, 1.5, -0.75, newFill, 0.001, 100.0   # a = 1500: past the range of 1- and 2-byte types


def humidity_inputs(seed, shape):
    """(q, T) over physical ranges, T 200-320 K and q 0-0.03, with a NaN in each."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.0, 0.03, shape).astype(f32)
    T = rng.uniform(200.0, 320.0, shape).astype(f32)
    q[rng.uniform(size=shape) < 0.05] = 0.0
    q.reshape(-1)[1] = np.nan
    T.reshape(-1)[q.size // 2] = np.nan
    return q, T


def pressure_levels(seed, kind, nx, ny, nt, nz):
    """vertical_ref.Levels of `kind` in hPa between about 10 and 1050 hPa, with a NaN surface pressure (or level) in one column."""
    import vertical_ref as vr
    rng = np.random.default_rng(seed)
    eta = (np.arange(nz) + 0.5) / nz
    ps = (600.0 + 450.0 * rng.uniform(size=(nt, ny, nx))).astype(f32)
    b = eta ** 2
    ap = 1000.0 * (eta - b) + 10.0
    if kind == vr.HYBRID_SIGMA_AP:
        lv = vr.Levels(kind, nz, ap=ap, b=b, ps=ps)
    elif kind == vr.HYBRID_SIGMA:
        lv = vr.Levels(kind, nz, a=ap / 1000.0, b=b, p0=1000.0, ps=ps)
    elif kind == vr.SIGMA:
        lv = vr.Levels(kind, nz, sigma=eta, ptop=10.0, ps=ps)
    elif kind == vr.AXIS:
        lv = vr.Levels(kind, nz, axis=10.0 + 1040.0 * eta)
    else:
        lv = vr.Levels(vr.FIELD, nz, field=(10.0 + 1040.0 * rng.uniform(size=(nt, nz, ny, nx))).astype(f32))
    if lv.ps is not None:
        lv.ps[0, ny - 1, nx - 2] = np.nan
    elif lv.field is not None:
        lv.field[0, 0, ny - 1, nx - 2] = np.nan
    return lv


def accumulate_input(seed, dtype, nt, n):
    """[nt][n] of a stored type; the floating ones carry NaN at position 0 and later."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dtype.kind == "f":
        x = rng.uniform(-5.0, 50.0, (nt, n)).astype(dtype)
        x[0, ::7] = np.nan
        x[-1, 3::11] = np.nan
        if nt > 2:
            x[2, 5::13] = np.nan
    else:
        x = rng.integers(-300, 30000, (nt, n)).astype(dtype)
    return x


# ------------------------------------------------------------------ the recorded fixture
RECORDED_SCALED_VARIANTS = (0, 1)
RECORDED_SCALED_N = 40
RECORDED_ACCUMULATE_TYPES = (CDM_SHORT, CDM_FLOAT, CDM_DOUBLE)
# relative humidity as a fraction outside what a short holds at scale 25000, NaN, and the edges of the range
PACK_CASES = np.array([np.nan, 1.4, 3.0, 0.0, 1.0, 1.31068, 1.3107, 1.31072, 100.0, -0.5, 2.62144, 0.99999], f32)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def recorded_humidity_inputs():
    """(q, t, p): 2000 points over the physical ranges (T 200-320 K, q 0-0.03, p 10-1050 hPa), a few NaN, zero and negative values."""
    rng = np.random.default_rng(700)
    q, t = humidity_inputs(701, (2000,))
    p = rng.uniform(10.0, 1050.0, 2000).astype(f32)
    p[5], p[6], q[7], t[8] = np.nan, 0.0, -0.001, 35.86
    return q, t, p


def recorded_theta_inputs():
    rng = np.random.default_rng(710)
    theta = rng.uniform(250.0, 700.0, 500).astype(f32)
    p = rng.uniform(10.0, 1050.0, 500).astype(f32)
    theta[3], p[4], p[5], p[6] = np.nan, np.nan, 0.0, -5.0
    return theta, p, 273.15


def load_fixture(golden_dir):
    with np.load(os.path.join(golden_dir, FIXTURE)) as z:
        return {k: z[k] for k in z.files}
