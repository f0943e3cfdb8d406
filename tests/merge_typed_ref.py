"""CPU restatement of the reference's grid merging on variables in their stored types, composed of
parts that other tests pin to the reference:

  regrid_typed   data2InterpolationArray, the regrid on the raw counts as floats, interpolationArray2Data: oracle.* (the reference's
                 own C code, tests/test_oracle_vs_reference.py)
  unpack / pack  ScaleValue<T, double> / ScaleValue<double, T> of getScaledDataSlice and convertDataType: derived_ref.convert_scaled
  smooth_typed   CDMBorderSmoothing::getDataSlice (src/CDMBorderSmoothing.cc:101-102, 129-139, 155-159) with merge_ref.linear_alpha,
                 the blend kept in float64
  overlay_typed  CDMOverlay::getDataSlice (src/CDMOverlay.cc:80-92)
  merge_typed    the reader chain of CDMMergerPrivate::makeCDM (src/CDMMerger.cc:212-227); the merged CDM, and with it the packing of
                 every result, is the inner reader's (src/CDMMergeUtils.cc:214-219)

The reference's classes themselves sit behind libraries that are not built here: parity of the composition is pinned through
these parts and through the reference's known answers (tests/test_merge_typed_ref.py).  Test infrastructure: the product never
imports it.
"""
import collections

import numpy as np

import derived_ref as dr
import merge_ref as mr
import oracle

Packing = collections.namedtuple("Packing", "type fill scale offset")
NAN = float("nan")


def dtype_of(p):
    return np.dtype(dr.DTYPES[p.type])


def regrid_typed(method, px, py, X, p, inX, inY, outX, outY):
    """fimex_amd_regrid_apply_typed_device on X [nz][inY][inX] of p.type with p.fill -> (the result in p.type, the regrid's float
    result in front of interpolationArray2Data)"""
    f = oracle.data2interpolation_array(np.ascontiguousarray(X, dtype_of(p)), p.fill)
    r = oracle.interpolate_values(method, px, py, f.reshape(-1, inY, inX), inX, inY, outX, outY)
    return oracle.interpolation_array2data(r, p.type, p.fill), r


def unpack(x, p):
    """getScaledDataSlice: ScaleValue<T, double>(fill, scale, offset, NaN, 1, 0)"""
    return dr.convert_scaled(np.ascontiguousarray(x, dtype_of(p)), p.fill, p.scale, p.offset, dr.CDM_DOUBLE, NAN, 1.0, 0.0)


def pack(d, p):
    """convertDataType(MIFI_UNDEFINED_D, 1, 0, type, fill, scale, offset): ScaleValue<double, T>"""
    return dr.convert_scaled(np.ascontiguousarray(d, np.float64), NAN, 1.0, 0.0, p.type, p.fill, p.scale, p.offset)


# the branch a cell of the smoothing took
INNER_KEPT, BLENDED, OUTER_TAKEN, UNDEFINED = range(4)


def smooth_double(vi, vo, tw=5, bw=2, use_outer=True):
    """:129-139 with Linear :52-58, :84 on float64 fields [..][ny][nx] -> (float64, the branch of every cell)"""
    if tw <= 0:
        raise ValueError("invalid parameter values for linear smoothing")
    assert vi.shape == vo.shape and vi.ndim >= 2 and vi.dtype == vo.dtype == np.float64
    ny, nx = vi.shape[-2:]
    kind, alpha = mr._alpha_planes(nx, ny, tw, bw)  # from merge_ref.linear_alpha, cell by cell
    kind, alpha = np.broadcast_to(kind, vi.shape), np.broadcast_to(alpha, vi.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = vo - vi
        prod = alpha * diff
        blend = np.where(diff == 0, vo, vi + prod)
    smoothed = np.where(kind == 0, vo, np.where(kind == 1, vi, blend))
    inan, onan = np.isnan(vi), np.isnan(vo)
    m = np.where(inan, vo if use_outer else np.float64(np.nan), np.where(onan, vi, smoothed))
    branch = np.where(inan, OUTER_TAKEN if use_outer else UNDEFINED,
                      np.where(onan | (kind == 1), INNER_KEPT, np.where(kind == 0, OUTER_TAKEN, BLENDED)))
    branch = np.where(np.isnan(m), UNDEFINED, branch)
    return m, branch


def smooth_typed(I, pi, OI, po, tw=5, bw=2, use_outer=True):
    """step 2 -> (S in the inner's type and packing, the branch of every cell)"""
    m, branch = smooth_double(unpack(I, pi), unpack(OI, po), tw, bw, use_outer)
    return pack(m, pi), branch


def overlay_typed(top, pt, base, pb):
    """step 4: a defined top value is unpacked and packed again"""
    vt = unpack(top, pt)
    return pack(np.where(np.isnan(vt), unpack(base, pb), vt), pt)


Merged = collections.namedtuple("Merged", "out S branch OI OI_float ST OT OT_float")


def merge_typed(I, pi, O, po, pos, shapes, method=oracle.BILINEAR, smooth_method=oracle.BILINEAR, tw=5, bw=2, use_outer=True, outer_method=None):
    """steps 1-4 on I [nz][iy][ix] in packing pi and O [nz][oy][ox] in packing po.  pos: merge_ref.merge_positions' three pairs;
    shapes: ((iy, ix), (oy, ox), (ty, tx)); outer_method: the method of the outer -> target regrid where it is not `method`."""
    (iy, ix), (oy, ox), (ty, tx) = shapes
    (oi_x, oi_y), (it_x, it_y), (ot_x, ot_y) = pos
    I = np.ascontiguousarray(I, dtype_of(pi)).reshape(-1, iy, ix)
    O = np.ascontiguousarray(O, dtype_of(po)).reshape(-1, oy, ox)
    OI, OI_float = regrid_typed(smooth_method, oi_x, oi_y, O, po, ox, oy, ix, iy)  # step 1
    S, branch = smooth_typed(I, pi, OI, po, tw, bw, use_outer)                      # step 2
    ST, _ = regrid_typed(method, it_x, it_y, S, pi, ix, iy, tx, ty)                 # step 3
    OT, OT_float = regrid_typed(method if outer_method is None else outer_method, ot_x, ot_y, O, po, ox, oy, tx, ty)
    return Merged(overlay_typed(ST, pi, OT, po), S, branch, OI, OI_float, ST, OT, OT_float)  # step 4


def as_packed(field, p):
    """a float field with NaN holes as a variable in packing p: pack() of its values"""
    return pack(np.asarray(field, np.float64), p)


# ---- the synthetic geometries and fields of tests/test_gpu_merge.py (definitions copied)
class Axes:
    """a grid in a common plane: cell (i, j) lies at origin + i * ex * step + j * ey * step, ex the unit vector at `angle`"""

    def __init__(self, nx, ny, x0, y0, step, angle=0.0):
        self.nx, self.ny, self.x0, self.y0, self.step, self.angle = nx, ny, x0, y0, step, angle

    @property
    def shape(self):
        return self.ny, self.nx

    def mesh(self):
        i, j = np.meshgrid(np.arange(self.nx, dtype=np.float64), np.arange(self.ny, dtype=np.float64))
        c, s = np.cos(self.angle), np.sin(self.angle)
        return self.x0 + self.step * (c * i - s * j), self.y0 + self.step * (s * i + c * j)

    def index_of(self, X, Y):
        c, s = np.cos(self.angle), np.sin(self.angle)
        dx, dy = (X - self.x0) / self.step, (Y - self.y0) / self.step
        return (c * dx + s * dy).ravel(), (-s * dx + c * dy).ravel()


def geometries(tile_x=64, tile_y=4):
    outer = Axes(30, 28, 0., 0., 4.)
    inside = Axes(40, 36, 30.5, 28.25, 1.)
    row_out = Axes(40, 36, 30.5, 110.5 - 35., 1.)
    rotated = Axes(2 * tile_x + 9, 2 * tile_y + 39, 22.3, 31.7, 0.83, np.radians(17.))
    x = mr.extend_inner_axis(inside.x0 + inside.step * np.arange(inside.nx), outer.x0 + outer.step * np.arange(outer.nx))
    y = mr.extend_inner_axis(inside.y0 + inside.step * np.arange(inside.ny), outer.y0 + outer.step * np.arange(outer.ny))
    extended = Axes(x.size, y.size, x[0], y[0], inside.step)
    return {"inside-extended": (inside, outer, extended), "inside-rotated": (inside, outer, rotated), "rowout-rotated": (row_out, outer, rotated)}


GEOMETRIES = geometries()


def positions(geometry):
    inner, outer, target = GEOMETRIES[geometry]
    return outer.index_of(*inner.mesh()), inner.index_of(*target.mesh()), outer.index_of(*target.mesh())


def float_fields(geometry, nz):
    """tests/test_gpu_merge.py's fields: NaN holes in the inner's interior and frame, in the outer under and beside the inner, 1 %
    scattered"""
    inner, outer, _ = GEOMETRIES[geometry]
    rng = np.random.default_rng(nz * 31 + len(geometry))

    def field(g):
        X, Y = g.mesh()
        z = np.arange(nz, dtype=np.float64)[:, None, None]
        return (280 + 5 * np.sin(X / 17 + z) + 3 * np.cos(Y / 11 - z) + rng.normal(0, 0.3, (nz,) + g.shape)).astype(np.float32)

    I, O = field(inner), field(outer)
    I[:, 15:19, 20:24] = np.nan
    I[0, 0:3, 0:6] = np.nan
    I[:, 30:36, 37:40] = np.nan
    I[rng.random(I.shape) < 0.01] = np.nan
    O[:, 9:11, 10:12] = np.nan
    O[:, 20:22, 3:5] = np.nan
    O[rng.random(O.shape) < 0.01] = np.nan
    return I, O


# ---- the packings of the tests: name -> (inner, outer, what is added to the outer field before it is packed)
_A_INNER, _A_OUTER = Packing(dr.CDM_SHORT, -32768.0, 0.01, 273.15), Packing(dr.CDM_SHORT, -32767.0, 0.02, 250.0)
PACKINGS = {
    "a": (_A_INNER, _A_OUTER, 0.0),                                   # two packings of one type
    "b": (_A_INNER, _A_INNER, 0.0),                                   # one packing for both
    "c": (Packing(dr.CDM_SHORT, -32768.0, 1.0, 0.0), Packing(dr.CDM_SHORT, -32767.0, 1.0, 0.0), 0.0),  # integer-valued fields: exact .5 ties
    "d": (Packing(dr.CDM_SHORT, -32768.0, 0.001, 280.0), _A_OUTER, -40.0),  # outer values near 240 leave the inner's short range: they wrap
    # unsigned shorts, the fill value at either end of the range; outer values near 340 leave the inner's range (327.675) and wrap
    "u": (Packing(dr.CDM_USHORT, 65535.0, 0.005, 0.0), Packing(dr.CDM_USHORT, 0.0, 0.02, 200.0), 60.0),
    "e-int-short": (Packing(dr.CDM_INT, -2147483648.0, 0.001, 0.0), _A_OUTER, 0.0),
    "e-uchar-uchar": (Packing(dr.CDM_UCHAR, 255.0, 0.1, 268.0), Packing(dr.CDM_UCHAR, 0.0, 0.125, 265.0), 0.0),
    # two types of one element size: in place on the outer (base) is permitted
    "e-int-float": (Packing(dr.CDM_INT, -2147483648.0, 0.001, 0.0), Packing(dr.CDM_FLOAT, 9.9692099683868690e+36, 1.0, 0.0), 0.0),
    "e-short-ushort": (_A_INNER, Packing(dr.CDM_USHORT, 0.0, 0.02, 200.0), 0.0),
    "e-float-double": (Packing(dr.CDM_FLOAT, 9.9692099683868690e+36, 1.0, 0.0), Packing(dr.CDM_DOUBLE, NAN, 0.5, 100.0), 0.0),
    "e-double-double": (Packing(dr.CDM_DOUBLE, 9.9692099683868690e+36, 1.0, 0.0), Packing(dr.CDM_DOUBLE, -999.0, 2.0, -10.0), 0.0),
}
FUSED = ("a", "b", "c", "d", "u")  # the pairs the fused kernels serve
CHAINED = tuple(k for k in PACKINGS if k.startswith("e-"))


def packed_fields(I, O, key):
    """float fields with NaN holes -> (I in the inner's packing, pi, O in the outer's, po)"""
    pi, po, shift = PACKINGS[key]
    return as_packed(I, pi), pi, as_packed(np.asarray(O, np.float64) + shift, po), po


def raw_fields(key, seed, shape):
    """both variables of a packing pair: packed values around 280 with 10 % fill values each, and 5 % raw counts from the whole
    range of the type (values whose blend leaves the inner's range and wraps)"""
    rng = np.random.default_rng(seed)
    pi, po, shift = PACKINGS[key]
    out = []
    for p, add in ((pi, 0.0), (po, shift)):
        v = rng.normal(280, 5, shape) + add
        v[rng.random(shape) < 0.1] = np.nan
        raw = pack(v, p)
        wild = rng.random(shape) < 0.05
        if raw.dtype.kind in "iu":
            info = np.iinfo(raw.dtype)
            raw[wild] = rng.integers(info.min, info.max, size=int(wild.sum()), endpoint=True).astype(raw.dtype)
        else:
            raw[wild] = (rng.normal(0, 1e3, int(wild.sum()))).astype(raw.dtype)
            raw[rng.random(shape) < 0.02] = np.nan
        out.append(raw)
    return out[0], pi, out[1], po


# ---- the reference's own cases (test/testMerger.cc) in their stored types
_STORED = {"test_merger": ("test_merge_inner.nc", "test_merge_outer.nc", "ga_2t_1"),
           "test_merge_target": ("merge_target_base.nc", "merge_target_top.nc", "air_temperature_2m")}


def _stored(f, var):
    v = f.variables[var]
    a = np.array(v.data)
    a = a.astype(a.dtype.newbyteorder("=")).reshape((-1,) + a.shape[-2:])
    fill = getattr(v, "_FillValue", None)
    if fill is None:  # CDM::getFillValue (src/CDM.cc:486-500): the netCDF default of the type
        fill = {"f": np.float32(9.9692099683868690e+36), "d": 9.9692099683868690e+36}[a.dtype.char]
    p = Packing(oracle.cdm_type_of(a.dtype), float(fill), float(getattr(v, "scale_factor", 1.0)), float(getattr(v, "add_offset", 0.0)))
    return np.ascontiguousarray(a), p


def load_case_stored(golden_dir, name):
    """-> (I, pi, O, po): the two variables of merge_ref.load_case(name) as the files store them"""
    inner, outer, var = _STORED[name]
    I, pi = _stored(mr._read(golden_dir, inner), var)
    O, po = _stored(mr._read(golden_dir, outer), var)
    return I, pi, O, po
