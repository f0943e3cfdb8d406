"""tests/merge_vector_typed_ref.py, the CPU restatement of the merge of a packed x/y vector pair, held against what
is pinned already and against cells worked by hand.  The reference has no test of a merged vector:

  1  with rotations by nothing and the same undefined cells in u and v of each grid, the result is that of two scalar typed merges
     (merge_typed_ref.merge_typed, pinned by tests/test_merge_typed_ref.py), byte for byte
  2  with all four fields CDM_FLOAT, fill NaN, scale 1 and offset 0 the result is merge_vector_ref.merge_vector's, bit for bit
  3  a handful of cells of every kind worked by hand in numpy float64 scalars

No GPU is involved."""
import numpy as np
import pytest

import merge_typed_ref as mt
import merge_vector_ref as mv
import merge_vector_typed_ref as mvt
import oracle
import test_gpu_merge_vector as tgv

B, N, C = oracle.BILINEAR, oracle.NEAREST, oracle.BICUBIC
GEOMETRY = "inside-rotated"


def _bytes_equal(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    same = got.view(np.uint8).reshape(-1, got.dtype.itemsize) == want.view(np.uint8).reshape(-1, want.dtype.itemsize)
    assert same.all(), "%s: %d elements differ" % (label, np.count_nonzero(~same.all(axis=1)))


def _common_holes(fields):
    """the float fields of tests/test_gpu_merge_vector.py with the undefined cells of u and v of each grid made the same"""
    Iu, Iv, Ou, Ov = (np.array(f, np.float64) for f in fields)
    hi, ho = np.isnan(Iu) | np.isnan(Iv), np.isnan(Ou) | np.isnan(Ov)
    Iu[hi], Iv[hi], Ou[ho], Ov[ho] = np.nan, np.nan, np.nan, np.nan
    return Iu, Iv, Ou, Ov


@pytest.mark.parametrize("key", ["w", "wrap", "u"])
@pytest.mark.parametrize("methods", [(B, B), (N, C)], ids=["bilinear-bilinear", "nearest-bicubic"])
def test_rotations_by_nothing_give_two_scalar_merges(methods, key):
    smooth_method, method = methods
    nz = 3
    shapes, pos = tgv._shapes(GEOMETRY), tgv._positions(GEOMETRY)
    (iy, ix), _, (ty, tx) = shapes
    (Iu, pIu), (Iv, pIv), (Ou, pOu), (Ov, pOv) = mvt.packed_fields(_common_holes(tgv._fields(GEOMETRY, nz)), key)
    identity = (mv.identity_matrix(iy, ix), mv.identity_matrix(ty, tx), mv.identity_matrix(ty, tx))
    got = mvt.merge_vector_typed(Iu, pIu, Iv, pIv, Ou, pOu, Ov, pOv, pos, shapes, identity, method, smooth_method, 5, 2, True)
    wantU = mt.merge_typed(Iu, pIu, Ou, pOu, pos, shapes, method, smooth_method, 5, 2, True)
    wantV = mt.merge_typed(Iv, pIv, Ov, pOv, pos, shapes, method, smooth_method, 5, 2, True)
    _bytes_equal(got.outU, wantU.out, "outU")
    _bytes_equal(got.outV, wantV.out, "outV")
    _bytes_equal(got.Su, wantU.S, "Su")
    _bytes_equal(got.Sv, wantV.S, "Sv")
    fill = mt.pack(np.array([np.nan]), pIu)[0]
    assert (got.outU == fill).any() and (got.outU != fill).mean() > 0.5


@pytest.mark.parametrize("use_outer", [True, False], ids=["outer1", "outer0"])
def test_float_fields_give_the_float_vector_merge(use_outer):
    nz = 3
    shapes, pos, R = tgv._shapes(GEOMETRY), tgv._positions(GEOMETRY), tgv._matrices(GEOMETRY)
    fields = tgv._fields(GEOMETRY, nz)
    p = mt.Packing(oracle.CDM_FLOAT, float("nan"), 1.0, 0.0)
    got = mvt.merge_vector_typed(fields[0], p, fields[1], p, fields[2], p, fields[3], p, pos, shapes, R, B, B, 5, 2, use_outer)
    wantU, wantV, Su, Sv = mv.merge_vector(*fields, pos, shapes, R, B, B, 5, 2, use_outer)
    for g, w, label in ((got.outU, wantU, "outU"), (got.outV, wantV, "outV"), (got.Su, Su, "Su"), (got.Sv, Sv, "Sv")):
        gn, wn = np.isnan(g), np.isnan(w)
        assert np.array_equal(gn, wn) and np.array_equal(g.view(np.uint32)[~gn], w.view(np.uint32)[~wn]), label
    assert np.isnan(wantU).any() and np.isfinite(wantU).mean() > 0.5


# ---------------------------------------------------------------------------------------------------- cells worked by hand
f64, f32 = np.float64, np.float32
NX, NY, TW, BW = 15, 17, 5, 2


def _to_stored(f, p):
    """interpolationArray2Data on one float: NaN -> the fill value, else lround and long -> int -> T"""
    if np.isnan(f):
        return int(p.fill)
    r = int(np.trunc(f64(f)) + (np.copysign(1.0, f64(f)) if abs(f64(f) - np.trunc(f64(f))) >= 0.5 else 0.0))
    bits = 8 * mt.dtype_of(p).itemsize
    r &= (1 << bits) - 1
    return r - (1 << bits) if mt.dtype_of(p).kind == "i" and r >= 1 << (bits - 1) else r


def _as_float(count, p):
    """data2InterpolationArray on one count"""
    return f32(np.nan) if count == int(p.fill) else f32(count)


def _unpack(count, p):
    return f64(np.nan) if count == int(p.fill) else f64(p.scale) / f64(1.0) * f64(count) + (f64(p.offset) - f64(0.0)) / f64(1.0)


def _pack(d, p):
    if np.isnan(d):
        return int(p.fill)
    return _to_stored_d(f64(1.0) / f64(p.scale) * d + (f64(0.0) - f64(p.offset)) / f64(p.scale), p)


def _to_stored_d(d, p):
    r = int(np.trunc(d) + (np.copysign(1.0, d) if abs(d - np.trunc(d)) >= 0.5 else 0.0))
    bits = 8 * mt.dtype_of(p).itemsize
    r &= (1 << bits) - 1
    return r - (1 << bits) if mt.dtype_of(p).kind == "i" and r >= 1 << (bits - 1) else r


def _rotated(cu, pU, cv, pV, m):
    """regridRotT on one cell where the regrid is a copy: counts -> floats, the rotation, each component back to its type"""
    u, v = _as_float(cu, pU), _as_float(cv, pV)
    un = f64(u) * f64(m[0]) - f64(v) * f64(m[1])
    vn = f64(u) * f64(m[1]) + f64(v) * f64(m[0])
    return _to_stored(f32(un), pU), _to_stored(f32(vn), pV)


def _smoothed(ci, pI, co, pO, kind, alpha, use_outer):
    vi, vo = _unpack(ci, pI), _unpack(co, pO)
    if np.isnan(vi):
        return _pack(vo if use_outer else f64(np.nan), pI)
    if kind == "inner" or np.isnan(vo):
        return _pack(vi, pI)
    if kind == "frame":
        return _pack(vo, pI)
    diff = vo - vi
    return _pack(vo if diff == 0 else vi + f64(alpha) * diff, pI)


def _overlaid(ct, pI, cb, pO):
    vt = _unpack(ct, pI)
    return _pack(_unpack(cb, pO) if np.isnan(vt) else vt, pI)


# (y, x) -> (kind, alpha) with tw 5, bw 2 on 15 x 17: the frame is x < 2, the band 2 <= x < 7 with alpha (7 - x) / 5 in the middle rows
CELLS = {"frame": ((8, 0), "frame", 0.0), "band": ((8, 4), "band", 3.0 / 5.0), "inner": ((8, 8), "inner", 0.0),
         "inner-u-undefined": ((9, 8), "inner", 0.0), "both-undefined": ((7, 8), "inner", 0.0), "nan-R_st": ((10, 8), "inner", 0.0),
         "band-v-undefined": ((9, 4), "band", 3.0 / 5.0)}


@pytest.mark.parametrize("use_outer", [True, False], ids=["outer1", "outer0"])
@pytest.mark.parametrize("key", ["w", "u", "wrap"])
def test_cells_worked_by_hand(key, use_outer):
    """all three grids are one 15 x 17 grid and the regrids nearest-neighbour at the cells' own positions, so that every regrid is
    a copy and a cell depends on its own four counts and its three matrices alone"""
    rng = np.random.default_rng(7)
    fields = [rng.normal(0, 8, (1, NY, NX)) for _ in range(4)]
    for f in fields:
        f[rng.random(f.shape) < 0.1] = np.nan
    for (y, x), _, _ in CELLS.values():
        for k, f in enumerate(fields):
            f[0, y, x] = 3.25 + k - 0.5 * y + 0.75 * x
    fields[0][0, 9, 8] = np.nan                           # inner u undefined, inner v defined
    fields[1][0, 9, 4] = np.nan                           # in the band: inner v undefined
    fields[0][0, 7, 8], fields[1][0, 7, 8] = np.nan, np.nan  # both undefined: S is undefined without useOuter, ST undefined -> OT
    phis = [rng.uniform(-3, 3, (NY, NX)) for _ in range(3)]
    phis[1][10, 8] = np.nan                               # a NaN cell of R_st on a defined ST
    R = [mv.angle_matrix(phi) for phi in phis]
    (Iu, pIu), (Iv, pIv), (Ou, pOu), (Ov, pOv) = mvt.packed_fields(fields, key)
    j, i = np.meshgrid(np.arange(NY, dtype=np.float64), np.arange(NX, dtype=np.float64), indexing="ij")
    here = (i.ravel(), j.ravel())
    got = mvt.merge_vector_typed(Iu, pIu, Iv, pIv, Ou, pOu, Ov, pOv, (here,) * 3, ((NY, NX),) * 3, R, N, N, TW, BW, use_outer)
    fill_u = int(pIu.fill)
    seen_ot = False
    for name, ((y, x), kind, alpha) in CELLS.items():
        m = [r.reshape(NY, NX, 4)[y, x] for r in R]
        ciu, civ, cou, cov = (int(a[0, y, x]) for a in (Iu, Iv, Ou, Ov))
        oiu, oiv = _rotated(cou, pOu, cov, pOv, m[0])                                                 # step 1
        su, sv = _smoothed(ciu, pIu, oiu, pOu, kind, alpha, use_outer), _smoothed(civ, pIv, oiv, pOv, kind, alpha, use_outer)  # step 2
        assert (int(got.Su[0, y, x]), int(got.Sv[0, y, x])) == (su, sv), (name, "S")
        stu, stv = _rotated(su, pIu, sv, pIv, m[1])                                                   # step 3
        otu, otv = _rotated(cou, pOu, cov, pOv, m[2])
        want = _overlaid(stu, pIu, otu, pOu), _overlaid(stv, pIv, otv, pOv)                           # step 4
        assert (int(got.outU[0, y, x]), int(got.outV[0, y, x])) == want, (name, "out")
        seen_ot |= stu == fill_u and want[0] == _pack(_unpack(otu, pOu), pIu) != fill_u
        if name == "nan-R_st":
            assert su != fill_u and stu == fill_u and stv == int(pIv.fill)
        if name == "both-undefined" and not use_outer:
            assert su == fill_u and stu == fill_u
        if name == "inner-u-undefined":
            assert (su == fill_u) == (not use_outer or oiu == int(pOu.fill)) and sv != int(pIv.fill)
    assert seen_ot, "no hand-worked cell takes OT"
