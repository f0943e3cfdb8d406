"""CPU restatement of the reference's grid merging on an x/y vector pair in its stored types:
CDMMerger's reader chain (src/CDMMerger.cc:212-227) on a pair whose four fields -- inner u, inner v, outer u, outer v -- are packed,
each with its own packing.  The reference has no test of a merged vector, and its classes sit behind libraries that are not built
here: parity is pinned through the parts this restatement is composed of, which other tests pin to the reference:

  regrid_rotate_typed   CDMInterpolator::getDataSlice on a pair (src/CDMInterpolator.cc:255-285): oracle.data2interpolation_array,
                        oracle.interpolate_values, oracle.vector_reproject_values on the raw counts, oracle.interpolation_array2data
                        per component with its own type and fill value             tests/test_oracle_vs_reference.py
  smoothing, overlay    merge_typed_ref.smooth_typed, merge_typed_ref.overlay_typed  tests/test_merge_typed_ref.py

Consequences of the reference's order of work, restated here as they are: the rotation acts on counts, so an add_offset is not
rotated with the value and two components with different scales are rotated as if they had one; an undefined count in either
regridded component, or a NaN matrix cell, makes both rotated components the fill value; a rotated count outside the type's range
wraps through long -> int -> T.  Test infrastructure: the product never imports it.
"""
import collections

import numpy as np

import merge_typed_ref as mt
import oracle


def regrid_rotate_typed(method, pos, U, pU, V, pV, src_shape, dst_shape, matrix):
    """fimex_amd_regrid_apply_vector_typed_device -> (the pair in its stored types, the rotated float pair in front of
    interpolationArray2Data)"""
    (sy, sx), (dy, dx) = src_shape, dst_shape
    r = []
    for X, p in ((U, pU), (V, pV)):
        f = oracle.data2interpolation_array(np.ascontiguousarray(X, mt.dtype_of(p)), p.fill)
        r.append(oracle.interpolate_values(method, pos[0], pos[1], f.reshape(-1, sy, sx), sx, sy, dx, dy))
    ru, rv = oracle.vector_reproject_values(matrix, r[0], r[1], dx, dy)
    return oracle.interpolation_array2data(ru, pU.type, pU.fill), oracle.interpolation_array2data(rv, pV.type, pV.fill), (ru, rv)


MergedPair = collections.namedtuple("MergedPair", "outU outV Su Sv branchU branchV OI_float ST_float OT_float")


def merge_vector_typed(Iu, pIu, Iv, pIv, Ou, pOu, Ov, pOv, pos, shapes, matrices, method=oracle.BILINEAR, smooth_method=oracle.BILINEAR, tw=5,
                       bw=2, use_outer=True, outer_method=None):
    """steps 1-4.  pos: merge_ref.merge_positions' three pairs; shapes: ((iy, ix), (oy, ox), (ty, tx)); matrices: (R_oi on the inner
    grid, R_st and R_ot on the target), each the reference's double[4 * cells]; outer_method: the method of the outer -> target regrid where it is not
    `method`.  outU has inner u's type and packing, outV inner
    v's; the *_float members are the rotated float pairs of the three regrids, in front of their roundings."""
    inner, outer, target = (tuple(s) for s in shapes)
    p_oi, p_st, p_ot = pos
    R_oi, R_st, R_ot = matrices
    Iu = np.ascontiguousarray(Iu, mt.dtype_of(pIu)).reshape((-1,) + inner)
    Iv = np.ascontiguousarray(Iv, mt.dtype_of(pIv)).reshape((-1,) + inner)
    Ou = np.ascontiguousarray(Ou, mt.dtype_of(pOu)).reshape((-1,) + outer)
    Ov = np.ascontiguousarray(Ov, mt.dtype_of(pOv)).reshape((-1,) + outer)
    OIu, OIv, OI_float = regrid_rotate_typed(smooth_method, p_oi, Ou, pOu, Ov, pOv, outer, inner, R_oi)   # step 1
    Su, branchU = mt.smooth_typed(Iu, pIu, OIu, pOu, tw, bw, use_outer)                                    # step 2
    Sv, branchV = mt.smooth_typed(Iv, pIv, OIv, pOv, tw, bw, use_outer)
    STu, STv, ST_float = regrid_rotate_typed(method, p_st, Su, pIu, Sv, pIv, inner, target, R_st)          # step 3
    OTu, OTv, OT_float = regrid_rotate_typed(method if outer_method is None else outer_method, p_ot, Ou, pOu, Ov, pOv, outer, target, R_ot)
    return MergedPair(mt.overlay_typed(STu, pIu, OTu, pOu), mt.overlay_typed(STv, pIv, OTv, pOv), Su, Sv, branchU, branchV, OI_float, ST_float,
                      OT_float)                                                                             # step 4


S, U = oracle.CDM_SHORT, oracle.CDM_USHORT
P = mt.Packing
# name -> (inner u, inner v, outer u, outer v)
PACKINGS = {
    "w": (P(S, -32768.0, 0.01, 0.0), P(S, -32767.0, 0.01, 0.0), P(S, -32767.0, 0.02, 0.0), P(S, -32768.0, 0.05, -3.0)),  # four different packings
    "same": (P(S, -32768.0, 0.01, 0.0),) * 4,                                                                             # one packing
    # fields rounded to integers: exact .5 ties in front of the roundings
    "ties": (P(S, -32768.0, 1.0, 0.0), P(S, -32767.0, 1.0, 0.0), P(S, -32767.0, 1.0, 0.0), P(S, -32768.0, 1.0, 0.0)),
    # rotated counts beyond +-32767
    "wrap": (P(S, -32768.0, 0.0005, 0.0), P(S, -32767.0, 0.0005, 0.0), P(S, -32767.0, 0.0005, 0.0), P(S, -32768.0, 0.0005, 0.0)),
    # unsigned, the fill value at either end, counts that go negative under rotation
    "u": (P(U, 65535.0, 0.01, -100.0), P(U, 0.0, 0.01, -100.0), P(U, 0.0, 0.02, -200.0), P(U, 65535.0, 0.02, -200.0)),
}


def packed_fields(fields, key):
    """four float fields with NaN holes (Iu, Iv, Ou, Ov) -> [(field in its packing, packing)] * 4; "ties" rounds the fields first"""
    if key == "ties":
        fields = [np.round(np.asarray(f, np.float64)) for f in fields]
    return [(mt.as_packed(f, p), p) for f, p in zip(fields, PACKINGS[key])]


def out_of_range(rotated, p):
    """how many values of a rotated float component leave the range of p's type at interpolationArray2Data"""
    info = np.iinfo(mt.dtype_of(p))
    r = rotated[~np.isnan(rotated)].astype(np.float64)
    return int(np.count_nonzero((r >= info.max + 0.5) | (r <= info.min - 0.5)))
