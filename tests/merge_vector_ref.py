"""CPU restatement of the reference's grid merging on an x/y vector pair: CDMMerger's reader chain
(src/CDMMerger.cc:212-227) where every CDMInterpolator rotates the pair behind its regrid (src/CDMInterpolator.cc:259-283).  The
reference has no test of a merged vector; the result is pinned by composing parts that are pinned:

  regrid and rotation   oracle.interpolate_values, oracle.vector_reproject_values   tests/test_oracle_vs_reference.py
  smoothing, overlay    merge_ref.border_smooth, merge_ref.overlay                  tests/test_merge_ref.py

Test infrastructure: the product never imports it.
"""
import numpy as np

import merge_ref as mr
import oracle


def identity_matrix(ny, nx):
    """a rotation by nothing as the reference lays it out, (m0, m1, m2, m3) = (1, 0, -0, 0) per cell"""
    m = np.zeros((ny, nx, 4), np.float64)
    m[..., 0] = 1.0
    m[..., 2] = -0.0
    return m.ravel()


def angle_matrix(phi):
    """[ny][nx] angles (radians, NaN allowed) -> the reference's double[4 * ny * nx]: (cos, sin, -sin, phi) per cell"""
    phi = np.asarray(phi, np.float64)
    m = np.empty(phi.shape + (4,), np.float64)
    m[..., 0], m[..., 1], m[..., 2], m[..., 3] = np.cos(phi), np.sin(phi), -np.sin(phi), phi
    return m.ravel()


def regrid_rotate(method, pos, u, v, src_shape, dst_shape, matrix):
    """CDMInterpolator::getDataSlice on a pair: both components through the one plan, then the rotation in place"""
    (sy, sx), (dy, dx) = src_shape, dst_shape
    ru = oracle.interpolate_values(method, pos[0], pos[1], u, sx, sy, dx, dy)
    rv = oracle.interpolate_values(method, pos[0], pos[1], v, sx, sy, dx, dy)
    return oracle.vector_reproject_values(matrix, ru, rv, dx, dy)


def merge_vector(Iu, Iv, Ou, Ov, pos, shapes, matrices, method=oracle.BILINEAR, smooth_method=oracle.BILINEAR, tw=5, bw=2, use_outer=True,
                 outer_method=None):
    """pos: merge_ref.merge_positions' three pairs; shapes: ((iy, ix), (oy, ox), (ty, tx)); matrices: (R_oi on the inner grid, R_st
    and R_ot on the target), each the reference's double[4 * cells]; outer_method: the method of the outer -> target regrid where it
    is not `method`.  -> (outU, outV, Su, Sv)"""
    inner, outer, target = shapes
    p_oi, p_st, p_ot = pos
    R_oi, R_st, R_ot = matrices
    Iu, Iv = (np.asarray(a, np.float32).reshape((-1,) + tuple(inner)) for a in (Iu, Iv))
    Ou, Ov = (np.asarray(a, np.float32).reshape((-1,) + tuple(outer)) for a in (Ou, Ov))
    OIu, OIv = regrid_rotate(smooth_method, p_oi, Ou, Ov, outer, inner, R_oi)                               # step 1
    Su, Sv = mr.border_smooth(Iu, OIu, tw, bw, use_outer), mr.border_smooth(Iv, OIv, tw, bw, use_outer)     # step 2
    STu, STv = regrid_rotate(method, p_st, Su, Sv, inner, target, R_st)                                     # step 3
    OTu, OTv = regrid_rotate(method if outer_method is None else outer_method, p_ot, Ou, Ov, outer, target, R_ot)
    return mr.overlay(STu, OTu), mr.overlay(STv, OTv), Su, Sv                                               # step 4
