"""tests/merge_vector_ref.py, the CPU restatement of grid merging on an x/y vector pair.  The reference has no test of a merged
vector, so the restatement is held from three sides: with rotations by nothing it must be two scalar merges (tests/merge_ref.py,
pinned to the reference's known answers) bit for bit; a NaN in one component must spread to the other exactly as the joint rotation
says; and single cells of every kind are worked by hand from the literal formulas of the issue in numpy float64
scalars, the regrids alone taken from the oracle."""
import functools

import numpy as np
import pytest

import merge_ref as mr
import merge_vector_ref as mv
import oracle
from test_gpu_merge import GEOMETRIES, _pos  # the geometries only: nothing of that module's GPU tests runs here

GEOMETRY = "inside-extended"
B = oracle.BILINEAR


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same(got, want):
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(_bits(got)[~gn], _bits(want)[~wn])


@functools.lru_cache(maxsize=None)
def _setup():
    inner, outer, target = GEOMETRIES[GEOMETRY]
    pos = (_pos(outer, inner), _pos(inner, target), _pos(outer, target))
    shapes = (inner.shape, outer.shape, target.shape)
    rng = np.random.default_rng(5)

    def field(shape, nz=2):  # wind-like, no NaN, no zeros
        f = rng.normal(0, 8, (nz,) + shape).astype(np.float32)
        f[f == 0] = 1.0
        return f

    return pos, shapes, field(inner.shape), field(inner.shape), field(outer.shape), field(outer.shape)


def _identities(shapes):
    return mv.identity_matrix(*shapes[0]), mv.identity_matrix(*shapes[2]), mv.identity_matrix(*shapes[2])


@pytest.mark.parametrize("use_outer", [True, False])
def test_identity_rotations_give_two_scalar_merges(use_outer):
    pos, shapes, Iu, Iv, Ou, Ov = _setup()
    outU, outV, Su, Sv = mv.merge_vector(Iu, Iv, Ou, Ov, pos, shapes, _identities(shapes), B, B, 5, 2, use_outer)
    wantU, wSu = mr.merge(Iu, Ou, pos, shapes, B, B, 5, 2, use_outer)
    wantV, wSv = mr.merge(Iv, Ov, pos, shapes, B, B, 5, 2, use_outer)
    assert not np.isnan(Su).any() and np.isnan(outU).sum() == np.isnan(wantU).sum()
    for got, want in ((outU, wantU), (outV, wantV), (Su, wSu), (Sv, wSv)):
        assert _same(got, want)


def test_a_nan_in_one_component_spreads_through_the_rotation():
    """one NaN in Ov, beside the inner grid: outU is NaN exactly where the scalar merge of v is NaN because of it"""
    pos, shapes, Iu, Iv, Ou, Ov = _setup()
    Ov = Ov.copy()
    Ov[:, 20, 3] = np.nan
    clean, _ = mr.merge(Iv, _setup()[5], pos, shapes)
    because, _ = mr.merge(Iv, Ov, pos, shapes)
    cells = np.isnan(because) & ~np.isnan(clean)
    assert cells.any() and not np.isnan(mr.merge(Iu, Ou, pos, shapes)[0])[cells].any()
    outU, outV, Su, Sv = mv.merge_vector(Iu, Iv, Ou, Ov, pos, shapes, _identities(shapes))
    assert np.array_equal(np.isnan(outU), np.isnan(because)) and np.array_equal(np.isnan(outV), np.isnan(because))
    # and under the inner grid the smoothing falls back to the inner value in both components
    Ov[:, 10, 11] = np.nan
    _, _, Su, Sv = mv.merge_vector(Iu, Iv, Ou, Ov, pos, shapes, _identities(shapes))
    OIv = oracle.interpolate_values(B, *pos[0], Ov, shapes[1][1], shapes[1][0], shapes[0][1], shapes[0][0])
    hit = np.isnan(OIv)
    assert hit.any() and np.array_equal(_bits(Su)[hit], _bits(Iu)[hit]) and np.array_equal(_bits(Sv)[hit], _bits(Iv)[hit])


# ---- hand-worked cells
def _rot(u, v, m0, m1):
    """u' = (double)u * m0 - (double)v * m1, v' = (double)u * m1 + (double)v * m0, each narrowed to float once"""
    with np.errstate(invalid="ignore", over="ignore"):
        u, v, m0, m1 = np.float64(u), np.float64(v), np.float64(m0), np.float64(m1)
        return np.float32(u * m0 - v * m1), np.float32(u * m1 + v * m0)


def _smooth(branch, alpha, I, O, use_outer):
    """one component of step 2 on one cell, from the issue's contract and CDMBorderSmoothing.cc:129-139"""
    if np.isnan(I):
        return np.float32(O) if use_outer else np.float32(np.nan)
    if np.isnan(O) or branch == mr.INNER:
        return np.float32(I)
    if branch == mr.OUTER:
        return np.float32(O)
    vi, vo = np.float64(I), np.float64(O)
    diff = vo - vi
    return np.float32(vo) if diff == 0 else np.float32(vi + alpha * diff)


@functools.lru_cache(maxsize=None)
def _hand_case(use_outer):
    pos, shapes, Iu, Iv, Ou, Ov = _setup()
    (iy, ix), (oy, ox), (ty, tx) = shapes
    Iu, Iv = Iu.copy(), Iv.copy()
    Iu[:, 17, 21] = np.nan   # interior, u only
    Iv[:, 4, 4] = np.nan     # transition band, v only
    Iu[:, 0, 7] = Iv[:, 0, 7] = np.nan  # frame, both
    j, i = np.meshgrid(np.arange(iy), np.arange(ix), indexing="ij")
    phi_oi = 0.3 + 0.05 * i - 0.04 * j
    j, i = np.meshgrid(np.arange(ty), np.arange(tx), indexing="ij")
    phi_st, phi_ot = 1.1 - 0.03 * i + 0.02 * j, -0.7 + 0.01 * i + 0.05 * j
    # the target cell that lies on inner cell (20, 20): the target continues the inner axes, so it is an exact copy of S there
    inner, outer, target = GEOMETRIES[GEOMETRY]
    tx0, ty0 = int(round((inner.x0 - target.x0) / inner.step)), int(round((inner.y0 - target.y0) / inner.step))
    nan_cell = (ty0 + 20, tx0 + 20)
    phi_st[nan_cell] = np.nan
    R = (mv.angle_matrix(phi_oi), mv.angle_matrix(phi_st), mv.angle_matrix(phi_ot))
    out = mv.merge_vector(Iu, Iv, Ou, Ov, pos, shapes, R, B, B, 5, 2, use_outer)
    regrid = lambda p, f, s, d: oracle.interpolate_values(B, p[0], p[1], f, s[1], s[0], d[1], d[0])
    parts = dict(OIu=regrid(pos[0], Ou, shapes[1], shapes[0]), OIv=regrid(pos[0], Ov, shapes[1], shapes[0]),
                 OTu=regrid(pos[2], Ou, shapes[1], shapes[2]), OTv=regrid(pos[2], Ov, shapes[1], shapes[2]),
                 STu=regrid(pos[1], out[2], shapes[0], shapes[2]), STv=regrid(pos[1], out[3], shapes[0], shapes[2]))
    return (Iu, Iv), R, out, parts, (tx0, ty0), nan_cell


# inner cells (x, y) of the 40 x 36 grid with tw 5, bw 2: xmin1 2, xmax1 7, xmin2 33, xmax2 38; ymin1 2, ymax1 7, ymin2 29, ymax2 34
INNER_CELLS = [((1, 20), mr.OUTER), ((20, 35), mr.OUTER), ((4, 20), mr.BLEND), ((4, 4), mr.BLEND), ((35, 31), mr.BLEND), ((20, 20), mr.INNER),
               ((21, 17), mr.INNER), ((7, 0), mr.OUTER)]


@pytest.mark.parametrize("use_outer", [True, False])
def test_hand_worked_inner_cells(use_outer):
    (Iu, Iv), R, (outU, outV, Su, Sv), parts, _, _ = _hand_case(use_outer)
    (iy, ix) = Iu.shape[1:]
    m = R[0].reshape(iy, ix, 4)
    kinds = set()
    for (x, y), branch in INNER_CELLS:
        got_branch, alpha = mr.linear_alpha(ix, iy, 5, 2, x, y)
        assert got_branch == branch
        for z in range(Iu.shape[0]):
            ou, ov = _rot(parts["OIu"][z, y, x], parts["OIv"][z, y, x], m[y, x, 0], m[y, x, 1])  # step 1
            wu = _smooth(branch, alpha, Iu[z, y, x], ou, use_outer)                               # step 2
            wv = _smooth(branch, alpha, Iv[z, y, x], ov, use_outer)
            assert _same(Su[z, y, x], wu) and _same(Sv[z, y, x], wv), ((x, y, z), Su[z, y, x], wu, Sv[z, y, x], wv)
            kinds.add((branch, bool(np.isnan(Iu[z, y, x])), bool(np.isnan(Iv[z, y, x]))))
    # the outer frame, the blend band and the inside with both components defined; one undefined in the band and inside; both in the frame
    assert kinds >= {(mr.OUTER, False, False), (mr.BLEND, False, False), (mr.INNER, False, False), (mr.BLEND, False, True),
                     (mr.INNER, True, False), (mr.OUTER, True, True)}
    assert np.isnan(Su[0, 17, 21]) != use_outer and not np.isnan(Sv[0, 17, 21])


def test_hand_worked_target_cells():
    (Iu, Iv), R, (outU, outV, Su, Sv), parts, (tx0, ty0), nan_cell = _hand_case(True)
    ty, tx = outU.shape[1:]
    mS, mO = R[1].reshape(ty, tx, 4), R[2].reshape(ty, tx, 4)
    cells = [(ty0 + 20, tx0 + 21), (ty0 + 5, tx0 + 5), (2, 3), (ty - 2, tx - 4), nan_cell]  # inside the footprint, beyond it, the NaN cell of R_st
    took_base = 0
    for (y, x) in cells:
        for z in range(outU.shape[0]):
            su, sv = _rot(parts["STu"][z, y, x], parts["STv"][z, y, x], mS[y, x, 0], mS[y, x, 1])  # step 3
            bu, bv = _rot(parts["OTu"][z, y, x], parts["OTv"][z, y, x], mO[y, x, 0], mO[y, x, 1])
            wu, wv = (bu if np.isnan(su) else su), (bv if np.isnan(sv) else sv)                     # step 4
            assert _same(outU[z, y, x], wu) and _same(outV[z, y, x], wv), ((x, y, z), outU[z, y, x], wu)
            took_base += int(np.isnan(su))
    assert took_base == 3 * outU.shape[0]
    # ST undefined -> OT: beyond the inner grid the regrid of S is undefined
    assert np.isnan(parts["STu"][0, 2, 3]) and not np.isnan(outU[0, 2, 3])
    # the NaN cell of R_st lies on inner cell (20, 20): ST is defined there, the rotated pair is not, the outer pair is taken
    y, x = nan_cell
    assert not np.isnan(parts["STu"][0, y, x]) and not np.isnan(parts["STv"][0, y, x])
    bu, bv = _rot(parts["OTu"][0, y, x], parts["OTv"][0, y, x], mO[y, x, 0], mO[y, x, 1])
    assert np.array_equal(_bits(outU[0, y, x]), _bits(bu)) and np.array_equal(_bits(outV[0, y, x]), _bits(bv))
