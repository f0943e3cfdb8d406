"""Grid merging of an x/y vector pair on the GPU (include/fimex_amd.h): the fused entry and its chain against
tests/merge_vector_ref.py, the CPU restatement composed of the pinned oracle parts (regrid, rotation) and the pinned merge parts
(smoothing, overlay).

The bar is bit-identical, NaN positions and the sign of zero included: the rotation is two double products and one double add or
subtract narrowed once, the same IEEE operations in the same order on both sides, and everything else is what
tests/test_gpu_merge.py already holds to that bar.  Every cell is compared; the share of bit-identical cells is printed before the
assertion (test_gpu_merge._identical).
"""
import functools

import numpy as np
import pytest

import merge_ref as mr
import merge_vector_ref as mv
import oracle
from test_gpu_merge import GEOMETRIES as SCALAR_GEOMETRIES, MERGE_CASES, TILE_X, Axes, _dev, _extended_target, _identical, _pos, _stream

pytestmark = pytest.mark.gpu

# an inner grid wider than a tile: two full tiles and a partial one in x, and with tw 5, bw 2 on 11 rows transition bands that overlap in y
INNER_WIDE, OUTER_WIDE = Axes(150, 11, 8.5, 6.25, 1.), Axes(45, 10, 0., 0., 4.)
assert 2 * TILE_X < INNER_WIDE.nx < 3 * TILE_X
GEOMETRIES = dict(SCALAR_GEOMETRIES, wide=(INNER_WIDE, OUTER_WIDE, _extended_target(INNER_WIDE, OUTER_WIDE)))
# NaN holes of the outer field [rows, columns]: under the inner grid and beside it
OUTER_HOLES = {"wide": ((slice(2, 4), slice(10, 12)), (slice(7, 9), slice(3, 5)))}
OUTER_HOLES_DEFAULT = ((slice(9, 11), slice(10, 12)), (slice(20, 22), slice(3, 5)))

B, N, C = oracle.BILINEAR, oracle.NEAREST, oracle.BICUBIC
# (geometry, method of step 1, method of steps 3 and 4, nz, useOuter): the scalar merge's eight and the wide inner grid
CASES = MERGE_CASES + [("wide", B, B, 3, True), ("wide", N, C, 9, False), ("wide", C, N, 1, True)]


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    lib = capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    assert hasattr(lib, "fimex_amd_merge_apply_vector_device")
    return capi


@functools.lru_cache(maxsize=None)
def _positions(geometry):
    inner, outer, target = GEOMETRIES[geometry]
    return _pos(outer, inner), _pos(inner, target), _pos(outer, target)


def _shapes(geometry):
    return tuple(g.shape for g in GEOMETRIES[geometry])


@functools.lru_cache(maxsize=None)
def _footprint(geometry):
    """[ty][tx] the target cells that the inner grid reaches with a nearest-neighbour plan"""
    (iy, ix), _, (ty, tx) = _shapes(geometry)
    return ~np.isnan(oracle.interpolate_values(N, *_positions(geometry)[1], np.zeros((iy, ix), np.float32), ix, iy, tx, ty)[0])


def _angles(shape, seed, nan_cells):
    """an angle field that varies smoothly over more than a full turn, with a patch of exactly 0, a patch of exactly 90 degrees
    (cos = 6.1e-17) and NaN in nan_cells"""
    ny, nx = shape
    j, i = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    phi = 2.4 * np.pi * i / max(nx - 1, 1) + 0.9 * np.sin(j / 5. + seed) - 1.0
    assert phi.max() - phi.min() > 2 * np.pi
    phi[ny // 2:ny // 2 + 2, nx // 3:nx // 3 + 3] = 0.0
    phi[ny // 4:ny // 4 + 2, nx // 2:nx // 2 + 3] = np.pi / 2
    for (y, x) in nan_cells:
        phi[y, x] = np.nan
    return phi


@functools.lru_cache(maxsize=None)
def _matrices(geometry):
    """(R_oi on the inner grid, R_st and R_ot on the target), each with a few NaN cells: R_oi's in the frame, the band and the
    inside, R_st's inside the inner's footprint on the target and beyond it, R_ot's likewise"""
    (iy, ix), _, (ty, tx) = _shapes(geometry)
    inside = np.argwhere(_footprint(geometry))
    beyond = np.argwhere(~_footprint(geometry))
    pick = lambda cells, fractions: [tuple(cells[int(f * (len(cells) - 1))]) for f in fractions]
    R = (mv.angle_matrix(_angles((iy, ix), 0, [(0, 3), (iy // 2, 4), (iy // 2, ix // 2), (iy // 2, ix // 2 + 1), (iy - 4, ix - 5)])),
         mv.angle_matrix(_angles((ty, tx), 1, pick(inside, (0.2, 0.4, 0.45, 0.7, 0.9)) + pick(beyond, (0.3, 0.8)))),
         mv.angle_matrix(_angles((ty, tx), 2, pick(inside, (0.4, 0.6)) + pick(beyond, (0.1, 0.5, 0.9)))))
    for m in R:
        m.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def _fields(geometry, nz):
    """(Iu, Iv, Ou, Ov): NaN holes placed independently in the two inner components (interior, frame, a corner), NaN holes of the
    outer under and beside the inner grid, 1 % scattered in each, one +inf and one -inf"""
    inner, outer, _ = GEOMETRIES[geometry]
    rng = np.random.default_rng(nz * 37 + len(geometry))

    def field(g, k):
        X, Y = g.mesh()
        z = np.arange(nz, dtype=np.float64)[:, None, None]
        return (8 * np.sin(X / 17 + z + k) + 5 * np.cos(Y / 11 - z - k) + rng.normal(0, 0.5, (nz,) + g.shape)).astype(np.float32)

    Iu, Iv, Ou, Ov = field(inner, 0), field(inner, 1), field(outer, 0), field(outer, 1)
    ny, nx = inner.shape
    Iu[:, ny // 2 - 1:ny // 2 + 1, nx // 2 - 2:nx // 2 + 2] = np.nan   # interior
    Iu[0, 0:3, 0:6] = np.nan                                           # frame and transition band, corner
    Iu[:, ny - 4:, nx - 3:] = np.nan                                   # frame, far corner
    Iv[:, ny // 3:ny // 3 + 2, nx // 4:nx // 4 + 4] = np.nan           # interior, elsewhere
    Iv[:, 0:2, nx - 9:nx - 4] = np.nan                                 # frame
    Iv[nz - 1, ny - 3:, 0:4] = np.nan                                  # the other corner
    under, beside = OUTER_HOLES.get(geometry, OUTER_HOLES_DEFAULT)
    Ou[(slice(None),) + under] = np.nan
    Ou[(slice(None),) + beside] = np.nan
    Ov[:, under[0], slice(under[1].start + 1, under[1].stop + 1)] = np.nan
    Ov[:, slice(beside[0].start + 1, beside[0].stop + 1), beside[1]] = np.nan
    for f in (Iu, Iv, Ou, Ov):
        f[rng.random(f.shape) < 0.01] = np.nan
    Iu[0, ny // 2 + 2, nx // 3] = np.inf
    Ov[0, 4, 6] = -np.inf
    for f in (Iu, Iv, Ou, Ov):
        f.setflags(write=False)
    return Iu, Iv, Ou, Ov


@functools.lru_cache(maxsize=None)
def _want(geometry, nz, smooth_method, method, use_outer, tw=5, bw=2):
    out = mv.merge_vector(*_fields(geometry, nz), _positions(geometry), _shapes(geometry), _matrices(geometry), method, smooth_method, tw, bw,
                          use_outer)
    for a in out:
        a.setflags(write=False)
    return out


class Plans:
    """the merge plan of a case with its three regrid plans and its three rotations"""

    def __init__(self, fa, geometry, smooth_method, method, tw=5, bw=2, use_outer=True):
        inner, outer, target = GEOMETRIES[geometry]
        (oix, oiy), (itx, ity), (otx, oty) = _positions(geometry)
        self.regrids = (fa.RegridPlan(smooth_method, oix, oiy, outer.nx, outer.ny, inner.nx, inner.ny),
                        fa.RegridPlan(method, itx, ity, inner.nx, inner.ny, target.nx, target.ny),
                        fa.RegridPlan(method, otx, oty, outer.nx, outer.ny, target.nx, target.ny))
        self.merge = fa.MergePlan(*self.regrids, tw, bw, use_outer)
        R = _matrices(geometry)
        self.rotations = (fa.VectorPlan(R[0], inner.nx, inner.ny), fa.VectorPlan(R[1], target.nx, target.ny), fa.VectorPlan(R[2], target.nx, target.ny))

    def close(self):
        self.merge.close()
        for r in self.rotations:
            r.close()


def _run(fa, plans, entry, inputs, nz, target_shape, fill):
    import torch
    outU = torch.full((nz,) + target_shape, fill, dtype=torch.float32, device="cuda")
    outV = torch.full((nz,) + target_shape, fill - 1, dtype=torch.float32, device="cuda")
    getattr(plans.merge, entry)(*plans.rotations, *[d.data_ptr() for d in inputs], nz, outU.data_ptr(), outV.data_ptr(), _stream())
    return outU.cpu().numpy(), outV.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-m%d-m%d-nz%d-outer%d" % c)
def test_merge_apply_vector(fa, case):
    geometry, smooth_method, method, nz, use_outer = case
    (iy, ix), _, target_shape = _shapes(geometry)
    fields = _fields(geometry, nz)
    Iu, Iv, Ou, Ov = fields
    wantU, wantV, Su, Sv = _want(geometry, nz, smooth_method, method, use_outer)
    # the case holds what it is meant to hold
    for w in (wantU, wantV):
        assert np.isnan(w).any() and np.isfinite(w).mean() > 0.5
    nan_st = np.isnan(_matrices(geometry)[1].reshape(target_shape + (4,))[..., 0]) & _footprint(geometry)
    assert nan_st.sum() >= 3 and np.isfinite(wantU[:, nan_st]).any(), "no cell inside the inner's footprint takes OT because of a NaN cell of R_st"
    assert (np.isnan(Iu) ^ np.isnan(Iv)).any(), "no inner cell with exactly one component undefined"
    band = mr._alpha_planes(ix, iy, 5, 2)[0] == 2
    with np.errstate(invalid="ignore"):
        assert band.any() and np.any(Su[:, band] != Iu[:, band]), "the smoothing changes nothing in the band"
    label = "merge vector %s step1 %d steps34 %d nz %d useOuter %d" % case
    plans = Plans(fa, geometry, smooth_method, method, 5, 2, use_outer)
    inputs = [_dev(f) for f in fields]
    fusedU, fusedV = _run(fa, plans, "apply_vector_device", inputs, nz, target_shape, -7.0)
    chainU, chainV = _run(fa, plans, "apply_vector_chain_device", inputs, nz, target_shape, -17.0)
    for name, fused, chain, want in (("u", fusedU, chainU, wantU), ("v", fusedV, chainV, wantV)):
        _identical(fused, want, "%s %s fused" % (label, name))
        _identical(chain, want, "%s %s chain" % (label, name))
        _identical(fused, chain, "%s %s fused against chain" % (label, name))
    for d, f in zip(inputs, fields):
        assert np.array_equal(d.cpu().numpy().view(np.uint32), f.view(np.uint32)), "an input was written to"
    plans.close()


def test_merge_apply_vector_host(fa):
    geometry, nz = "inside-rotated", 3
    wantU, wantV, _, _ = _want(geometry, nz, B, B, True)
    plans = Plans(fa, geometry, B, B)
    gotU, gotV = plans.merge.apply_vector_host(*plans.rotations, *_fields(geometry, nz))
    _identical(gotU, wantU, "merge vector host u")
    _identical(gotV, wantV, "merge vector host v")
    plans.close()


def test_smoothing_widths_reach_the_fused_kernels(fa):
    """another (tw, bw) than the default through the merge plan: the overlapping bands of a 40 x 36 inner with tw 15, bw 6"""
    geometry, nz = "inside-extended", 3
    wantU, wantV, _, _ = _want(geometry, nz, B, B, True, 15, 6)
    default = _want(geometry, nz, B, B, True)
    assert not np.array_equal(wantU.view(np.uint32), default[0].view(np.uint32))
    plans = Plans(fa, geometry, B, B, 15, 6, True)
    gotU, gotV = _run(fa, plans, "apply_vector_device", [_dev(f) for f in _fields(geometry, nz)], nz, _shapes(geometry)[2], -7.0)
    _identical(gotU, wantU, "merge vector tw 15 bw 6 u")
    _identical(gotV, wantV, "merge vector tw 15 bw 6 v")
    plans.close()


def test_refusals(fa):
    import torch
    geometry = "inside-rotated"
    (iy, ix), (oy, ox), (ty, tx) = _shapes(geometry)
    plans = Plans(fa, geometry, B, B)
    r_oi, r_st, r_ot = plans.rotations
    # one allocation cut into Iu, Iv, Ou, Ov, outU, outV in this order, so that which buffers overlap is known
    sizes = [iy * ix, iy * ix, oy * ox, oy * ox, ty * tx, ty * tx]
    pool = torch.zeros(sum(sizes), dtype=torch.float32, device="cuda")
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    ptrs = [pool.data_ptr() + 4 * int(o) for o in starts]
    ins, (outU, outV) = ptrs[:4], ptrs[4:]
    for entry in (plans.merge.apply_vector_device, plans.merge.apply_vector_chain_device):
        # a vector plan whose grid is not its regrid plan's output grid, in each of the three places
        for rotations in ((r_st, r_st, r_ot), (r_oi, r_oi, r_ot), (r_oi, r_st, r_oi)):
            with pytest.raises(fa.FimexAmdError, match="differs from the (inner|target) grid"):
                entry(*rotations, *ins, 1, outU, outV, _stream())
        # an output buffer that overlaps any other buffer: an input, the other output
        with pytest.raises(fa.FimexAmdError, match="overlaps the outer field's y component"):
            entry(r_oi, r_st, r_ot, *ins, 1, outU, ins[3], _stream())
        with pytest.raises(fa.FimexAmdError, match="overlaps the inner field's x component"):
            entry(r_oi, r_st, r_ot, *ins, 1, ins[0], outV, _stream())
        with pytest.raises(fa.FimexAmdError, match="overlaps the other output"):
            entry(r_oi, r_st, r_ot, *ins, 1, outU, outU + 4, _stream())
        # a NULL buffer with nz > 0; nz == 0 is a successful no-op
        for hole in range(6):
            p = [0 if k == hole else a for k, a in enumerate(ins + [outU, outV])]
            with pytest.raises(fa.FimexAmdError, match="NULL data buffer"):
                entry(r_oi, r_st, r_ot, *p[:4], 1, *p[4:], _stream())
        entry(r_oi, r_st, r_ot, 0, 0, 0, 0, 0, 0, 0, _stream())
    assert float(pool.abs().max()) == 0.0  # nothing was launched by any of them
    if fa.device_count() >= 2:  # plans on another device than the calling thread's
        fa.set_device(1)
        try:
            with pytest.raises(fa.FimexAmdError, match="lives on device"):
                plans.merge.apply_vector_device(r_oi, r_st, r_ot, *ins, 1, outU, outV, 0)
            elsewhere = fa.VectorPlan(_matrices(geometry)[1], tx, ty)  # a vector plan on another device than the merge plan
        finally:
            fa.set_device(0)
        with pytest.raises(fa.FimexAmdError, match="different devices"):
            plans.merge.apply_vector_device(r_oi, elsewhere, r_ot, *ins, 1, outU, outV, _stream())
        elsewhere.close()
    plans.close()
