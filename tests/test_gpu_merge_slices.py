"""The z loops and the stencil pairs of the fused merge kernels (csrc/merge_launch.hpp and the four merge*.hip), which the cases of
the four test_gpu_merge*.py modules leave out: those use one method for both target plans and 1, 3 or 9 slices.

Geometry "inside-rotated" with 7 slices.  The inner grid is 40 x 36 (nine tiles), the target 137 x 47, so tile_grid gives four
slices per block and two z chunks: chunk 0 is a whole group of four (for the pair kernels two groups of two, or four of one), chunk
1 the remaining three slices one by one (for the bilinear pair kernels a group of two and one slice).  Every kernel instance runs
its group path, its tail path and a second z chunk in one launch.

All nine (inner -> target, outer -> target) method pairs, the method of step 1 cycled so that each smoothing stencil occurs three
times, useOuter alternating; the stored-type entries on short and on unsigned short.  The bar is that of the four modules, bit for
bit: fused == chain, and both == the CPU restatement.  Every output has guard elements in front of it and behind it.
"""
import functools

import numpy as np
import pytest

import merge_ref as mr
import merge_typed_ref as mt
import merge_vector_ref as mv
import merge_vector_typed_ref as mvt
import oracle
import test_gpu_merge as tm
import test_gpu_merge_typed as tt
import test_gpu_merge_vector as tgv
import test_gpu_merge_vector_typed as tvt

pytestmark = pytest.mark.gpu

GEOMETRY, NZ = "inside-rotated", 7
GUARD = 256  # elements in front of and behind every output
METHODS = (oracle.NEAREST, oracle.BILINEAR, oracle.BICUBIC)
# (method of step 1, method of inner -> target, method of outer -> target, useOuter)
CASES = [(METHODS[(i + j) % 3], METHODS[i], METHODS[j], (3 * i + j) % 2 == 0) for i in range(3) for j in range(3)]
assert all(sum(c[0] == m for c in CASES) == 3 for m in METHODS) and {c[3] for c in CASES} == {True, False}
assert len({c[1:3] for c in CASES}) == 9
IDS = ["s%d-st%d-ot%d-outer%d" % c for c in CASES]


def test_the_launch_layout_is_the_one_described():
    """tile_grid (csrc/merge_launch.hpp) restated: 256 * 8 * 4 workgroups wanted, chunks of a multiple of four slices"""
    inner, _, target = tm.GEOMETRIES[GEOMETRY]
    assert (inner.nx, inner.ny, target.nx, target.ny) == (40, 36, 137, 47)
    for g, tiles in ((inner, 9), (target, 36)):
        assert -(-g.nx // tm.TILE_X) * -(-g.ny // tm.TILE_Y) == tiles
        chunks = min(-(-256 * 8 * 4 // tiles), NZ)
        z_per_block = -(-(-(-NZ // chunks)) // 4) * 4
        assert z_per_block == 4 and -(-NZ // z_per_block) == 2 and NZ - z_per_block == 3


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


class Guarded:
    """an output of `like`'s shape and type on the device with GUARD elements of a pattern on either side"""

    def __init__(self, like, value):
        import torch
        self.like, self.size = like, like.dtype.itemsize
        self.t = torch.full((like.nbytes + 2 * GUARD * self.size,), value, dtype=torch.uint8, device="cuda")
        self.value = value
        self.ptr = self.t.data_ptr() + GUARD * self.size

    def result(self, label):
        raw = self.t.cpu().numpy()
        lead = GUARD * self.size
        guards = np.concatenate([raw[:lead], raw[lead + self.like.nbytes:]])
        assert guards.size == 2 * lead and np.all(guards == self.value), label + ": a guard element was written"
        return raw[lead:lead + self.like.nbytes].view(self.like.dtype).reshape(self.like.shape)


def _plans(fa, smooth_method, st_method, ot_method, use_outer):
    """tgv.Plans with a method of its own for the outer -> target plan"""
    plans = tgv.Plans(fa, GEOMETRY, smooth_method, st_method, 5, 2, use_outer)
    if ot_method != st_method:
        _, outer, target = tgv.GEOMETRIES[GEOMETRY]
        otx, oty = tgv._positions(GEOMETRY)[2]
        regrids = plans.regrids[:2] + (fa.RegridPlan(ot_method, otx, oty, outer.nx, outer.ny, target.nx, target.ny),)
        plans.merge.close()
        plans.regrids, plans.merge = regrids, fa.MergePlan(*regrids, 5, 2, use_outer)
    return plans


def _unchanged(devs, fields):
    for d, f in zip(devs, fields):
        assert np.array_equal(d.cpu().numpy().view(np.uint8).ravel()[-f.nbytes:], np.ascontiguousarray(f).view(np.uint8).ravel()), "an input was written to"


# ------------------------------------------------------------------------------------------------------------------------ float
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_merge_apply(fa, case):
    smooth_method, st_method, ot_method, use_outer = case
    I, O = tm._merge_fields(GEOMETRY, NZ)
    want, _ = mr.merge(I, O, tm._positions(GEOMETRY), tgv._shapes(GEOMETRY), st_method, smooth_method, 5, 2, use_outer, outer_method=ot_method)
    assert np.isnan(want).any() and np.isfinite(want).mean() > 0.5
    plans = _plans(fa, smooth_method, st_method, ot_method, use_outer)
    dI, dO = tm._dev(I), tm._dev(O)
    fused, chain = Guarded(want, 0xA5), Guarded(want, 0x5A)
    plans.merge.apply_device(dI.data_ptr(), dO.data_ptr(), NZ, fused.ptr, tm._stream())
    plans.merge.apply_chain_device(dI.data_ptr(), dO.data_ptr(), NZ, chain.ptr, tm._stream())
    label = "merge nz 7 step1 %d st %d ot %d useOuter %d" % case
    fused, chain = fused.result(label + " fused"), chain.result(label + " chain")
    tm._identical(fused, want, label + " fused")
    tm._identical(chain, want, label + " chain")
    tm._identical(fused, chain, label + " fused against chain")
    _unchanged((dI, dO), (I, O))
    plans.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_merge_apply_vector(fa, case):
    smooth_method, st_method, ot_method, use_outer = case
    fields = tgv._fields(GEOMETRY, NZ)
    wantU, wantV, _, _ = mv.merge_vector(*fields, tgv._positions(GEOMETRY), tgv._shapes(GEOMETRY), tgv._matrices(GEOMETRY), st_method, smooth_method, 5, 2,
                                         use_outer, outer_method=ot_method)
    for w in (wantU, wantV):
        assert np.isnan(w).any() and np.isfinite(w).mean() > 0.5
    plans = _plans(fa, smooth_method, st_method, ot_method, use_outer)
    devs = [tm._dev(f) for f in fields]
    outs = {entry: (Guarded(wantU, value), Guarded(wantV, value)) for entry, value in (("apply_vector_device", 0xA5), ("apply_vector_chain_device", 0x5A))}
    for entry, (gu, gv) in outs.items():
        getattr(plans.merge, entry)(*plans.rotations, *[d.data_ptr() for d in devs], NZ, gu.ptr, gv.ptr, tm._stream())
    label = "merge vector nz 7 step1 %d st %d ot %d useOuter %d" % case
    for k, (name, want) in enumerate((("u", wantU), ("v", wantV))):
        fused, chain = (outs[e][k].result("%s %s" % (label, name)) for e in ("apply_vector_device", "apply_vector_chain_device"))
        tm._identical(fused, want, "%s %s fused" % (label, name))
        tm._identical(chain, want, "%s %s chain" % (label, name))
        tm._identical(fused, chain, "%s %s fused against chain" % (label, name))
    _unchanged(devs, fields)
    plans.close()


# ----------------------------------------------------------------------------------------------------------------- stored types
@functools.lru_cache(maxsize=None)
def _typed_fields(key):
    return tt._fields(GEOMETRY, NZ, key)


@pytest.mark.parametrize("key", ["a", "u"])  # merge_typed_ref.PACKINGS: shorts, unsigned shorts
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_merge_apply_typed(fa, case, key):
    smooth_method, st_method, ot_method, use_outer = case
    rI, pi, rO, po = _typed_fields(key)
    assert rI.dtype == rO.dtype == (np.int16 if key == "a" else np.uint16)
    want = mt.merge_typed(rI, pi, rO, po, mt.positions(GEOMETRY), tt._shapes(GEOMETRY), st_method, smooth_method, 5, 2, use_outer, outer_method=ot_method).out
    fills = tt._is_fill(want, pi)
    assert fills.any() and (~fills).mean() > 0.5
    plans = _plans(fa, smooth_method, st_method, ot_method, use_outer)
    (tI, dI), (tO, dO) = tt._dev(rI), tt._dev(rO)
    fused, chain = Guarded(want, 0xA5), Guarded(want, 0x5A)
    path = plans.merge.apply_typed_device(dI, tt._pk(fa, pi), dO, tt._pk(fa, po), NZ, fused.ptr, tt._stream())
    plans.merge.apply_typed_chain_device(dI, tt._pk(fa, pi), dO, tt._pk(fa, po), NZ, chain.ptr, tt._stream())
    assert path == 1, path
    label = "merge typed %s nz 7 step1 %d st %d ot %d useOuter %d" % ((key,) + case)
    fused, chain = fused.result(label + " fused"), chain.result(label + " chain")
    tt._identical(fused, want, label + " fused")
    tt._identical(chain, want, label + " chain")
    tt._identical(fused, chain, label + " fused against chain")
    _unchanged((tI, tO), (rI, rO))
    plans.close()


@pytest.mark.parametrize("key", ["w", "u"])  # merge_vector_typed_ref.PACKINGS: shorts, unsigned shorts
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_merge_apply_vector_typed(fa, case, key):
    smooth_method, st_method, ot_method, use_outer = case
    packed = tvt._packed(GEOMETRY, NZ, key)
    assert all(a.dtype == (np.int16 if key == "w" else np.uint16) for a, _ in packed)
    (Iu, pIu), (Iv, pIv), (Ou, pOu), (Ov, pOv) = packed
    m = mvt.merge_vector_typed(Iu, pIu, Iv, pIv, Ou, pOu, Ov, pOv, tgv._positions(GEOMETRY), tgv._shapes(GEOMETRY), tgv._matrices(GEOMETRY), st_method,
                               smooth_method, 5, 2, use_outer, outer_method=ot_method)
    for out, p in ((m.outU, pIu), (m.outV, pIv)):
        fills = tvt._is_fill(out, p)
        assert fills.any() and (~fills).mean() > 0.5
    plans = _plans(fa, smooth_method, st_method, ot_method, use_outer)
    devs = [tt._dev(a) for a, _ in packed]
    args = [x for (_, ptr), (_, p) in zip(devs, packed) for x in (ptr, tt._pk(fa, p))]
    fused, chain = (Guarded(m.outU, 0xA5), Guarded(m.outV, 0xA5)), (Guarded(m.outU, 0x5A), Guarded(m.outV, 0x5A))
    path = plans.merge.apply_vector_typed_device(*plans.rotations, *args, NZ, fused[0].ptr, fused[1].ptr, tt._stream())
    plans.merge.apply_vector_typed_chain_device(*plans.rotations, *args, NZ, chain[0].ptr, chain[1].ptr, tt._stream())
    assert path == 1, path
    label = "merge vector typed %s nz 7 step1 %d st %d ot %d useOuter %d" % ((key,) + case)
    for k, (name, want) in enumerate((("u", m.outU), ("v", m.outV))):
        f, c = fused[k].result("%s %s fused" % (label, name)), chain[k].result("%s %s chain" % (label, name))
        tt._identical(f, want, "%s %s fused" % (label, name))
        tt._identical(c, want, "%s %s chain" % (label, name))
        tt._identical(f, c, "%s %s fused against chain" % (label, name))
    _unchanged([t for t, _ in devs], [a for a, _ in packed])
    plans.close()
