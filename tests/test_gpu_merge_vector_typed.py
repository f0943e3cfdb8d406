"""Grid merging of an x/y vector pair in its stored types on the GPU (include/fimex_amd.h): the entry with its
dispatch, its chain and its host form against tests/merge_vector_typed_ref.py, the CPU restatement composed of the pinned oracle
parts (counts to floats, regrid, rotation, floats to counts) and the pinned typed merge parts (smoothing, overlay).

The bar is byte for byte on every cell.  No tolerance is needed: the rotation is two double products and one double add or
subtract narrowed once, the roundings and the blend are correctly rounded IEEE operations in the restatement's order, there are no
transcendentals, and the regrids are the ones already bit-exact.  The share of identical elements is printed before each assertion
(test_gpu_merge_typed._identical).

Geometries, float fields and rotation matrices are those of tests/test_gpu_merge_vector.py, packed with merge_typed_ref.as_packed
in the packings of merge_vector_typed_ref.PACKINGS.  Slice counts: that file's CASES (nz 1, 3, 9) and one row with nz 5; with 4
slices per z block on these grids that is the single-slice tail, a partial group, two z blocks and three."""
import functools

import numpy as np
import pytest

import merge_typed_ref as mt
import merge_vector_typed_ref as mvt
import oracle
import test_gpu_merge_vector as tgv
from test_gpu_merge_typed import _back, _dev, _identical, _out, _pk, _stream

pytestmark = pytest.mark.gpu

B, N, C = oracle.BILINEAR, oracle.NEAREST, oracle.BICUBIC
NZ5 = ("inside-extended", B, B, 5, True)
# every geometry and method row with "w"; one bilinear row with each of the other packings ("wrap" on an inside-* geometry)
TYPED_CASES = [(c, "w") for c in tgv.CASES + [NZ5]] + [(("inside-rotated", B, B, 3, True), "same"), (("inside-extended", B, B, 3, True), "ties"),
                                                       (("inside-rotated", B, B, 9, True), "wrap"), (("inside-rotated", B, B, 3, True), "u")]
assert {c[3] for c, _ in TYPED_CASES} == {1, 3, 5, 9}
# The bounds of `conditions` (19 cells of S with one component at its fill value, a fill share of 0.05 to 0.5) were taken on batches
# of three and five slices.  Two rows have one slice AND a nearest-neighbour regrid in steps 3 and 4, which spreads no hole over a
# stencil; they get bounds of their own, (cells, lower fill share), worked out from the fields and not from the results: a third of
# the slices gives a third of the cells, 19 / 3 rounded down, and a nearest-neighbour regrid of the outer passes on at least the
# 1 % of undefined cells that tests/test_gpu_merge_vector.py scatters over every field.  Every other bound holds for them as it stands.
SINGLE_SLICE_NEAREST_BOUNDS = {("inside-extended", N, N, 1, True): (6, 0.01), ("wide", C, N, 1, True): (6, 0.01)}
assert all(c in tgv.CASES and c[2] == N and c[3] == 1 for c in SINGLE_SLICE_NEAREST_BOUNDS)

S, U = oracle.CDM_SHORT, oracle.CDM_USHORT
P = mt.Packing
NC_FILL_FLOAT = 9.9692099683868690e+36
# components and grids of different types: (inner u, inner v, outer u, outer v); all of them take the chain
MIXES = {
    "int-short": (P(oracle.CDM_INT, -2147483648.0, 0.001, 0.0), P(S, -32768.0, 0.01, 0.0), P(S, -32767.0, 0.02, 0.0), P(oracle.CDM_INT, -1.0, 0.002, -3.0)),
    "uchar-uchar": (P(oracle.CDM_UCHAR, 255.0, 0.125, -16.0), P(oracle.CDM_UCHAR, 0.0, 0.125, -16.0), P(oracle.CDM_UCHAR, 0.0, 0.25, -32.0),
                    P(oracle.CDM_UCHAR, 255.0, 0.25, -32.0)),
    "float-double": (P(oracle.CDM_FLOAT, NC_FILL_FLOAT, 1.0, 0.0), P(oracle.CDM_DOUBLE, -999.0, 0.5, 1.0), P(oracle.CDM_DOUBLE, NC_FILL_FLOAT, 2.0, -10.0),
                     P(oracle.CDM_FLOAT, -999.0, 1.0, 0.0)),
    "short-ushort": (P(S, -32768.0, 0.01, 0.0), P(U, 65535.0, 0.01, -100.0), P(U, 0.0, 0.02, -200.0), P(S, -32767.0, 0.02, 0.0)),
}
MIX_CASE = ("inside-rotated", B, B, 3, True)


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    lib = capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    assert hasattr(lib, "fimex_amd_merge_apply_vector_typed_device")
    return capi


@functools.lru_cache(maxsize=None)
def _packed(geometry, nz, key):
    """[(field in its packing, packing)] for inner u, inner v, outer u, outer v"""
    fields = tgv._fields(geometry, nz)
    if key in MIXES:
        packed = [(mt.as_packed(f, p), p) for f, p in zip(fields, MIXES[key])]
    else:
        packed = mvt.packed_fields(fields, key)
    for a, _ in packed:
        a.setflags(write=False)
    return packed


@functools.lru_cache(maxsize=None)
def _want(case, key, tw=5, bw=2):
    geometry, smooth_method, method, nz, use_outer = case
    (Iu, pIu), (Iv, pIv), (Ou, pOu), (Ov, pOv) = _packed(geometry, nz, key)
    m = mvt.merge_vector_typed(Iu, pIu, Iv, pIv, Ou, pOu, Ov, pOv, tgv._positions(geometry), tgv._shapes(geometry), tgv._matrices(geometry), method,
                               smooth_method, tw, bw, use_outer)
    for a in (m.outU, m.outV):
        a.setflags(write=False)
    return m


def _is_fill(a, p):
    return np.isnan(mt.unpack(a, p))


def conditions(case, key):
    """what a row is meant to hold, from the restatement alone (the bounds: DESIGN.md 6.17) -> the figures, asserted"""
    geometry, _, _, nz, _ = case
    m = _want(case, key)
    (_, pIu), (_, pIv), (_, pOu), (_, pOv) = _packed(geometry, nz, key)
    figures = {"branches": [sorted(np.unique(b).tolist()) for b in (m.branchU, m.branchV)],
               "one_fill_in_S": int(np.count_nonzero(_is_fill(m.Su, pIu) ^ _is_fill(m.Sv, pIv))),
               "fill_share": [float(_is_fill(m.outU, pIu).mean()), float(_is_fill(m.outV, pIv).mean())],
               "out_of_range_step1": mvt.out_of_range(m.OI_float[0], pOu) + mvt.out_of_range(m.OI_float[1], pOv),
               "out_of_range_step3": sum(mvt.out_of_range(r, p) for r, p in zip(m.ST_float + m.OT_float, (pIu, pIv, pOu, pOv)))}
    print("conditions %s %s: %s" % (key, case, figures))
    every = [mt.INNER_KEPT, mt.BLENDED, mt.OUTER_TAKEN, mt.UNDEFINED]
    assert figures["branches"] == [every, every], "a branch of the smoothing does not occur in both components"
    min_one_fill, min_share = SINGLE_SLICE_NEAREST_BOUNDS.get(case, (19, 0.05))
    assert figures["one_fill_in_S"] >= min_one_fill
    assert all(min_share <= s <= 0.5 for s in figures["fill_share"])
    if key == "u":
        assert figures["out_of_range_step1"] >= 1000 and figures["out_of_range_step3"] >= 1000
    if key == "wrap":
        assert figures["out_of_range_step1"] + figures["out_of_range_step3"] >= 1
    if key == "ties":  # stencil fractions are multiples of 1/8 on integer counts rotated by nothing or a quarter turn: exact .5 ties
        ties = sum(int(np.count_nonzero(np.abs(r - np.trunc(r)) == 0.5)) for r in m.OI_float + m.ST_float + m.OT_float)
        print("exact .5 ties in front of interpolationArray2Data:", ties)
        assert ties >= 1
    return figures


def _run_both(fa, case, key, lead_elems=0, tw=5, bw=2):
    """-> (path, (outU, outV) of the entry, (outU, outV) of the chain) with the inputs checked unchanged"""
    geometry, smooth_method, method, nz, use_outer = case
    packed = _packed(geometry, nz, key)
    m = _want(case, key, tw, bw)
    leads = [lead_elems * a.dtype.itemsize for a, _ in packed]
    plans = tgv.Plans(fa, geometry, smooth_method, method, tw, bw, use_outer)
    devs = [_dev(a, lead) for (a, _), lead in zip(packed, leads)]
    fields = [x for (_, ptr), (_, p) in zip(devs, packed) for x in (ptr, _pk(fa, p))]
    (tFu, dFu), (tFv, dFv) = _out(m.outU.nbytes, leads[0], 0xA5), _out(m.outV.nbytes, leads[1], 0xA5)
    (tCu, dCu), (tCv, dCv) = _out(m.outU.nbytes, leads[0], 0x5A), _out(m.outV.nbytes, leads[1], 0x5A)
    path = plans.merge.apply_vector_typed_device(*plans.rotations, *fields, nz, dFu, dFv, _stream())
    plans.merge.apply_vector_typed_chain_device(*plans.rotations, *fields, nz, dCu, dCv, _stream())
    entry = _back(tFu, m.outU, leads[0]), _back(tFv, m.outV, leads[1])
    chain = _back(tCu, m.outU, leads[0]), _back(tCv, m.outV, leads[1])
    for (t, _), (a, _), lead, name in zip(devs, packed, leads, ("inner u", "inner v", "outer u", "outer v")):
        _identical(_back(t, a, lead), a, name + " unchanged")
    plans.close()
    return path, entry, chain


def _compare(label, path, entry, chain, m):
    for name, e, c, want in (("u", entry[0], chain[0], m.outU), ("v", entry[1], chain[1], m.outV)):
        _identical(e, want, "%s %s %s" % (label, name, "fused" if path == 1 else "entry"))
        _identical(c, want, "%s %s chain" % (label, name))
        _identical(e, c, "%s %s entry against chain" % (label, name))


@pytest.mark.parametrize("case,key", TYPED_CASES, ids=lambda v: v if isinstance(v, str) else "%s-m%d-m%d-nz%d-outer%d" % v)
def test_merge_apply_vector_typed(fa, case, key):
    conditions(case, key)
    m = _want(case, key)
    for out, (_, p) in zip((m.outU, m.outV), _packed(case[0], case[3], key)[:2]):
        fills = _is_fill(out, p)
        assert fills.any() and (~fills).mean() > 0.5
    path, entry, chain = _run_both(fa, case, key)
    assert path == 1, path
    _compare("merge vector typed %s %s step1 %d steps34 %d nz %d useOuter %d" % ((key,) + case), path, entry, chain, m)


@pytest.mark.parametrize("key", sorted(MIXES))
def test_other_types_take_the_chain(fa, key):
    path, entry, chain = _run_both(fa, MIX_CASE, key)
    assert path == 0, path
    m = _want(MIX_CASE, key)
    assert (m.outU.dtype, m.outV.dtype) == tuple(mt.dtype_of(p) for p in MIXES[key][:2])
    _compare("merge vector typed " + key, path, entry, chain, m)


def test_smoothing_widths_reach_the_fused_kernels(fa):
    """another (tw, bw) than the default through the merge plan: the overlapping bands of a 40 x 36 inner with tw 15, bw 6"""
    case = ("inside-extended", B, B, 3, True)
    m = _want(case, "w", 15, 6)
    assert not np.array_equal(m.outU, _want(case, "w").outU)
    path, entry, chain = _run_both(fa, case, "w", tw=15, bw=6)
    assert path == 1
    _compare("merge vector typed tw 15 bw 6", path, entry, chain, m)


def test_buffers_at_odd_elements(fa):
    """all six buffers one element into their allocations: 2-byte but not 4-byte aligned"""
    case = ("inside-rotated", B, B, 3, True)
    path, entry, chain = _run_both(fa, case, "w", lead_elems=1)
    assert path == 1
    _compare("merge vector typed, buffers at odd elements", path, entry, chain, _want(case, "w"))


def test_switched_off_in_the_tuning_build(fa, tuning_build, monkeypatch):
    case = ("inside-rotated", B, B, 3, True)
    path, entry, chain = _run_both(fa, case, "w")
    assert path == 1
    _compare("merge vector typed in the tuning build", path, entry, chain, _want(case, "w"))
    monkeypatch.setenv("FIMEX_AMD_MERGE_VECTOR_TYPED_FUSED", "0")
    path, entry, chain = _run_both(fa, case, "w")
    assert path == 0
    _compare("merge vector typed with the fused kernels switched off", path, entry, chain, _want(case, "w"))


def test_host_form(fa):
    case = ("inside-rotated", B, B, 3, True)
    for key in ("w", "float-double"):
        m = _want(case, key)
        plans = tgv.Plans(fa, case[0], B, B)
        fields = [x for a, p in _packed(case[0], case[3], key) for x in (a, _pk(fa, p))]
        gotU, gotV = plans.merge.apply_vector_typed_host(*plans.rotations, *fields)
        _identical(gotU, m.outU, "merge vector typed host %s u" % key)
        _identical(gotV, m.outV, "merge vector typed host %s v" % key)
        plans.close()


def test_refusals_that_need_a_plan(fa):
    import torch
    geometry = "inside-rotated"
    (iy, ix), (oy, ox), (ty, tx) = tgv._shapes(geometry)
    plans = tgv.Plans(fa, geometry, B, B)
    r_oi, r_st, r_ot = plans.rotations
    packings = [_pk(fa, p) for p in mvt.PACKINGS["w"]]
    # one allocation cut into Iu, Iv, Ou, Ov, outU, outV in this order, so that which buffers overlap is known
    sizes = [iy * ix, iy * ix, oy * ox, oy * ox, ty * tx, ty * tx]
    pool = torch.zeros(sum(sizes), dtype=torch.int16, device="cuda")
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    ptrs = [pool.data_ptr() + 2 * int(o) for o in starts]
    ins, (outU, outV) = ptrs[:4], ptrs[4:]

    def fields(buffers, pk=packings):
        return [x for b, p in zip(buffers, pk) for x in (b, p)]

    for entry in (plans.merge.apply_vector_typed_device, plans.merge.apply_vector_typed_chain_device):
        # a vector plan whose grid is not its regrid plan's output grid, in each of the three places
        for rotations in ((r_st, r_st, r_ot), (r_oi, r_oi, r_ot), (r_oi, r_st, r_oi)):
            with pytest.raises(fa.FimexAmdError, match="differs from the (inner|target) grid"):
                entry(*rotations, *fields(ins), 1, outU, outV, _stream())
        # an output buffer that overlaps any other buffer: an input, the other output
        with pytest.raises(fa.FimexAmdError, match="overlaps the outer field's y component"):
            entry(r_oi, r_st, r_ot, *fields(ins), 1, outU, ins[3], _stream())
        with pytest.raises(fa.FimexAmdError, match="overlaps the inner field's x component"):
            entry(r_oi, r_st, r_ot, *fields(ins), 1, ins[0], outV, _stream())
        with pytest.raises(fa.FimexAmdError, match="overlaps the other output"):
            entry(r_oi, r_st, r_ot, *fields(ins), 1, outU, outU + 2, _stream())
        # sizes are counted in each buffer's own element size: outV directly behind a short outU is apart, behind an int outU it is not
        wide = [fa.Packing(fa.CDM_INT, -2147483648.0, 0.001, 0.0)] + packings[1:]
        with pytest.raises(fa.FimexAmdError, match="overlaps the other output"):
            entry(r_oi, r_st, r_ot, *fields(ins, wide), 1, outU, outV, _stream())
        # an inner fill value that its type cannot hold
        with pytest.raises(fa.FimexAmdError, match="not representable"):
            entry(r_oi, r_st, r_ot, *fields(ins, [packings[0], fa.Packing(fa.CDM_SHORT, -40000.0, 0.01, 0.0)] + packings[2:]), 1, outU, outV, _stream())
        # a NULL buffer with nz > 0; nz == 0 is a successful no-op
        for hole in range(6):
            p = [0 if k == hole else a for k, a in enumerate(ins + [outU, outV])]
            with pytest.raises(fa.FimexAmdError, match="NULL data buffer"):
                entry(r_oi, r_st, r_ot, *fields(p[:4]), 1, *p[4:], _stream())
        entry(r_oi, r_st, r_ot, *fields([0] * 4), 0, 0, 0, _stream())
    assert float(pool.abs().max()) == 0.0  # nothing was written by any of them
    if fa.device_count() >= 2:  # plans on another device than the calling thread's
        fa.set_device(1)
        try:
            with pytest.raises(fa.FimexAmdError, match="lives on device"):
                plans.merge.apply_vector_typed_device(r_oi, r_st, r_ot, *fields(ins), 1, outU, outV, 0)
            elsewhere = fa.VectorPlan(tgv._matrices(geometry)[1], tx, ty)  # a vector plan on another device than the merge plan
        finally:
            fa.set_device(0)
        with pytest.raises(fa.FimexAmdError, match="different devices"):
            plans.merge.apply_vector_typed_device(r_oi, elsewhere, r_ot, *fields(ins), 1, outU, outV, _stream())
        elsewhere.close()
    plans.close()
