"""Grid merging on stored types on the GPU (include/fimex_amd.h): typed border smoothing, typed overlay, the fused
typed merge and its chain against tests/merge_typed_ref.py, the CPU restatement that tests/test_merge_typed_ref.py pins to the
reference's known answers.

The bar is byte for byte.  No tolerance is needed: every operation is a correctly rounded IEEE add, multiply, divide or square
root in the restatement's order, there are no transcendentals, and the regrids are the ones already bit-exact.  Every element is
compared; the share of identical elements is printed before the assertion.
"""
import functools

import numpy as np
import pytest

import merge_ref as mr
import merge_typed_ref as mt
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    lib = capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    assert hasattr(lib, "fimex_amd_merge_apply_typed_device")
    return capi


def _dev(a, lead=0):
    """a copy of a's bytes on the device, `lead` bytes into an allocation -> (tensor that owns it, pointer)"""
    import torch
    raw = np.concatenate([np.zeros(lead, np.uint8), np.ascontiguousarray(a).view(np.uint8).ravel()])
    t = torch.from_numpy(raw).cuda()
    return t, t.data_ptr() + lead


def _out(nbytes, lead=0, value=0xA5):
    import torch
    t = torch.full((nbytes + lead,), value, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr() + lead


def _back(t, like, lead=0):
    return t.cpu().numpy()[lead:lead + like.nbytes].view(like.dtype).reshape(like.shape)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _pk(fa, p):
    return fa.Packing(p.type, p.fill, p.scale, p.offset)


def _identical(got, want, label):
    """every element the same bytes; prints the share of identical elements first"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    size = want.dtype.itemsize
    same = (got.view(np.uint8).reshape(-1, size) == want.view(np.uint8).reshape(-1, size)).all(axis=1)
    print("%s: %d elements, %.4f %% identical" % (label, want.size, 100.0 * np.count_nonzero(same) / max(want.size, 1)))
    if not np.all(same):
        i = int(np.argwhere(~same)[0, 0])
        raise AssertionError("%s: %d elements differ; first at %d: got %r want %r" % (label, np.count_nonzero(~same), i, got.flat[i], want.flat[i]))


# ------------------------------------------------------------------------------------------------- the elementwise entries
SHAPES = [(1, 1), (3, 9), (4, 4), (15, 17), (150, 11)]
WIDTHS = [(5, 2), (1, 0), (3, 4), (9, 20)]
ELEMENTWISE_KEYS = ("a", "c", "u") + mt.CHAINED


@functools.lru_cache(maxsize=None)
def _raw(key, nx, ny, nz):
    I, pi, O, po = mt.raw_fields(key, 1000 * nx + 10 * ny + nz, (nz, ny, nx))
    I.setflags(write=False)
    O.setflags(write=False)
    return I, pi, O, po


@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "tw%d-bw%d" % w)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_border_smooth_typed(fa, shape, widths):
    (nx, ny), (tw, bw) = shape, widths
    for key in ELEMENTWISE_KEYS:
        for nz in (1, 3, 5):
            I, pi, O, po = _raw(key, nx, ny, nz)
            one_size = I.dtype.itemsize == O.dtype.itemsize
            for use_outer in (True, False):
                want, _ = mt.smooth_typed(I, pi, O, po, tw, bw, use_outer)
                label = "border_smooth_typed %s %dx%dx%d tw %d bw %d useOuter %d" % (key, nx, ny, nz, tw, bw, use_outer)
                (tI, dI), (tO, dO), (tS, dS) = _dev(I), _dev(O), _out(want.nbytes)
                args = (nx, ny, nz, tw, bw, use_outer, _stream())
                fa.border_smooth_typed_device(dI, _pk(fa, pi), dO, _pk(fa, po), dS, *args)
                _identical(_back(tS, want), want, label + " out of place")
                _identical(_back(tI, I), I, label + " inner unchanged")
                _identical(_back(tO, O), O, label + " outer unchanged")
                fa.border_smooth_typed_device(dI, _pk(fa, pi), dO, _pk(fa, po), dI, *args)
                _identical(_back(tI, want), want, label + " in place on the inner")
                (tI, dI) = _dev(I)
                if one_size:
                    fa.border_smooth_typed_device(dI, _pk(fa, pi), dO, _pk(fa, po), dO, *args)
                    _identical(_back(tO, want), want, label + " in place on the outer")
                else:
                    with pytest.raises(fa.FimexAmdError, match="overlaps"):
                        fa.border_smooth_typed_device(dI, _pk(fa, pi), dO, _pk(fa, po), dO, *args)


@pytest.mark.parametrize("shape", SHAPES + [(2 * 4 * 256 + 37, 1)], ids=lambda s: "%dx%d" % s)
def test_overlay_typed(fa, shape):
    nx, ny = shape
    for key in ELEMENTWISE_KEYS:
        for nz in (1, 3, 5):
            top, pt, base, pb = _raw(key, nx, ny, nz)
            one_size = top.dtype.itemsize == base.dtype.itemsize
            want = mt.overlay_typed(top, pt, base, pb)
            label = "overlay_typed %s %d values" % (key, top.size)
            (tT, dT), (tB, dB), (tS, dS) = _dev(top), _dev(base), _out(want.nbytes)
            fa.overlay_typed_device(dT, _pk(fa, pt), dB, _pk(fa, pb), dS, top.size, _stream())
            _identical(_back(tS, want), want, label + " out of place")
            _identical(_back(tT, top), top, label + " top unchanged")
            _identical(_back(tB, base), base, label + " base unchanged")
            fa.overlay_typed_device(dT, _pk(fa, pt), dB, _pk(fa, pb), dT, top.size, _stream())
            _identical(_back(tT, want), want, label + " in place on the top")
            (tT, dT) = _dev(top)
            if one_size:
                fa.overlay_typed_device(dT, _pk(fa, pt), dB, _pk(fa, pb), dB, top.size, _stream())
                _identical(_back(tB, want), want, label + " in place on the base")
            else:
                with pytest.raises(fa.FimexAmdError, match="overlaps"):
                    fa.overlay_typed_device(dT, _pk(fa, pt), dB, _pk(fa, pb), dB, top.size, _stream())
            if nz == 3 and shape == (15, 17):
                _identical(fa.overlay_typed_host(top, _pk(fa, pt), base, _pk(fa, pb)), want, label + " host")
                w, _ = mt.smooth_typed(top, pt, base, pb, 5, 2, True)
                _identical(fa.border_smooth_typed_host(top, _pk(fa, pt), base, _pk(fa, pb), 5, 2, True), w, label + " smoothing, host")


def test_elementwise_refusals(fa):
    I, pi, O, po = _raw("a", 15, 17, 3)
    (tI, dI), (tO, dO), (tS, dS) = _dev(I), _dev(O), _out(I.nbytes)
    with pytest.raises(fa.FimexAmdError, match="overlaps"):  # partly overlapping output
        fa.border_smooth_typed_device(dI, _pk(fa, pi), dO, _pk(fa, po), dI + 2, 15, 17, 3, 5, 2, True, _stream())
    with pytest.raises(fa.FimexAmdError, match="overlaps"):
        fa.overlay_typed_device(dI, _pk(fa, pi), dO, _pk(fa, po), dO + 2, I.size - 1, _stream())
    with pytest.raises(fa.FimexAmdError, match="not representable"):
        fa.overlay_typed_device(dI, fa.Packing(pi.type, 40000.0, 1.0, 0.0), dO, _pk(fa, po), dS, I.size, _stream())
    _identical(_back(tS, I), np.full_like(I, np.int16(0xA5A5 - 65536)), "nothing written by a refused call")


# --------------------------------------------------------------------------------------------------------------- the merge
B, N, C = oracle.BILINEAR, oracle.NEAREST, oracle.BICUBIC
# tests/test_gpu_merge.py's MERGE_CASES: (geometry, method of step 1, method of steps 3 and 4, nz, useOuter)
MERGE_CASES = [
    ("inside-extended", B, B, 3, True),
    ("inside-extended", N, N, 1, True),
    ("inside-extended", C, C, 3, False),
    ("inside-rotated", B, C, 9, True),
    ("inside-rotated", B, B, 1, False),
    ("rowout-rotated", B, B, 9, False),
    ("rowout-rotated", C, C, 1, True),
    ("rowout-rotated", N, N, 3, False),
]
TYPED_CASES = [(c, "a") for c in MERGE_CASES] + [(("inside-rotated", B, B, 1, False), "b"), (("inside-extended", B, B, 3, True), "c"),
                                                 (("rowout-rotated", B, B, 9, False), "d"), (("inside-rotated", B, B, 3, True), "u")] + [
    (("inside-rotated", B, B, 3, True), k) for k in mt.CHAINED]

@functools.lru_cache(maxsize=None)
def _fields(geometry, nz, key):
    I, O = mt.float_fields(geometry, nz)
    if (geometry, nz) == ("inside-extended", 1):
        # the one-slice nearest-neighbour row: the copied holes of inner and outer do not meet there, so one more hole in the outer,
        # under the inner's interior hole, gives the row its undefined cells
        O[0, 11:13, 13] = np.nan
    rI, pi, rO, po = mt.packed_fields(I, O, key)
    rI.setflags(write=False)
    rO.setflags(write=False)
    return rI, pi, rO, po


def _shapes(geometry):
    inner, outer, target = mt.GEOMETRIES[geometry]
    return inner.shape, outer.shape, target.shape


@functools.lru_cache(maxsize=None)
def _want(case, key, tw=5, bw=2):
    geometry, smooth_method, method, nz, use_outer = case
    rI, pi, rO, po = _fields(geometry, nz, key)
    m = mt.merge_typed(rI, pi, rO, po, mt.positions(geometry), _shapes(geometry), method, smooth_method, tw, bw, use_outer)
    m.out.setflags(write=False)
    return m


def _plans(fa, geometry, smooth_method, method, tw=5, bw=2, use_outer=True):
    inner, outer, target = mt.GEOMETRIES[geometry]
    (oix, oiy), (itx, ity), (otx, oty) = mt.positions(geometry)
    oi = fa.RegridPlan(smooth_method, oix, oiy, outer.nx, outer.ny, inner.nx, inner.ny)
    it = fa.RegridPlan(method, itx, ity, inner.nx, inner.ny, target.nx, target.ny)
    ot = fa.RegridPlan(method, otx, oty, outer.nx, outer.ny, target.nx, target.ny)
    return fa.MergePlan(oi, it, ot, tw, bw, use_outer), (oi, it, ot)


def _is_fill(a, p):
    fill = mt.pack(np.array([np.nan]), p)[0]
    return np.isnan(a) if a.dtype.kind == "f" and np.isnan(fill) else a == fill


def _run_both(fa, case, key, lead_elems=0):
    """-> (path, the entry's result, the chain's result) with the inputs checked unchanged"""
    geometry, smooth_method, method, nz, use_outer = case
    rI, pi, rO, po = _fields(geometry, nz, key)
    want = _want(case, key).out
    lead = lead_elems * rI.dtype.itemsize, lead_elems * rO.dtype.itemsize
    plan, keep = _plans(fa, geometry, smooth_method, method, 5, 2, use_outer)
    (tI, dI), (tO, dO) = _dev(rI, lead[0]), _dev(rO, lead[1])
    (tF, dF), (tC, dC) = _out(want.nbytes, lead[0], 0xA5), _out(want.nbytes, lead[0], 0x5A)
    path = plan.apply_typed_device(dI, _pk(fa, pi), dO, _pk(fa, po), nz, dF, _stream())
    plan.apply_typed_chain_device(dI, _pk(fa, pi), dO, _pk(fa, po), nz, dC, _stream())
    fused, chain = _back(tF, want, lead[0]), _back(tC, want, lead[0])
    _identical(_back(tI, rI, lead[0]), rI, "inner unchanged")
    _identical(_back(tO, rO, lead[1]), rO, "outer unchanged")
    plan.close()
    return path, fused, chain


@pytest.mark.parametrize("case,key", TYPED_CASES, ids=lambda v: v if isinstance(v, str) else "%s-m%d-m%d-nz%d-outer%d" % v)
def test_merge_apply_typed(fa, case, key):
    geometry, smooth_method, method, nz, use_outer = case
    rI, pi, rO, po = _fields(geometry, nz, key)
    m = _want(case, key)
    # the case holds what it is meant to hold
    branches = set(np.unique(m.branch).tolist())
    assert branches == {mt.INNER_KEPT, mt.BLENDED, mt.OUTER_TAKEN, mt.UNDEFINED}, branches
    fills = _is_fill(m.out, pi)
    assert fills.any() and (~fills).mean() > 0.5
    if key == "c" and geometry == "inside-extended":  # stencil fractions are multiples of 1/8 on integer counts: exact .5 ties
        ties = sum(int(np.count_nonzero(np.abs(r - np.trunc(r)) == 0.5)) for r in (m.OI_float, m.OT_float))
        print("exact .5 ties in front of interpolationArray2Data:", ties)
        assert ties >= 1
    if key in ("d", "u"):  # blended and outer values leave the range of the inner's type: the casts wrap
        blended, _ = mt.smooth_double(mt.unpack(rI, pi), mt.unpack(m.OI, po), 5, 2, use_outer)
        counts = (blended - pi.offset) / pi.scale
        info = np.iinfo(mt.dtype_of(pi))
        counts = counts[~np.isnan(counts)]
        wrapped = np.count_nonzero((counts > info.max + 0.5) | (counts < info.min - 0.5))
        print("values of S beyond the range of the type:", wrapped)
        assert wrapped >= 1
    label = "merge typed %s %s step1 %d steps34 %d nz %d useOuter %d" % ((key,) + case)
    path, fused, chain = _run_both(fa, case, key)
    assert path == (1 if key in mt.FUSED else 0), path
    _identical(fused, m.out, label + (" fused" if path == 1 else " entry"))
    _identical(chain, m.out, label + " chain")
    _identical(fused, chain, label + " entry against chain")


def test_merge_apply_typed_unaligned(fa):
    """d_out, d_inner and d_outer one element into their allocations: 2-byte but not 4-byte aligned"""
    case = ("inside-rotated", B, B, 3, True)
    path, fused, chain = _run_both(fa, case, "a", lead_elems=1)
    assert path == 1
    _identical(fused, _want(case, "a").out, "merge typed, buffers at odd elements, fused")
    _identical(chain, _want(case, "a").out, "merge typed, buffers at odd elements, chain")


def test_merge_apply_typed_switched_off(fa, tuning_build, monkeypatch):
    case = ("inside-rotated", B, B, 3, True)
    path, fused, _ = _run_both(fa, case, "a")
    assert path == 1
    _identical(fused, _want(case, "a").out, "merge typed in the tuning build")
    monkeypatch.setenv("FIMEX_AMD_MERGE_TYPED_FUSED", "0")
    path, entry, _ = _run_both(fa, case, "a")
    assert path == 0
    _identical(entry, _want(case, "a").out, "merge typed with the fused kernels switched off")


def test_merge_apply_typed_host(fa):
    case = ("inside-rotated", B, B, 3, True)
    for key in ("a", "e-float-double"):
        rI, pi, rO, po = _fields(case[0], case[3], key)
        plan, keep = _plans(fa, case[0], B, B)
        _identical(plan.apply_typed_host(rI, _pk(fa, pi), rO, _pk(fa, po)), _want(case, key).out, "merge typed host " + key)
        plan.close()


def test_merge_smoothing_widths_reach_the_typed_kernels(fa):
    case = ("inside-extended", B, B, 3, True)
    rI, pi, rO, po = _fields(case[0], case[3], "a")
    want = _want(case, "a", 15, 6).out
    plan, keep = _plans(fa, case[0], B, B, 15, 6, True)
    (tI, dI), (tO, dO), (tF, dF) = _dev(rI), _dev(rO), _out(want.nbytes)
    assert plan.apply_typed_device(dI, _pk(fa, pi), dO, _pk(fa, po), case[3], dF, _stream()) == 1
    _identical(_back(tF, want), want, "merge typed tw 15 bw 6")
    plan.close()


# --------------------------------------------------------------------------------------- the reference's fixtures, end to end
@pytest.mark.parametrize("name", sorted(mr.KNOWN))
def test_reference_fixtures_in_their_stored_types(fa, golden_dir, name):
    """test/testMerger.cc on the variables as the files store them (double; float with the netCDF default fill value): equal to the
    restatement fed with the same positions, the known answers within the reference's bounds"""
    shape, known, bound = mr.KNOWN[name]
    c = mr.load_case(golden_dir, name)
    pos = mr.merge_positions(c["inner"], c["outer"], c["target"], project_axes=fa.project_axes_host, points2position=fa.points2position_host,
                             types=(fa.PROJ_AXIS, fa.LONGITUDE, fa.LATITUDE))
    (iy, ix), (oy, ox), (ty, tx) = mr.case_shapes(c)
    I, pi, O, po = mt.load_case_stored(golden_dir, name)
    oi = fa.RegridPlan(fa.BILINEAR, pos[0][0], pos[0][1], ox, oy, ix, iy)
    it = fa.RegridPlan(fa.BILINEAR, pos[1][0], pos[1][1], ix, iy, tx, ty)
    ot = fa.RegridPlan(fa.BILINEAR, pos[2][0], pos[2][1], ox, oy, tx, ty)
    plan = fa.MergePlan(oi, it, ot)
    got = plan.apply_typed_host(I, _pk(fa, pi), O, _pk(fa, po))
    assert got.shape == (1,) + shape and got.dtype == I.dtype
    values = mt.unpack(got, pi)
    for kx, ky, expected in known:
        print("%s (%d, %d): %.6f, expected %s" % (name, kx, ky, float(values[0, ky, kx]), expected))
        assert abs(float(values[0, ky, kx]) - expected) < bound
    _identical(got, mt.merge_typed(I, pi, O, po, pos, mr.case_shapes(c)).out, name + " whole field")
    plan.close()


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_that_need_a_plan(fa):
    case = ("inside-rotated", B, B, 1, False)
    rI, pi, rO, po = _fields(case[0], case[3], "a")
    want = _want(case, "a").out
    plan, keep = _plans(fa, case[0], B, B)
    (tI, dI), (tO, dO), (tF, dF) = _dev(rI), _dev(rO), _out(want.nbytes)
    for apply in (plan.apply_typed_device, plan.apply_typed_chain_device):
        with pytest.raises(fa.FimexAmdError, match="overlaps the inner"):
            apply(dI, _pk(fa, pi), dO, _pk(fa, po), 1, dI, _stream())
        with pytest.raises(fa.FimexAmdError, match="overlaps the outer"):
            apply(dI, _pk(fa, pi), dO, _pk(fa, po), 1, dO + 2, _stream())
        with pytest.raises(fa.FimexAmdError, match="not representable"):
            apply(dI, fa.Packing(pi.type, -40000.0, pi.scale, pi.offset), dO, _pk(fa, po), 1, dF, _stream())
    with pytest.raises(fa.FimexAmdError, match="not representable"):
        plan.apply_typed_host(rI, fa.Packing(pi.type, float("nan"), pi.scale, pi.offset), rO, _pk(fa, po))
    # nz == 0 is a successful no-op, as for the float applies
    assert plan.apply_typed_device(0, _pk(fa, pi), 0, _pk(fa, po), 0, 0, _stream()) == 0
    plan.apply_typed_chain_device(0, _pk(fa, pi), 0, _pk(fa, po), 0, 0, _stream())
    if fa.device_count() >= 2:  # a plan on another device than the calling thread's
        fa.set_device(1)
        try:
            with pytest.raises(fa.FimexAmdError, match="lives on device"):
                plan.apply_typed_device(dI, _pk(fa, pi), dO, _pk(fa, po), 1, dF, 0)
        finally:
            fa.set_device(0)
    plan.close()
