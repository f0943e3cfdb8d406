"""The merge's per-cell arithmetic the HIP kernels compile (fimex_amd/csrc/merge_math.hpp: the cell classes and the blend of
CDMBorderSmoothing_Linear, ScaleValue, and the cells of the smoothing and the overlay on stored types) run here on the CPU:
tests/merge_math_host.cc uses the header the way merge_typed.hip does and fimex_amd/build.py compiles it with g++, without any
HIP header.  Every result must equal the restatement of tests/merge_typed_ref.py (and, for the float form, tests/merge_ref.py)
byte for byte.  No GPU is involved."""
import ctypes

import numpy as np
import pytest

import merge_ref as mr
import merge_typed_ref as mt
import oracle
from fimex_amd import build as fb

NX, NY, NZ = 15, 17, 2
WIDTHS = [(5, 2), (1, 0), (3, 4), (9, 20)]


class PackingArg(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int), ("fill", ctypes.c_double), ("scale", ctypes.c_double), ("offset", ctypes.c_double)]


def _arg(p):
    return ctypes.byref(PackingArg(p.type, p.fill, p.scale, p.offset))


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(fb.build_merge_math_host())
    V, Z, P = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(PackingArg)
    lib.merge_math_smooth_float.argtypes = [V, V, V, Z, Z, Z, Z, Z, ctypes.c_int]
    lib.merge_math_smooth_typed.argtypes = [V, P, V, P, V, Z, Z, Z, Z, Z, ctypes.c_int]
    lib.merge_math_overlay_typed.argtypes = [V, P, V, P, V, Z]
    lib.merge_math_regrid_overlay_typed.argtypes = [V, P, V, P, V, Z]
    return lib


def _same_bytes(got, want, label):
    assert got.dtype == want.dtype and got.shape == want.shape, label
    same = got.view(np.uint8) == want.view(np.uint8)
    if not same.all():
        i = np.argwhere(got != want)
        raise AssertionError("%s: %d elements differ; first at %s: got %r want %r" % (
            label, len(i), tuple(i[0]) if len(i) else "?", got[tuple(i[0])] if len(i) else None, want[tuple(i[0])] if len(i) else None))


@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "tw%d-bw%d" % w)
def test_float_form_keeps_the_bits_of_the_float_merge(shim, widths):
    tw, bw = widths
    rng = np.random.default_rng(tw * 100 + bw)
    I = rng.normal(280, 5, (NZ, NY, NX)).astype(np.float32)
    O = rng.normal(280, 5, (NZ, NY, NX)).astype(np.float32)
    I[rng.random(I.shape) < 0.1] = np.nan
    O[rng.random(O.shape) < 0.1] = np.nan
    O[0, 3, 3], I[0, 3, 3] = I[0, 4, 4], I[0, 4, 4]  # diff == 0
    for use_outer in (True, False):
        got = np.empty_like(I)
        assert shim.merge_math_smooth_float(I.ctypes.data, O.ctypes.data, got.ctypes.data, NX, NY, NZ, tw, bw, int(use_outer)) == 0
        want = mr.border_smooth(I, O, tw, bw, use_outer)
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn) and np.array_equal(got[~gn].view(np.uint32), want[~wn].view(np.uint32))


@pytest.mark.parametrize("key", sorted(mt.PACKINGS))
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "tw%d-bw%d" % w)
def test_smooth_cell_typed(shim, widths, key):
    tw, bw = widths
    I, pi, O, po = mt.raw_fields(key, 7 + tw, (NZ, NY, NX))
    for use_outer in (True, False):
        got = np.empty_like(I)
        assert shim.merge_math_smooth_typed(I.ctypes.data, _arg(pi), O.ctypes.data, _arg(po), got.ctypes.data, NX, NY, NZ, tw, bw, int(use_outer)) == 0
        want, branch = mt.smooth_typed(I, pi, O, po, tw, bw, use_outer)
        _same_bytes(got, want, "smooth %s tw %d bw %d useOuter %d" % (key, tw, bw, use_outer))
        if (tw, bw) == (5, 2):
            assert set(np.unique(branch)) >= {mt.INNER_KEPT, mt.BLENDED, mt.OUTER_TAKEN} and (use_outer or (branch == mt.UNDEFINED).any())


@pytest.mark.parametrize("key", sorted(mt.PACKINGS))
def test_overlay_cell_typed(shim, key):
    top, pt, base, pb = mt.raw_fields(key, 11, (NZ, NY, NX))
    got = np.empty_like(top)
    assert shim.merge_math_overlay_typed(top.ctypes.data, _arg(pt), base.ctypes.data, _arg(pb), got.ctypes.data, top.size) == 0
    _same_bytes(got, mt.overlay_typed(top, pt, base, pb), "overlay " + key)


@pytest.mark.parametrize("key", sorted(mt.PACKINGS))
def test_regrid_overlay_cell_typed(shim, key):
    """steps 3 and 4 from float regrid results: exact .5 ties, values beyond the type's range, NaN in either or both"""
    pt, pb, shift = mt.PACKINGS[key]
    assert mt.dr.representable(pt.fill, mt.dtype_of(pt)) and mt.dr.representable(pb.fill, mt.dtype_of(pb))
    rng = np.random.default_rng(13)
    n = 4000
    top = (rng.integers(-70000, 70000, n) / 2.0).astype(np.float32)  # every second one a tie
    base = (rng.integers(-70000, 70000, n) / 2.0).astype(np.float32)
    top[rng.random(n) < 0.3] = np.nan
    base[rng.random(n) < 0.3] = np.nan
    assert np.count_nonzero(np.abs(top - np.trunc(top)) == 0.5) > 100
    got = np.empty(n, mt.dtype_of(pt))
    assert shim.merge_math_regrid_overlay_typed(top.ctypes.data, _arg(pt), base.ctypes.data, _arg(pb), got.ctypes.data, n) == 0
    ST = oracle.interpolation_array2data(top, pt.type, pt.fill)
    OT = oracle.interpolation_array2data(base, pb.type, pb.fill)
    _same_bytes(got, mt.overlay_typed(ST, pt, OT, pb), "regrid + overlay " + key)


def test_unrepresentable_output_fill_is_refused(shim):
    bad = mt.Packing(mt.dr.CDM_SHORT, 1e9, 1.0, 0.0)
    ok = mt.PACKINGS["a"][1]
    x = np.zeros(4, np.int16)
    assert shim.merge_math_overlay_typed(x.ctypes.data, _arg(bad), x.ctypes.data, _arg(ok), x.ctypes.data, 4) == -1
    assert shim.merge_math_overlay_typed(x.ctypes.data, _arg(mt.Packing(0, 0.0, 1.0, 0.0)), x.ctypes.data, _arg(ok), x.ctypes.data, 4) == -1
