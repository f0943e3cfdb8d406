"""tests/merge_typed_ref.py, the CPU restatement of grid merging on stored types, against the reference's own known answers
(test/testMerger.cc:58-60, :92-94, on its own fixtures in the types the files store and within its own bounds) and, where a
variable is a float with a NaN fill value, scale 1 and offset 0, against tests/merge_ref.py, the restatement on float arrays."""
import functools

import numpy as np
import pytest

import merge_ref as mr
import merge_typed_ref as mt
import oracle

STORED = {"test_merger": (mt.dr.CDM_DOUBLE, None), "test_merge_target": (mt.dr.CDM_FLOAT, 9.96921e36)}


@functools.lru_cache(maxsize=None)
def _merged(golden_dir, name):
    c = mr.load_case(golden_dir, name)
    pos = mr.merge_positions(c["inner"], c["outer"], c["target"])
    I, pi, O, po = mt.load_case_stored(golden_dir, name)
    return pi, po, mt.merge_typed(I, pi, O, po, pos, mr.case_shapes(c))


@pytest.mark.parametrize("name", sorted(mr.KNOWN))
def test_known_answers_of_the_reference_in_the_stored_types(golden_dir, name):
    shape, known, bound = mr.KNOWN[name]
    pi, po, m = _merged(golden_dir, name)
    cdm_type, fill = STORED[name]
    assert pi.type == po.type == cdm_type and m.out.dtype == mt.dtype_of(pi) and m.out.shape == (1,) + shape
    if fill is not None:
        assert np.float32(pi.fill) == np.float32(fill) and np.float32(po.fill) == np.float32(fill)
    values = mt.unpack(m.out, pi)
    for ix, iy, expected in known:
        got = float(values[0, iy, ix])
        print("%s (%d, %d): %.6f, expected %s" % (name, ix, iy, got, expected))
        assert abs(got - expected) < bound  # the reference's own bound


# ---- float, NaN fill, scale 1, offset 0: the typed chain is the float chain
B, N, C = oracle.BILINEAR, oracle.NEAREST, oracle.BICUBIC


@pytest.mark.parametrize("case", [("inside-extended", B, B, 3, True), ("inside-rotated", B, C, 2, False), ("rowout-rotated", N, N, 1, True)],
                         ids=lambda c: "%s-m%d-m%d-nz%d-outer%d" % c)
def test_float_with_nan_fill_is_the_float_merge(case):
    geometry, smooth_method, method, nz, use_outer = case
    inner, outer, target = mt.GEOMETRIES[geometry]
    I, O = mt.float_fields(geometry, nz)
    shapes = (inner.shape, outer.shape, target.shape)
    p = mt.Packing(mt.dr.CDM_FLOAT, mt.NAN, 1.0, 0.0)
    m = mt.merge_typed(I, p, O, p, mt.positions(geometry), shapes, method, smooth_method, 5, 2, use_outer)
    want, S = mr.merge(I, O, mt.positions(geometry), shapes, method, smooth_method, 5, 2, use_outer)
    for got, ref, label in ((m.S, S, "S"), (m.out, want, "out")):
        assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape
        gn, rn = np.isnan(got), np.isnan(ref)
        assert np.array_equal(gn, rn), label + ": NaN positions differ"
        assert np.array_equal(got[~gn], ref[~rn]), label + ": values differ"  # ==: interpolationArray2Data turns -0 into +0
    assert np.isnan(want).any() and np.isfinite(want).mean() > 0.5
