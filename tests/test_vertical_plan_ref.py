"""tests/vertical_plan_ref.py against tests/vertical_ref.py: a plan followed by its apply is getLevelDataSlice.  The fold of the seven
blends into one factor and one apply rule is what the GPU kernels implement (include/fimex_amd.h, 8f n5b); here it is pinned to the
restatement that tests/test_vertical_ref.py pins to the reference's own answers.  NaN positions must be identical and every defined
cell bit-identical, for the log methods too: both sides take the C library's log.  CPU only."""
import numpy as np
import pytest

import oracle
import test_gpu_vertical as tgv
import vertical_plan_ref as vpr
import vertical_ref as vr

SMALL = tgv.CONFIGS[:6]  # the 53 x 37 cases


def _identical(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "NaN positions differ in %d cells" % np.count_nonzero(gn != wn)
    assert np.array_equal(got[~gn].view(np.uint32), want[~wn].view(np.uint32)), "%d defined cells differ" % np.count_nonzero(
        got[~gn].view(np.uint32) != want[~wn].view(np.uint32))


def _case(seed, kind_in, kind_out, config, safe):
    nx, ny, nt, nzi, nzo, order = config
    data, inL, outL, level1 = tgv.make_case(seed, kind_in, kind_out, nx, ny, nt, nzi, nzo, order, safe)
    ilev = vr.level_field(inL, nt, ny, nx)
    x = vr.level_field(outL, nt, ny, nx).astype(np.float64) if outL is not None else np.asarray(level1, np.float64)[None, :, None, None]
    return data, ilev, x


@pytest.mark.parametrize("config", range(len(SMALL)))
@pytest.mark.parametrize("method", vr.LINEAR_FAMILY)
def test_linear_family_equals_the_restatement(method, config):
    kind_in = vr.KINDS[(method + config) % 5]
    kind_out = vr.KINDS[(method + 2 * config + 1) % 5] if config % 2 else None
    data, ilev, x = _case(300 + 10 * method + config, kind_in, kind_out, SMALL[config], False)
    rng = np.random.default_rng(config)
    ny, nx = data.shape[2:]
    vmin = rng.uniform(5., 300., (ny, nx)) if config in (1, 3) else None
    vmax = rng.uniform(400., 1200., (ny, nx)) if config in (3, 4) else None
    for cmin, cmax in ((np.nan, np.nan), (279., 281.)):
        want = vr.interpolate(method, data, ilev, x, validMin=vmin, validMax=vmax, clampMin=cmin, clampMax=cmax)
        got = vpr.apply(vpr.build(method, ilev, x, vmin, vmax), data, clampMin=cmin, clampMax=cmax)
        _identical(got, want)
    if SMALL[config][3] >= 2:
        assert np.count_nonzero(~np.isnan(want)) > 0


def test_linear_family_on_special_targets():
    """Targets on a level, beyond both ends, +-inf, NaN, 1e30 and DBL_MAX, levels that repeat (a == b is impossible for a pair,
    but equal neighbours are not) and NaN levels."""
    nx, ny, nt, nzi, nzo = 53, 37, 2, 7, 12
    data, inL, _, level1 = tgv.make_case(60, vr.FIELD, None, nx, ny, nt, nzi, nzo, "rep", False)
    level1[-8:] = [1e30, -1e30, 3e19, np.inf, -np.inf, np.nan, np.finfo(np.float64).max, float(inL.field[0, 2, 0, 0])]
    ilev = inL.field.copy()
    ilev[np.random.default_rng(1).uniform(size=ilev.shape) < 0.05] = np.nan
    x = level1[None, :, None, None]
    for method in vr.LINEAR_FAMILY:
        _identical(vpr.apply(vpr.build(method, ilev, x), data), vr.interpolate(method, data, ilev, x))


@pytest.mark.parametrize("config", [0, 2, 4, 5])
@pytest.mark.parametrize("method", [vr.LOG, vr.LOGLOG])
def test_log_methods_equal_the_blend_cell_by_cell(method, config):
    kind_in = vr.KINDS[(method + config) % 5]
    kind_out = vr.KINDS[(config + 3) % 5] if config == 2 else None
    data, ilev, x = _case(400 + 10 * method + config, kind_in, kind_out, SMALL[config], True)
    want = vr.interpolate(method, data, ilev, x)  # cell by cell through the C blend
    _identical(vpr.apply(vpr.build(method, ilev, x), data), want)


@pytest.mark.parametrize("method", [vr.LOG, vr.LOGLOG])
def test_non_positive_levels_are_undefined_under_the_log_methods(method):
    nx, ny = 11, 5
    ilev = np.broadcast_to(np.array([-50., 0., 100., 200., 400.], np.float32)[None, :, None, None], (1, 5, ny, nx)).copy()
    data = tgv.cases.field(5, ny, nx, seed=9, nan_frac=0.0, extremes=False).reshape(1, 5, ny, nx)
    x = np.array([-60., -20., 0., 50., 150., 300., 500.])[None, :, None, None]
    entries = vpr.build(method, ilev, x)
    assert np.all(entries[3][0, :4]) and not np.any(entries[3][0, 4:6])
    _identical(vpr.apply(entries, data), vr.interpolate(method, data, ilev, x))


@pytest.mark.parametrize("dtype,fill", [(np.int8, -128), (np.uint8, 255), (np.int16, -32768), (np.uint16, 65535), (np.int32, -2 ** 31),
                                        (np.uint32, 2 ** 31), (np.int64, -999), (np.uint64, 999), (np.float32, 9.96921e36),
                                        (np.float64, -1e300)], ids=lambda v: getattr(v, "__name__", None))
def test_typed_apply_is_the_float_apply_between_the_two_conversions(dtype, fill):
    """apply on a stored type == interpolationArray2Data(apply on data2InterpolationArray(data)), with the oracle's conversions."""
    nx, ny, nt, nzi, nzo = 53, 37, 2, 7, 5
    rng = np.random.default_rng(5)
    ilev = np.broadcast_to(np.arange(1., nzi + 1, dtype=np.float32)[None, :, None, None], (nt, nzi, ny, nx)).copy()
    x = np.array([1.5, 2.0, 3.25, 6.5, 9.0])[None, :, None, None]
    raw = rng.integers(20, 61, (nt, nzi, ny, nx)).astype(np.float64)
    if np.dtype(dtype).kind == "f":
        raw += rng.integers(0, 4, raw.shape) * 0.25
        raw[0, 0, 0, :4] = -0.0
    data = raw.astype(dtype)
    data[rng.uniform(size=data.shape) < 0.05] = np.array(fill, np.float64).astype(dtype)
    entries = vpr.build(vr.LIN, ilev, x)
    got = vpr.apply(entries, data, dtype, fill, 15., 70.)
    mid = vpr.apply(entries, oracle.data2interpolation_array(data, fill), np.float32, np.nan, 15., 70.)
    want = oracle.interpolation_array2data(mid, oracle.cdm_type_of(np.dtype(dtype)), fill)
    assert got.dtype == np.dtype(dtype) and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert np.count_nonzero(got == np.array(fill, np.float64).astype(dtype)) > 0
    if np.dtype(dtype).kind in "iu":
        assert np.count_nonzero(np.abs(mid[~np.isnan(mid)] % 1.0) == 0.5) > 100  # results on .5: the rounding rule matters
