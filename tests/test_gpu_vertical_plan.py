"""Vertical interpolation plans on the GPU (include/fimex_amd.h, 8f n5b): a plan followed by its apply against the one-shot entry
fimex_amd_vertical_interpolate_device (bit for bit, NaN positions identical), against tests/vertical_plan_ref.py and
tests/vertical_ref.py, the CPU restatements, and on stored types against the chain of the three device calls it replaces.

The linear family is compared bit for bit everywhere.  The log methods take log() on the device, which is not the host's: against
the CPU restatement their results carry the bound of tests/test_gpu_vertical.py (_compare: 2^-22 |f (B - A)| + 2^-23 |want|) and
their factors its factor term, 2^-22 |f|; against the one-shot entry they too are bit-identical, since both run the same device code.

The shapes are the smallest at which the kernels can go wrong: a plane of 53 x 37 = 1961 cells is odd, so every level row of a
1- or 2-byte variable starts at another offset from a 16-byte boundary, and 1961 cells are more than one workgroup of float groups.
"""
import numpy as np
import pytest

import cases
import test_gpu_vertical as tgv
import vertical_plan_ref as vpr
import vertical_ref as vr

pytestmark = pytest.mark.gpu

SMALL = tgv.CONFIGS[:6]  # (53, 37) with (nt, nzi, nzo) of (1, 7, 3), (3, 65, 20), (1, 2, 1), (3, 7, 20), (1, 65, 3), (1, 1, 3)
NAN = float("nan")
FILLS = [(np.int8, -128), (np.uint8, 255), (np.int16, -32768), (np.uint16, 65535), (np.int32, -2 ** 31), (np.uint32, 2 ** 31),
         (np.int64, -999), (np.uint64, 999), (np.float32, 9.96921e36), (np.float64, -1e300)]


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    lib = capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    assert hasattr(lib, "fimex_amd_vertical_plan_apply_device")
    return capi


# ------------------------------------------------------------------ helpers
def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _up(a):
    """A host array of any stored type as device bytes."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()


def _down(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def _levels_x(inL, outL, level1, shape):
    nt, _, ny, nx = shape
    ilev = vr.level_field(inL, nt, ny, nx)
    x = vr.level_field(outL, nt, ny, nx).astype(np.float64) if outL is not None else np.asarray(level1, np.float64)[None, :, None, None]
    return ilev, x


def _device_plan(fa, method, data_shape, inL, outL, level1, vmin=None, vmax=None, stream=None):
    """A plan built from device arrays on `stream`; returns (plan, what must stay alive)."""
    nt, _, ny, nx = data_shape
    li = tgv._fa_levels(fa, inL, device=True)
    lo = tgv._fa_levels(fa, outL, device=True) if outL is not None else None
    d_min = _up(np.asarray(vmin, np.float64)) if vmin is not None else None
    d_max = _up(np.asarray(vmax, np.float64)) if vmax is not None else None
    plan = fa.VerticalPlan(method, nx, ny, nt, li, lo, level1, validMin=d_min.data_ptr() if d_min is not None else None,
                           validMax=d_max.data_ptr() if d_max is not None else None, device=True, stream=_stream() if stream is None else stream)
    return plan, (li, lo, d_min, d_max)


def _float_apply(fa, plan, data, clampMin=NAN, clampMax=NAN):
    import torch
    d_in = torch.from_numpy(data).cuda()
    d_out = torch.full(plan.out_shape, -2.0, dtype=torch.float32, device="cuda")
    plan.apply_device(d_in.data_ptr(), fa.CDM_FLOAT, d_out.data_ptr(), clampMin=clampMin, clampMax=clampMax, stream=_stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _one_shot(fa, method, data, inL, outL, level1, vmin=None, vmax=None, clampMin=NAN, clampMax=NAN):
    import torch
    nt, _, ny, nx = data.shape
    nzo = outL.nz if outL is not None else len(level1)
    li = tgv._fa_levels(fa, inL, device=True)
    lo = tgv._fa_levels(fa, outL, device=True) if outL is not None else None
    d_min = _up(np.asarray(vmin, np.float64)) if vmin is not None else None
    d_max = _up(np.asarray(vmax, np.float64)) if vmax is not None else None
    d_in = torch.from_numpy(data).cuda()
    d_out = torch.full((nt, nzo, ny, nx), -1.0, dtype=torch.float32, device="cuda")
    fa.vertical_interpolate_device(method, nx, ny, nt, d_in.data_ptr(), li, d_out.data_ptr(), outLevels=lo, level1=level1,
                                   d_validMin=d_min.data_ptr() if d_min is not None else None,
                                   d_validMax=d_max.data_ptr() if d_max is not None else None, clampMin=clampMin, clampMax=clampMax, stream=_stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _check_entries(method, plan, ilev, x, vmin=None, vmax=None):
    rFirst, rSecond, rFactor, rUndefined = vpr.build(method, ilev, x, vmin, vmax)
    first, second, factor = plan.entries()
    assert np.all(first[rUndefined] == second[rUndefined]), "an entry the restatement calls undefined is defined"
    d = ~rUndefined
    assert np.array_equal(first[d], rFirst[d]) and np.array_equal(second[d], rSecond[d]), "%d pairs differ" % np.count_nonzero(
        (first[d] != rFirst[d]) | (second[d] != rSecond[d]))
    got, want = factor[d], rFactor[d]
    if method in vr.LINEAR_FAMILY:
        assert np.all(tgv._same_cells(got, want)), "%d factors differ" % np.count_nonzero(~tgv._same_cells(got, want))
        return
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    tol = 2.0 ** -22 * np.abs(want[fin].astype(np.float64))
    print("factors of method %d: %d finite, max error / tolerance %.3f" % (method, err.size, float(np.max(err / np.maximum(tol, 1e-300))) if err.size else 0.0))
    assert np.all(err <= tol), "%d factors over 2^-22 |f|" % np.count_nonzero(err > tol)


# ------------------------------------------------------------------ plan + apply versus the one-shot entry, and the entries
@pytest.mark.parametrize("template", [False, True], ids=["fixed", "template"])
@pytest.mark.parametrize("kind_in", vr.KINDS)
@pytest.mark.parametrize("method", vr.METHODS)
def test_plan_and_apply_equal_the_one_shot_entry(fa, method, kind_in, template):
    i = method * 10 + kind_in * 2 + int(template)
    nx, ny, nt, nzi, nzo, order = SMALL[i % len(SMALL)]
    kind_out = vr.KINDS[(kind_in + 1 + method) % 5] if template else None
    data, inL, outL, level1 = tgv.make_case(1000 + i, kind_in, kind_out, nx, ny, nt, nzi, nzo, order, method in (vr.LOG, vr.LOGLOG))
    plan, keep = _device_plan(fa, method, data.shape, inL, outL, level1)
    assert (plan.info.nx, plan.info.ny, plan.info.nt, plan.info.nzi, plan.info.nzo, plan.info.method) == (nx, ny, nt, nzi, nzo, method)
    assert plan.info.entryBytes == 8 * nt * nzo * ny * nx
    got = _float_apply(fa, plan, data)
    one = _one_shot(fa, method, data, inL, outL, level1)
    assert cases.same(got, one), cases.describe_mismatch(got, one)
    want, A, B, f = tgv._want(method, data, inL, outL, level1)
    share = np.count_nonzero(~np.isnan(want)) / want.size
    print("defined share of the reference result: %.3f" % share)
    if nzi >= 2:
        assert share >= 0.25
    else:
        assert share == 0.0  # one input level: no second distinct level, all NaN by the reference's rule
    tgv._compare(method, got, want, A, B, f, "plan, kind %d %s" % (kind_in, "template %d" % kind_out if template else "fixed"))
    _check_entries(method, plan, *_levels_x(inL, outL, level1, data.shape))


# ------------------------------------------------------------------ stored types
def _stored_case(dtype, fill, shape, seed=5):
    """Values 20 .. 60 (quarters for the floating types, and -0.0), the fill value in 5 % of the cells."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(20, 61, shape).astype(np.float64)
    if np.dtype(dtype).kind == "f":
        raw += rng.integers(0, 4, raw.shape) * 0.25
        raw[0, :, 0, :4] = -0.0
    data = raw.astype(dtype)
    data[rng.uniform(size=data.shape) < 0.05] = np.array(fill, np.float64).astype(dtype)
    return data


@pytest.mark.parametrize("dtype,fill", FILLS, ids=[np.dtype(d).name for d, _ in FILLS])
def test_stored_types_equal_the_three_call_chain(fa, dtype, fill):
    """Levels 1 .. 7 with targets on a level, halfway (results on .5 for odd differences), at a quarter and beyond the last level,
    where the linear method extrapolates out of the range of the 1-byte types and the clamp brings it back."""
    import torch
    nx, ny, nt, nzi, nzo = 53, 37, 2, 7, 5
    inL = vr.Levels(vr.AXIS, nzi, axis=np.arange(1., nzi + 1))
    level1 = np.array([1.5, 2.0, 3.25, 6.5, 9.0])
    data = _stored_case(dtype, fill, (nt, nzi, ny, nx))
    code = fa.cdm_type_of(dtype)
    plan, keep = _device_plan(fa, vr.LIN, data.shape, inL, None, level1)
    d_in = _up(data)
    nOut = nt * nzo * ny * nx
    d_out = torch.zeros(nOut * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")
    plan.apply_device(d_in.data_ptr(), code, d_out.data_ptr(), badValue=fill, clampMin=15., clampMax=70., stream=_stream())
    # the chain on the device
    f_in = torch.empty(data.size, dtype=torch.float32, device="cuda")
    f_out = torch.empty(nOut, dtype=torch.float32, device="cuda")
    c_out = torch.zeros_like(d_out)
    fa.data2interpolation_device(d_in.data_ptr(), code, data.size, fill, f_in.data_ptr(), _stream())
    fa.vertical_interpolate_device(vr.LIN, nx, ny, nt, f_in.data_ptr(), keep[0], f_out.data_ptr(), level1=level1, clampMin=15., clampMax=70., stream=_stream())
    fa.interpolation2data_device(f_out.data_ptr(), nOut, code, fill, c_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    got, chain = _down(d_out, dtype, plan.out_shape), _down(c_out, dtype, plan.out_shape)
    assert np.array_equal(got.view(np.uint8), chain.view(np.uint8)), "%d elements differ from the chain" % np.count_nonzero(got != chain)
    ilev, x = _levels_x(inL, None, level1, data.shape)
    want = vpr.apply(vpr.build(vr.LIN, ilev, x), data, dtype, fill, 15., 70.)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), "%d elements differ from the restatement" % np.count_nonzero(got != want)
    fillT = np.array(fill, np.float64).astype(dtype)
    assert np.count_nonzero(got == fillT) > 100 and np.count_nonzero(got != fillT) > got.size // 2
    mid = f_out.cpu().numpy()
    if np.dtype(dtype).kind in "iu":
        assert np.count_nonzero(np.abs(mid[~np.isnan(mid)] % 1.0) == 0.5) > 100  # results on .5: the rounding rule matters


def test_negative_zero(fa):
    """A float variable with a fill value is stored as interpolationArray2Data stores it: -0.0 becomes +0.0.  With a NaN fill value
    it is an interpolation array and keeps the bits of the one-shot entry."""
    nx, ny, nt, nzi = 8, 4, 1, 3
    inL = vr.Levels(vr.AXIS, nzi, axis=np.arange(1., nzi + 1))
    level1 = np.array([2.0, 2.5])
    data = np.ones((nt, nzi, ny, nx), np.float32)
    data[0, 1, 0] = -0.0
    plan = fa.VerticalPlan(vr.LIN, nx, ny, nt, tgv._fa_levels(fa, inL), None, level1)
    stored, plain = plan.apply_host(data, badValue=9.96921e36), plan.apply_host(data)
    assert np.all(stored[0, 0, 0] == 0) and not np.signbit(stored[0, 0, 0]).any()
    assert np.all(plain[0, 0, 0] == 0) and np.signbit(plain[0, 0, 0]).all()
    assert cases.same(plain, fa.vertical_interpolate_host(vr.LIN, data, tgv._fa_levels(fa, inL), None, level1))
    assert np.array_equal(stored[0, 1], plain[0, 1]) and np.all(stored[0, 1, 0] == 0.5)


# ------------------------------------------------------------------ many variables
@pytest.mark.parametrize("nvar", [1, 3, 9])
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["float", "short"])
def test_many_variables_equal_single_applies(fa, dtype, nvar):
    import torch
    nx, ny, nt, nzi, nzo = 53, 37, 2, 7, 5
    _, inL, _, level1 = tgv.make_case(71, vr.HYBRID_SIGMA_AP, None, nx, ny, nt, nzi, nzo, "dec", False)
    plan, keep = _device_plan(fa, vr.LIN_WEAK_EXTRA, (nt, nzi, ny, nx), inL, None, level1)
    if dtype == np.float32:
        fills = [(9.96921e36, -999.0, NAN)[v % 3] for v in range(nvar)]
    else:
        fills = [(-32768, 32767, -1)[v % 3] for v in range(nvar)]
    cmins = [(NAN, 25.0 + v)[v % 2] for v in range(nvar)]
    cmaxs = [(55.0 - v, NAN, 50.0)[v % 3] for v in range(nvar)]
    datas = [_stored_case(dtype, -999.0 if fills[v] != fills[v] else fills[v], (nt, nzi, ny, nx), seed=20 + v) for v in range(nvar)]
    d_ins = [_up(d) for d in datas]
    size = nt * nzo * ny * nx * np.dtype(dtype).itemsize
    together = [torch.zeros(size, dtype=torch.uint8, device="cuda") for _ in range(nvar)]
    single = [torch.zeros(size, dtype=torch.uint8, device="cuda") for _ in range(nvar)]
    code = fa.cdm_type_of(dtype)
    plan.apply_device([t.data_ptr() for t in d_ins], code, [t.data_ptr() for t in together], badValue=fills, clampMin=cmins, clampMax=cmaxs,
                      stream=_stream())
    for v in range(nvar):
        plan.apply_device(d_ins[v].data_ptr(), code, single[v].data_ptr(), badValue=fills[v], clampMin=cmins[v], clampMax=cmaxs[v], stream=_stream())
    torch.cuda.synchronize()
    ilev, x = _levels_x(inL, None, level1, (nt, nzi, ny, nx))
    entries = vpr.build(vr.LIN_WEAK_EXTRA, ilev, x)
    assert entries[3].any() and not entries[3].all()  # defined and undefined entries
    for v in range(nvar):
        a, b = together[v].cpu().numpy(), single[v].cpu().numpy()
        assert np.array_equal(a, b), "variable %d of %d differs from its single apply" % (v, nvar)
        want = vpr.apply(entries, datas[v], dtype, fills[v], cmins[v], cmaxs[v])
        got = a.view(dtype).reshape(want.shape)
        if dtype == np.float32:
            assert cases.same(got, want), "variable %d: %s" % (v, cases.describe_mismatch(got, want))
        else:
            assert np.array_equal(got, want), "variable %d differs from the restatement" % v


# ------------------------------------------------------------------ edges of the streaming loop
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one element off"])
@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.float32], ids=["int8", "int16", "float"])
@pytest.mark.parametrize("plane", [1, 3, 63, 64, 65, 257])
def test_edges_of_the_streaming_loop(fa, plane, dtype, offset):
    """Planes below, at and just over one 16-byte group and one wavefront of groups; input and output one element off a 16-byte
    boundary (a level field that differs from column to column: neighbouring cells take their values from different planes)."""
    import torch
    nt, nzi, nzo = 2, 7, 5
    fdata, inL, _, level1 = tgv.make_case(80 + plane, vr.FIELD, None, plane, 1, nt, nzi, nzo, "inc", False)
    if dtype == np.float32:
        data, fill = fdata, NAN
    else:
        fill = -128
        with np.errstate(invalid="ignore", over="ignore"):
            data = np.clip(np.nan_to_num(np.round((fdata - 280.0) * 3), nan=fill, posinf=100, neginf=-100), -100, 100).astype(dtype)
        data[np.isnan(fdata)] = fill
    plan, keep = _device_plan(fa, vr.LIN, data.shape, inL, None, level1)
    elem = np.dtype(dtype).itemsize
    off = offset * elem
    buf_in = torch.zeros(data.size * elem + 32, dtype=torch.uint8, device="cuda")
    buf_out = torch.full((nt * nzo * plane * elem + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf_in.data_ptr() % 16 == 0 and buf_out.data_ptr() % 16 == 0
    buf_in[off:off + data.size * elem] = _up(data)
    cmin, cmax = (NAN, NAN) if dtype == np.float32 else (-100., 100.)  # the linear method extrapolates out of the range of int8
    plan.apply_device(buf_in.data_ptr() + off, fa.cdm_type_of(dtype), buf_out.data_ptr() + off, badValue=fill, clampMin=cmin, clampMax=cmax,
                      stream=_stream())
    torch.cuda.synchronize()
    raw = buf_out.cpu().numpy()
    n = nt * nzo * plane * elem
    assert np.all(raw[:off] == 0xA5) and np.all(raw[off + n:] == 0xA5), "the apply wrote outside its output"
    got = raw[off:off + n].copy().view(dtype).reshape(plan.out_shape)
    ilev, x = _levels_x(inL, None, level1, data.shape)
    want = vpr.apply(vpr.build(vr.LIN, ilev, x), data, dtype, fill, cmin, cmax)
    if dtype == np.float32:
        assert cases.same(got, want), cases.describe_mismatch(got, want)
    else:
        assert np.array_equal(got, want), "%d of %d elements differ" % (np.count_nonzero(got != want), got.size)


# ------------------------------------------------------------------ carried-over behaviour
@pytest.mark.parametrize("bounds", ["min", "max", "both"])
def test_validity_ranges(fa, bounds):
    """Through the *_host forms."""
    nx, ny, nt, nzi, nzo = 53, 37, 2, 7, 20
    data, inL, _, level1 = tgv.make_case(21, vr.SIGMA, None, nx, ny, nt, nzi, nzo, "inc", False)
    rng = np.random.default_rng(4)
    vmin = rng.uniform(5., 300., (ny, nx)) if bounds in ("min", "both") else None
    vmax = rng.uniform(400., 1200., (ny, nx)) if bounds in ("max", "both") else None
    if vmin is not None:
        vmin[0, :nzo] = level1  # x == validMin is inside (>=)
    if vmax is not None:
        vmax[1, :nzo] = level1  # x == validMax is inside (<=)
    plan = fa.VerticalPlan(vr.LIN, nx, ny, nt, tgv._fa_levels(fa, inL), None, level1, validMin=vmin, validMax=vmax)
    got = plan.apply_host(data)
    want = tgv._want(vr.LIN, data, inL, None, level1, validMin=vmin, validMax=vmax)[0]
    plain = tgv._want(vr.LIN, data, inL, None, level1)[0]
    assert np.count_nonzero(np.isnan(want) & ~np.isnan(plain)) > 100  # the ranges do cut
    assert cases.same(got, want), cases.describe_mismatch(got, want)
    one = fa.vertical_interpolate_host(vr.LIN, data, tgv._fa_levels(fa, inL), None, level1, validMin=vmin, validMax=vmax)
    assert cases.same(got, one), cases.describe_mismatch(got, one)
    _check_entries(vr.LIN, plan, *_levels_x(inL, None, level1, data.shape), vmin, vmax)


def test_clamping_with_nan_data(fa):
    nx, ny, nt, nzi, nzo = 53, 37, 1, 7, 3
    data, inL, _, level1 = tgv.make_case(33, vr.HYBRID_SIGMA, None, nx, ny, nt, nzi, nzo, "shuf", False)
    assert np.isnan(data).any()
    plan, keep = _device_plan(fa, vr.LIN, data.shape, inL, None, level1)
    for cmin, cmax in ((279., 281.), (NAN, 281.), (279., NAN), (NAN, NAN)):
        got = _float_apply(fa, plan, data, cmin, cmax)
        want = tgv._want(vr.LIN, data, inL, None, level1, clampMin=cmin, clampMax=cmax)[0]
        assert np.isnan(want).any() and cases.same(got, want), cases.describe_mismatch(got, want)
        one = _one_shot(fa, vr.LIN, data, inL, None, level1, clampMin=cmin, clampMax=cmax)
        assert cases.same(got, one), cases.describe_mismatch(got, one)


@pytest.mark.parametrize("where", ["first", "all", "scattered"])
@pytest.mark.parametrize("method", [vr.LIN, vr.LIN_NO_EXTRA, vr.LOG])
def test_nan_inside_the_level_field(fa, method, where):
    """Columns that must be walked."""
    nx, ny, nt, nzi, nzo = 53, 37, 1, 7, 20
    data, inL, _, level1 = tgv.make_case(44, vr.FIELD, None, nx, ny, nt, nzi, nzo, "shuf", method == vr.LOG)
    f = inL.field.copy()
    rng = np.random.default_rng(8)
    cols = rng.uniform(size=(ny, nx)) < 0.5
    if where == "first":
        f[:, 0][:, cols] = np.nan
    elif where == "all":
        f[:, :, cols] = np.nan
    else:
        f[rng.uniform(size=f.shape) < 0.15] = np.nan
    inL = vr.Levels(vr.FIELD, nzi, field=f)
    plan, keep = _device_plan(fa, method, data.shape, inL, None, level1)
    got = _float_apply(fa, plan, data)
    one = _one_shot(fa, method, data, inL, None, level1)
    assert cases.same(got, one), cases.describe_mismatch(got, one)
    tgv._compare(method, got, *tgv._want(method, data, inL, None, level1), label="plan, NaN levels (%s)" % where)
    _check_entries(method, plan, *_levels_x(inL, None, level1, data.shape))


@pytest.mark.parametrize("method", [vr.LOG, vr.LOGLOG])
def test_non_positive_levels_are_undefined_under_the_log_methods(fa, method):
    nx, ny, nt = 11, 5, 1
    inL = vr.Levels(vr.AXIS, 5, axis=np.array([-50., 0., 100., 200., 400.]))
    data = cases.field(5, ny, nx, seed=9, nan_frac=0.0, extremes=False).reshape(1, 5, ny, nx)
    level1 = np.array([-60., -20., 0., 50., 150., 300., 500.])
    plan = fa.VerticalPlan(method, nx, ny, nt, tgv._fa_levels(fa, inL), None, level1)
    got = plan.apply_host(data)
    first, second, _ = plan.entries()
    assert np.all(first[0, :4] == second[0, :4]) and np.all(first[0, 4:6] != second[0, 4:6])
    assert np.all(np.isnan(got[0, :4])) and np.all(np.isfinite(got[0, 4:6]))
    tgv._compare(method, got, *tgv._want(method, data, inL, None, level1), label="plan, non-positive levels")
    _check_entries(method, plan, *_levels_x(inL, None, level1, data.shape))


@pytest.mark.parametrize("order", ["inc", "dec", "rep"])
@pytest.mark.parametrize("kind_in", [vr.FIELD, vr.AXIS, vr.HYBRID_SIGMA])
def test_bisection_and_walk_give_the_same_entries(fa, tuning_build, monkeypatch, kind_in, order):
    """The plan of the tuning build with every column walked, and with groups of 8 output levels, holds the entries of the default
    build's.  The targets include values so large that x - level rounds to the same double for neighbouring levels, +-inf, NaN and
    DBL_MAX."""
    nx, ny, nt, nzi, nzo = 53, 37, 2, 7, 11
    data, inL, _, level1 = tgv.make_case(60, kind_in, None, nx, ny, nt, nzi, nzo, order, False)
    level1[-7:] = [1e30, -1e30, 3e19, np.inf, -np.inf, np.nan, np.finfo(np.float64).max]
    fa.use_tuning_build(False)
    try:
        default = fa.VerticalPlan(vr.LIN, nx, ny, nt, tgv._fa_levels(fa, inL), None, level1).entries()
    finally:
        fa.use_tuning_build(True)
    ilev, x = _levels_x(inL, None, level1, data.shape)
    for bisect, group in ((0, 4), (1, 8), (0, 8), (1, 4)):
        monkeypatch.setenv("FIMEX_AMD_VERTICAL_BISECT", str(bisect))
        monkeypatch.setenv("FIMEX_AMD_VERTICAL_GROUP", str(group))
        plan = fa.VerticalPlan(vr.LIN, nx, ny, nt, tgv._fa_levels(fa, inL), None, level1)
        first, second, factor = plan.entries()
        assert np.array_equal(first, default[0]) and np.array_equal(second, default[1]), (bisect, group)
        assert np.all(tgv._same_cells(factor, default[2])), (bisect, group)
        _check_entries(vr.LIN, plan, ilev, x)


@pytest.mark.parametrize("group", [4, 8])
@pytest.mark.parametrize("nzo", [1, 3, 4, 5, 9])
def test_short_last_groups_of_the_build(fa, tuning_build, monkeypatch, nzo, group):
    """Output level counts below, at and above the group sizes: a short last group of 4 and of 8 (tuning build) stores its own entries
    only."""
    monkeypatch.setenv("FIMEX_AMD_VERTICAL_GROUP", str(group))
    data, inL, _, level1 = tgv.make_case(70 + nzo, vr.FIELD, None, 31, 9, 2, 7, nzo, "inc", False)
    plan = fa.VerticalPlan(vr.LIN, 31, 9, 2, tgv._fa_levels(fa, inL), None, level1)
    _check_entries(vr.LIN, plan, *_levels_x(inL, None, level1, data.shape))
    tgv._compare(vr.LIN, _float_apply(fa, plan, data), *tgv._want(vr.LIN, data, inL, None, level1))


@pytest.mark.parametrize("method", vr.LINEAR_FAMILY)
def test_bisecting_and_walking_columns_in_one_wave(fa, method):
    data, inL, level1 = tgv.mixed_columns(80, 53, 37, 2, 7, 11)
    plan, keep = _device_plan(fa, method, data.shape, inL, None, level1)
    _check_entries(method, plan, *_levels_x(inL, None, level1, data.shape))
    tgv._compare(method, _float_apply(fa, plan, data), *tgv._want(method, data, inL, None, level1))


@pytest.mark.parametrize("plane", [tgv.BLOCK - 1, tgv.BLOCK, tgv.BLOCK + 1])
def test_build_on_planes_around_a_workgroup(fa, plane):
    data, inL, _, level1 = tgv.make_case(90 + plane, vr.HYBRID_SIGMA, None, plane, 1, 2, 7, 5, "dec", False)
    plan, keep = _device_plan(fa, vr.LIN_WEAK_EXTRA, data.shape, inL, None, level1)
    _check_entries(vr.LIN_WEAK_EXTRA, plan, *_levels_x(inL, None, level1, data.shape))
    tgv._compare(vr.LIN_WEAK_EXTRA, _float_apply(fa, plan, data), *tgv._want(vr.LIN_WEAK_EXTRA, data, inL, None, level1))


# ------------------------------------------------------------------ streams
def test_a_side_stream_equals_the_host_forms(fa):
    import torch
    nx, ny, nt, nzi, nzo = 53, 37, 3, 7, 20
    data, inL, outL, _ = tgv.make_case(55, vr.HYBRID_SIGMA_AP, vr.FIELD, nx, ny, nt, nzi, nzo, "dec", False)
    rng = np.random.default_rng(6)
    vmin, vmax = rng.uniform(5., 100., (ny, nx)), rng.uniform(800., 1600., (ny, nx))
    hostPlan = fa.VerticalPlan(vr.LIN_WEAK_EXTRA, nx, ny, nt, tgv._fa_levels(fa, inL), tgv._fa_levels(fa, outL), None, validMin=vmin, validMax=vmax)
    host = hostPlan.apply_host(data, clampMin=270., clampMax=300.)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_in = torch.from_numpy(data).cuda()
        d_out = torch.full((nt, nzo, ny, nx), -1.0, dtype=torch.float32, device="cuda")
        plan, keep = _device_plan(fa, vr.LIN_WEAK_EXTRA, data.shape, inL, outL, None, vmin, vmax, stream=side.cuda_stream)
        plan.apply_device(d_in.data_ptr(), fa.CDM_FLOAT, d_out.data_ptr(), clampMin=270., clampMax=300., stream=side.cuda_stream)  # at once
    side.synchronize()
    got = d_out.cpu().numpy()
    assert cases.same(got, host), cases.describe_mismatch(got, host)
    want = tgv._want(vr.LIN_WEAK_EXTRA, data, inL, outL, None, validMin=vmin, validMax=vmax, clampMin=270., clampMax=300.)[0]
    assert cases.same(got, want), cases.describe_mismatch(got, want)
    for a, b in zip(plan.entries(), hostPlan.entries()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_one_plan_applied_from_two_streams(fa):
    import torch
    nx, ny, nt, nzi, nzo = 53, 37, 3, 7, 20
    _, inL, _, level1 = tgv.make_case(56, vr.SIGMA, None, nx, ny, nt, nzi, nzo, "inc", False)
    data = _stored_case(np.int16, -32768, (nt, nzi, ny, nx))
    plan, keep = _device_plan(fa, vr.LIN, data.shape, inL, None, level1)
    torch.cuda.synchronize()  # the two streams below are ordered behind the build
    d_in = _up(data)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.zeros(nt * nzo * ny * nx * 2, dtype=torch.uint8, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for _ in range(3):
        for s, o in zip(streams, outs):
            plan.apply_device(d_in.data_ptr(), fa.CDM_SHORT, o.data_ptr(), badValue=-32768, stream=s.cuda_stream)
    for s in streams:
        s.synchronize()
    a, b = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    assert np.array_equal(a, b)
    ilev, x = _levels_x(inL, None, level1, data.shape)
    want = vpr.apply(vpr.build(vr.LIN, ilev, x), data, np.int16, -32768)
    assert np.array_equal(a.view(np.int16).reshape(want.shape), want)


# ------------------------------------------------------------------ refusals that need a plan
def test_bad_applies_are_refused(fa):
    import torch
    nx, ny, nt, nzi, nzo = 8, 4, 1, 3, 2
    plan = fa.VerticalPlan(vr.LIN, nx, ny, nt, fa.VerticalLevels.from_axis([1., 2., 3.]), None, [1.5, 2.5])
    d = torch.zeros(nt * (nzi + nzo) * ny * nx * 2 + 8, dtype=torch.float32, device="cuda")
    p_in, p_out = d.data_ptr(), d.data_ptr() + 4 * nt * nzi * ny * nx
    plan.apply_device(p_in, fa.CDM_FLOAT, p_out, stream=_stream())  # side by side is fine
    with pytest.raises(fa.FimexAmdError, match="overlaps the input of variable 0"):
        plan.apply_device(p_in, fa.CDM_FLOAT, p_out - 4, stream=_stream())
    with pytest.raises(fa.FimexAmdError, match="overlaps another output"):
        plan.apply_device([p_in, p_in], fa.CDM_FLOAT, [p_out, p_out + 4 * nx], stream=_stream())
    with pytest.raises(fa.FimexAmdError, match="not aligned to its element size of 4 bytes"):
        plan.apply_device(p_in, fa.CDM_FLOAT, p_out + 2, stream=_stream())
    with pytest.raises(fa.FimexAmdError, match="nvar == 0"):
        plan.apply_device([], fa.CDM_FLOAT, [], stream=_stream())
    with pytest.raises(fa.FimexAmdError):
        plan.apply_device(p_in, 6, p_out, stream=_stream())  # CDM_STRING
    with pytest.raises(fa.FimexAmdError, match="NULL data buffer of variable 0"):
        plan.apply_device(p_in, fa.CDM_FLOAT, 0, stream=_stream())
    torch.cuda.synchronize()
    plan.close()
    plan.close()
