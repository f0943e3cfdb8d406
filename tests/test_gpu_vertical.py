"""Vertical interpolation on the GPU (include/fimex_amd.h, 8f n5) against tests/vertical_ref.py, the CPU restatement of
CDMVerticalInterpolator::getLevelDataSlice that tests/test_vertical_ref.py pins to the reference's own known answers.

Nearest and the four linear methods, and the level fields, are compared bit for bit with identical NaN positions.  The log
and loglog methods take log() on the device, which is not the host's: both are accurate to about one unit in the last place
of a double, so with input levels at least 1e-4 relative apart the two values of f are equal or adjacent floats, and per cell
    |got - want| <= 2^-22 * |f * (B - A)| + 2^-23 * |want|,     NaN positions identical,
is asserted.  The cases of those two methods are built so that every target level equals an input level of its column or lies
at least 1e-3 relative away from every one (checked by _assert_safe), which rules out a flip of the f == 0 / f == 1 branches.
The share of bit-identical cells is printed (recorded in DESIGN.md, not asserted).
"""
import concurrent.futures

import numpy as np
import pytest

import cases
import vertical_ref as vr

pytestmark = pytest.mark.gpu

P0 = 1000.0
BLOCK = 256  # columns per workgroup (kBlock, csrc/common.hpp)
PS_CLASSES = np.array([955.0, 985.5, 1003.0, 1041.0], np.float32)


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    lib = capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    assert hasattr(lib, "fimex_amd_vertical_interpolate_device")
    return capi


# ------------------------------------------------------------------ case construction
def _spacing(nz, lo, hi):
    """Relative distance of neighbouring levels of _profile (the jitter is a share of it, so capped for very few levels)."""
    return min((hi / lo) ** (1.0 / (nz - 1)) - 1.0, 0.5) if nz > 1 else 0.05


def _profile(rng, nz, lo, hi, order):
    """nz values between lo and hi, neighbours well over 1e-4 relative apart; order: inc / dec / shuf / rep (shuffled, repeats)."""
    sp = _spacing(nz, lo, hi)
    v = lo * (hi / lo) ** (np.arange(nz) / max(nz - 1, 1)) * (1 + 0.2 * sp * rng.uniform(-1, 1, nz)) if nz > 1 else np.array([np.sqrt(lo * hi)])
    if order == "dec":
        v = v[::-1].copy()
    elif order in ("shuf", "rep"):
        v = rng.permutation(v)
        if order == "rep" and nz > 2:
            v[nz // 2] = v[0]
            v[-1] = v[1]
    return v


def _coefficients(kind, v):
    """Coefficient arrays that give the levels v in a column with ps == P0."""
    v = np.asarray(v, np.float64)
    if kind == vr.AXIS:
        return dict(axis=v)
    if kind == vr.SIGMA:
        return dict(sigma=(v - 5.0) / (P0 - 5.0), ptop=5.0)
    b = 0.9 * (v / P0) ** 2
    ap = v - b * P0
    if kind == vr.HYBRID_SIGMA:
        return dict(a=ap / P0, b=b, p0=P0)
    return dict(ap=ap, b=b)


def _levels(kind, v, ps, rng, nt, ny, nx, lo, hi):
    if kind == vr.FIELD:
        sp = _spacing(len(v), lo, hi)
        f = (v[None, :, None, None] * (1 + 0.2 * rng.uniform(-1, 1, (nt, 1, ny, nx))) *
             (1 + 0.1 * sp * rng.uniform(-1, 1, (nt, len(v), ny, nx)))).astype(np.float32)
        for k in range(len(v)):  # repeated levels of the profile stay exact repeats in every column
            first = int(np.nonzero(v == v[k])[0][0])
            if first != k:
                f[:, k] = f[:, first]
        return vr.Levels(vr.FIELD, len(v), field=f)
    return vr.Levels(kind, len(v), ps=None if kind == vr.AXIS else ps, **_coefficients(kind, v))


def _class_levels(kind, v):
    """float32 levels [nz][classes] of a formula / axis kind in columns of every ps class."""
    lv = vr.Levels(kind, len(v), ps=PS_CLASSES.reshape(1, 1, -1), **_coefficients(kind, v))
    return vr.level_field(lv, 1, 1, len(PS_CLASSES))[0, :, 0, :]


def _clear(x, lev):
    """x (float32-representable) equals, or is at least 1e-3 relative away from, every level."""
    x, lev = np.float64(x), np.asarray(lev, np.float64)
    return bool(np.all((lev == x) | (np.abs(lev - x) >= 1e-3 * np.maximum(np.abs(lev), np.abs(x)))))


def _near(x, lev):
    """x differs from lev by less than 1e-3 relative (in float64)."""
    x, lev = np.asarray(x, np.float64), np.asarray(lev, np.float64)
    return (x != lev) & (np.abs(x - lev) < 1e-3 * np.maximum(np.abs(lev), np.abs(x)))


def _assert_safe(ilev, x):
    """The input condition of the log tolerance, for every column: levels equal or >= 1e-4 relative apart, targets equal to
    a level or >= 1e-3 relative away from every one."""
    il = ilev.astype(np.float64)
    s = np.sort(il, axis=1)
    d = np.diff(s, axis=1)
    assert np.all((d == 0) | (d >= 1e-4 * np.abs(s[:, 1:]))), "input levels closer than 1e-4"
    for k in range(il.shape[1]):
        lk = il[:, k][:, None]
        gap = np.abs(x - lk)
        assert np.all((gap == 0) | (gap >= 1e-3 * np.maximum(np.abs(lk), np.abs(x)))), "a target within 1e-3 of input level %d" % k


def make_case(seed, kind_in, kind_out, nx, ny, nt, nzi, nzo, order, safe):
    """kind_out None: fixed levels.  Returns (data, inLevels, outLevels or None, level1 or None); safe: the log condition holds."""
    rng = np.random.default_rng(seed)
    lo, hi = 10.0, 1000.0
    data = cases.field(nt * nzi, ny, nx, seed=seed + 1, nan_frac=0.05).reshape(nt, nzi, ny, nx)
    formula_in = kind_in != vr.FIELD
    formula_out = kind_out is not None and kind_out != vr.FIELD
    if safe:
        ps = PS_CLASSES[rng.integers(0, len(PS_CLASSES), (nt, ny, nx))]
    else:
        ps = (P0 * (1 + 0.05 * rng.uniform(-1, 1, (nt, ny, nx)))).astype(np.float32)
        ps[0, 0, 0] = PS_CLASSES[0]
    v = _profile(rng, nzi, lo, hi, order)
    inL = _levels(kind_in, v, ps, rng, nt, ny, nx, lo, hi)
    ilev = vr.level_field(inL, nt, ny, nx)
    some = rng.uniform(size=(nt, ny, nx)) < 0.3  # columns where "on a level" targets are made exact when the kinds allow it

    def draw(j):  # one target value: inside the column range, on an input level, below, above
        what = ("inside", "on", "below", "above")[j % 4]
        if what == "inside":
            return float(np.exp(rng.uniform(np.log(lo * 1.3), np.log(hi * 0.7))))
        if what == "below":
            return float(lo * rng.uniform(0.3, 0.7))
        if what == "above":
            return float(hi * rng.uniform(1.4, 1.7))
        return float(ilev[0, rng.integers(0, nzi), 0, 0])  # a level of column (0, 0, 0)

    if kind_out is None:
        inClass = _class_levels(kind_in, v) if formula_in else None
        level1 = np.empty(nzo)
        for j in range(nzo):
            for _ in range(1000):
                level1[j] = float(np.float32(draw(j)))
                if not (safe and formula_in) or _clear(level1[j], inClass):
                    break
            else:
                raise AssertionError("no safe target found")
        x = np.broadcast_to(level1[None, :, None, None], (nt, nzo, ny, nx))
        outL = None
    else:
        level1 = None
        wlo, whi = 5.0, 1500.0
        w = _profile(rng, nzo, wlo, whi, "inc" if order in ("inc", "dec") else "shuf")
        if kind_in == vr.AXIS and kind_out == vr.AXIS and nzo > 1:
            w[1] = v[rng.integers(0, nzi)]  # exactly on an input level in every column
        if safe and formula_in and formula_out:
            inClass = _class_levels(kind_in, v)
            for j in range(nzo):
                base = w[j]
                for _ in range(1000):
                    oc = _class_levels(kind_out, w)[j]
                    if all(_clear(oc[c], inClass[:, c]) for c in range(len(PS_CLASSES))):
                        break
                    w[j] = base * (1 + 0.05 * rng.uniform(-1, 1))
                else:
                    raise AssertionError("no safe template level found")
        outL = _levels(kind_out, w, ps, rng, nt, ny, nx, wlo, whi)
        x = vr.level_field(outL, nt, ny, nx)
        if kind_out == vr.FIELD:  # targets exactly on an input level of their own column
            pick = rng.integers(0, nzi, x.shape)
            x = np.where(some[:, None], np.take_along_axis(ilev, pick, axis=1), x)
            if safe:
                for k in range(nzi):
                    lk = ilev[:, k][:, None]
                    x = np.where(_near(x, lk), lk, x)
            outL = vr.Levels(vr.FIELD, nzo, field=x)
        x = x.astype(np.float64)
    if kind_in == vr.FIELD and (kind_out is None or formula_out):
        # the level field is ours to shape: input levels ON a target in some columns, and (safe) none just beside one
        xs = np.broadcast_to(x, (nt, nzo, ny, nx)).astype(np.float32)
        f = ilev.copy()
        for j in range(nzo):
            xj = xs[:, j][:, None]
            if j % 4 == 1:
                k = int(rng.integers(0, nzi))
                f[:, k] = np.where(some, xs[:, j], f[:, k])
            if safe:
                f = np.where(_near(f, xj), xj, f)
        inL = vr.Levels(vr.FIELD, nzi, field=f)
        ilev = f
    if safe:
        _assert_safe(ilev, np.broadcast_to(x, (nt, nzo, ny, nx)))
    return data, inL, outL, level1


def _fa_levels(fa, lv, device=False):
    """vertical_ref.Levels -> capi.VerticalLevels (device=True: ps / field as torch tensors, returned to keep them alive)."""
    keep = []

    def big(v):
        if v is None or not device:
            return v
        import torch
        t = torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
        keep.append(t)
        return t.data_ptr()
    out = fa.VerticalLevels(lv.kind, lv.nz, axis=lv.axis, sigma=lv.sigma, a=lv.a, ap=lv.ap, b=lv.b, p0=lv.p0, ptop=lv.ptop,
                            ps=big(lv.ps), field=big(lv.field))
    out._tensors = keep
    return out


def _want(method, data, inL, outL, level1, **kw):
    nt, nzi, ny, nx = data.shape
    ilev = vr.level_field(inL, nt, ny, nx)
    x = vr.level_field(outL, nt, ny, nx).astype(np.float64) if outL is not None else np.asarray(level1, np.float64)[None, :, None, None]
    return vr.interpolate(method, data, ilev, x, details=True, **kw)


def _same_cells(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return (na & nb) | (~na & ~nb & (a.view(np.uint32) == b.view(np.uint32)))


_shares = []


def _compare(method, got, want, A, B, f, label=""):
    assert got.shape == want.shape
    if method in vr.LINEAR_FAMILY:
        assert cases.same(got, want), cases.describe_mismatch(got, want)
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "NaN positions differ in %d cells" % np.count_nonzero(gn != wn)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~wn], want[~fin & ~wn])
    g, w = got[fin].astype(np.float64), want[fin].astype(np.float64)
    with np.errstate(all="ignore"):
        tol = 2.0 ** -22 * np.abs(f[fin] * (B[fin].astype(np.float64) - A[fin].astype(np.float64))) + 2.0 ** -23 * np.abs(w)
    err = np.abs(g - w)
    same = np.count_nonzero(got[fin].view(np.uint32) == want[fin].view(np.uint32))
    share = same / max(g.size, 1)
    _shares.append((same, g.size))
    print("vertical %s method %d: %d finite cells, %.4f %% bit-identical, max error / tolerance %.3f"
          % (label, method, g.size, 100 * share, float(np.nanmax(np.where(np.isfinite(tol), err / np.maximum(tol, 1e-300), 0.0))) if g.size else 0.0))
    bad = err > tol
    assert not np.any(bad), "%d cells over the tolerance; worst: got %r want %r tol %r" % (
        np.count_nonzero(bad), g[bad][np.argmax((err - tol)[bad])], w[bad][np.argmax((err - tol)[bad])], tol[bad][np.argmax((err - tol)[bad])])


# (nx, ny, nt, nzi, nzo, order): every value of the issue's lists appears; the log methods take the first six (small grids,
# their yardstick goes cell by cell through the oracle) and the one 257 x 131 case with few cells per column
CONFIGS = [(53, 37, 1, 7, 3, "inc"), (53, 37, 3, 65, 20, "dec"), (53, 37, 1, 2, 1, "shuf"), (53, 37, 3, 7, 20, "rep"),
           (53, 37, 1, 65, 3, "shuf"), (53, 37, 1, 1, 3, "inc"), (257, 131, 1, 7, 3, "rep"),
           (257, 131, 3, 65, 20, "inc"), (257, 131, 1, 2, 20, "dec"), (257, 131, 3, 7, 1, "shuf"), (257, 131, 1, 65, 3, "rep"),
           (257, 131, 1, 1, 1, "dec")]


def _config(method, kind_in, template):
    i = method * 10 + kind_in * 2 + int(template)
    return CONFIGS[i % 7] if method in (vr.LOG, vr.LOGLOG) else CONFIGS[i % len(CONFIGS)]


@pytest.mark.parametrize("template", [False, True], ids=["fixed", "template"])
@pytest.mark.parametrize("kind_in", vr.KINDS)
@pytest.mark.parametrize("method", vr.METHODS)
def test_matches_the_cpu_restatement(fa, method, kind_in, template):
    nx, ny, nt, nzi, nzo, order = _config(method, kind_in, template)
    kind_out = vr.KINDS[(kind_in + 1 + method) % 5] if template else None
    safe = method in (vr.LOG, vr.LOGLOG)
    data, inL, outL, level1 = make_case(1000 + method * 10 + kind_in * 2 + int(template), kind_in, kind_out, nx, ny, nt, nzi, nzo, order, safe)
    got = fa.vertical_interpolate_host(method, data, _fa_levels(fa, inL), _fa_levels(fa, outL) if outL is not None else None, level1)
    want, A, B, f = _want(method, data, inL, outL, level1)
    if nzi > 1:
        assert np.count_nonzero(~np.isnan(want)) > 0
    _compare(method, got, want, A, B, f, "kind %d %s" % (kind_in, "template %d" % kind_out if template else "fixed"))


@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("nzo", [1, 3, 20])
@pytest.mark.parametrize("nzi", [1, 2, 7, 65])
def test_level_counts(fa, nzi, nzo, nt):
    """Every combination of the level counts (the group size of the kernel and its short last group), linear and log."""
    for method, kind_in, kind_out, order in ((vr.LIN, vr.HYBRID_SIGMA_AP, None, "shuf"), (vr.LOG, vr.FIELD, vr.SIGMA, "dec")):
        data, inL, outL, level1 = make_case(7 + nzi + nzo + nt, kind_in, kind_out, 31, 9, nt, nzi, nzo, order, method == vr.LOG)
        got = fa.vertical_interpolate_host(method, data, _fa_levels(fa, inL), _fa_levels(fa, outL) if outL is not None else None, level1)
        _compare(method, got, *_want(method, data, inL, outL, level1), label="nzi %d nzo %d nt %d" % (nzi, nzo, nt))


@pytest.mark.parametrize("kind", vr.KINDS)
def test_level_fields_are_bit_identical(fa, kind):
    for nx, ny, nt, nz, order in ((53, 37, 3, 7, "shuf"), (257, 131, 1, 65, "inc"), (5, 3, 2, 1, "inc")):
        _, inL, _, _ = make_case(50 + kind, kind, None, nx, ny, nt, nz, 1, order, False)
        want = vr.level_field(inL, nt, ny, nx)
        got = fa.vertical_levels_host(_fa_levels(fa, inL), nx, ny, nt)
        assert cases.same(got, want), cases.describe_mismatch(got, want)


def test_level_fields_on_the_device(fa):
    import torch
    nx, ny, nt, nz = 53, 37, 2, 7
    _, inL, _, _ = make_case(3, vr.HYBRID_SIGMA, None, nx, ny, nt, nz, 1, "dec", False)
    lv = _fa_levels(fa, inL, device=True)
    out = torch.zeros((nt, nz, ny, nx), dtype=torch.float32, device="cuda")
    fa.vertical_levels_device(lv, nx, ny, nt, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert cases.same(out.cpu().numpy(), vr.level_field(inL, nt, ny, nx))


@pytest.mark.parametrize("method", [vr.LOG, vr.LOGLOG])
def test_non_positive_levels_give_nan_under_the_log_methods(fa, method):
    """Where the reference's blend returns MIFI_ERROR and leaves the element unset, NaN is written."""
    nx, ny, nt = 11, 5, 1
    axis = np.array([-50., 0., 100., 200., 400.])
    data = cases.field(5, ny, nx, seed=9, nan_frac=0.0, extremes=False).reshape(1, 5, ny, nx)
    level1 = np.array([-60., -20., 0., 50., 150., 300., 500.])
    inL = vr.Levels(vr.AXIS, 5, axis=axis)
    got = fa.vertical_interpolate_host(method, data, _fa_levels(fa, inL), None, level1)
    want, A, B, f = _want(method, data, inL, None, level1)
    assert np.all(np.isnan(got[0, :4]))          # a, b or x <= 0
    assert np.all(np.isfinite(got[0, 4:6]))      # between positive levels
    _compare(method, got, want, A, B, f, "non-positive levels")


@pytest.mark.parametrize("bounds", ["min", "max", "both"])
@pytest.mark.parametrize("method", [vr.LIN, vr.LIN_CONST_EXTRA])
def test_validity_ranges(fa, method, bounds):
    nx, ny, nt, nzi, nzo = 53, 37, 2, 7, 20
    data, inL, outL, level1 = make_case(21, vr.SIGMA, None, nx, ny, nt, nzi, nzo, "inc", False)
    rng = np.random.default_rng(4)
    vmin = rng.uniform(5., 300., (ny, nx)) if bounds in ("min", "both") else None
    vmax = rng.uniform(400., 1200., (ny, nx)) if bounds in ("max", "both") else None
    if vmin is not None:
        vmin[0, :nzo] = level1  # x == validMin is inside (>=)
    if vmax is not None:
        vmax[1, :nzo] = level1  # x == validMax is inside (<=)
    got = fa.vertical_interpolate_host(method, data, _fa_levels(fa, inL), None, level1, validMin=vmin, validMax=vmax)
    want = _want(method, data, inL, None, level1, validMin=vmin, validMax=vmax)[0]
    plain = _want(method, data, inL, None, level1)[0]
    assert np.count_nonzero(np.isnan(want) & ~np.isnan(plain)) > 100  # the ranges do cut
    assert cases.same(got, want), cases.describe_mismatch(got, want)


def test_clamping_with_nan_data(fa):
    nx, ny, nt, nzi, nzo = 53, 37, 1, 7, 3
    data, inL, outL, level1 = make_case(33, vr.HYBRID_SIGMA, None, nx, ny, nt, nzi, nzo, "shuf", False)
    assert np.isnan(data).any()
    for cmin, cmax in ((279., 281.), (np.nan, 281.), (279., np.nan), (np.nan, np.nan)):
        got = fa.vertical_interpolate_host(vr.LIN, data, _fa_levels(fa, inL), None, level1, clampMin=cmin, clampMax=cmax)
        want = _want(vr.LIN, data, inL, None, level1, clampMin=cmin, clampMax=cmax)[0]
        assert np.isnan(want).any() and cases.same(got, want), cases.describe_mismatch(got, want)
        fin = np.isfinite(got)
        if not np.isnan(cmin):
            assert got[fin].min() >= cmin
        if not np.isnan(cmax):
            assert got[fin].max() <= cmax


@pytest.mark.parametrize("where", ["first", "middle", "all", "scattered"])
@pytest.mark.parametrize("method", [vr.LIN, vr.NN, vr.LIN_NO_EXTRA, vr.LOG])
def test_nan_inside_the_level_field(fa, method, where):
    nx, ny, nt, nzi, nzo = 53, 37, 1, 7, 20
    data, inL, outL, level1 = make_case(44, vr.FIELD, None, nx, ny, nt, nzi, nzo, "shuf", method == vr.LOG)
    f = inL.field.copy()
    rng = np.random.default_rng(8)
    cols = rng.uniform(size=(ny, nx)) < 0.5
    if where == "first":
        f[:, 0][:, cols] = np.nan
    elif where == "middle":
        f[:, nzi // 2][:, cols] = np.nan
    elif where == "all":
        f[:, :, cols] = np.nan
    else:
        f[rng.uniform(size=f.shape) < 0.15] = np.nan
    inL = vr.Levels(vr.FIELD, nzi, field=f)
    got = fa.vertical_interpolate_host(method, data, _fa_levels(fa, inL), None, level1)
    _compare(method, got, *_want(method, data, inL, None, level1), label="NaN levels (%s)" % where)


@pytest.mark.parametrize("template", [False, True])
def test_device_entry_on_a_side_stream_equals_the_host_entry(fa, template):
    import torch
    nx, ny, nt, nzi, nzo = 257, 131, 3, 7, 20
    data, inL, outL, level1 = make_case(55, vr.HYBRID_SIGMA_AP, vr.FIELD if template else None, nx, ny, nt, nzi, nzo, "dec", False)
    rng = np.random.default_rng(6)
    vmin, vmax = rng.uniform(5., 100., (ny, nx)), rng.uniform(800., 1600., (ny, nx))
    host = fa.vertical_interpolate_host(vr.LIN_WEAK_EXTRA, data, _fa_levels(fa, inL), _fa_levels(fa, outL) if template else None, level1,
                                        validMin=vmin, validMax=vmax, clampMin=270., clampMax=300.)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_in = torch.from_numpy(data).cuda()
        d_min, d_max = torch.from_numpy(vmin).cuda(), torch.from_numpy(vmax).cuda()
        d_out = torch.full((nt, nzo, ny, nx), -1.0, dtype=torch.float32, device="cuda")
        li = _fa_levels(fa, inL, device=True)
        lo = _fa_levels(fa, outL, device=True) if template else None
        fa.vertical_interpolate_device(vr.LIN_WEAK_EXTRA, nx, ny, nt, d_in.data_ptr(), li, d_out.data_ptr(), outLevels=lo, level1=level1,
                                       d_validMin=d_min.data_ptr(), d_validMax=d_max.data_ptr(), clampMin=270., clampMax=300.,
                                       stream=side.cuda_stream)
        # the coefficient arrays were copied by the call: a second call with other coefficients must not disturb the first
        other = torch.empty_like(d_out)
        fa.vertical_interpolate_device(vr.LIN, nx, ny, nt, d_in.data_ptr(), fa.VerticalLevels.from_axis(np.arange(1., nzi + 1)),
                                       other.data_ptr(), level1=np.linspace(0., 9., nzo), stream=side.cuda_stream)
    side.synchronize()
    got = d_out.cpu().numpy()
    assert cases.same(got, host), cases.describe_mismatch(got, host)
    want = _want(vr.LIN_WEAK_EXTRA, data, inL, outL, level1, validMin=vmin, validMax=vmax, clampMin=270., clampMax=300.)[0]
    assert cases.same(got, want), cases.describe_mismatch(got, want)


@pytest.mark.parametrize("order", ["inc", "dec", "rep"])
@pytest.mark.parametrize("kind_in", [vr.FIELD, vr.AXIS, vr.HYBRID_SIGMA])
def test_bisection_and_walk_give_the_same_bits(fa, tuning_build, monkeypatch, kind_in, order):
    """Columns with strictly monotonic levels take a bisection instead of the walk over the column, and the walk handles 4 or 8
    output levels at once: every variant (forced through the tuning build's switches) must give the bits of the restatement.
    The targets include values so large that x - level rounds to the same double for neighbouring levels (the walk then keeps
    the FIRST of them) and +-inf, NaN and DBL_MAX."""
    nx, ny, nt, nzi, nzo = 53, 37, 2, 7, 11
    data, inL, _, level1 = make_case(60, kind_in, None, nx, ny, nt, nzi, nzo, order, False)
    level1[-7:] = [1e30, -1e30, 3e19, np.inf, -np.inf, np.nan, np.finfo(np.float64).max]
    want = _want(vr.LIN, data, inL, None, level1)[0]
    wrong = []
    for bisect, group in ((1, 4), (0, 4), (1, 8), (0, 8)):
        monkeypatch.setenv("FIMEX_AMD_VERTICAL_BISECT", str(bisect))
        monkeypatch.setenv("FIMEX_AMD_VERTICAL_GROUP", str(group))
        got = fa.vertical_interpolate_host(vr.LIN, data, _fa_levels(fa, inL), None, level1)
        if not cases.same(got, want):
            per_level = [int(np.count_nonzero(~_same_cells(got[:, k], want[:, k]))) for k in range(nzo)]
            wrong.append((bisect, group, per_level))
    assert not wrong, wrong


@pytest.mark.parametrize("group", [4, 8])
@pytest.mark.parametrize("nzo", [1, 3, 4, 5, 9])
def test_short_last_groups(fa, tuning_build, monkeypatch, nzo, group):
    """Output level counts below, at and above the group sizes: a short last group of 4 and of 8 (tuning build) stores its own
    levels only, each with its own value."""
    monkeypatch.setenv("FIMEX_AMD_VERTICAL_GROUP", str(group))
    data, inL, _, level1 = make_case(70 + nzo, vr.FIELD, None, 31, 9, 2, 7, nzo, "inc", False)
    got = fa.vertical_interpolate_host(vr.LIN, data, _fa_levels(fa, inL), None, level1)
    _compare(vr.LIN, got, *_want(vr.LIN, data, inL, None, level1))


def mixed_columns(seed, nx, ny, nt, nzi, nzo):
    """make_case on a level field whose columns alternate along x between strictly increasing levels (the bisection) and levels with
    repeats (the walk): both kinds sit in every wave."""
    data, incL, _, level1 = make_case(seed, vr.FIELD, None, nx, ny, nt, nzi, nzo, "inc", False)
    _, repL, _, _ = make_case(seed + 1, vr.FIELD, None, nx, ny, nt, nzi, nzo, "rep", False)
    inc, rep = incL.field.reshape(nt, nzi, ny, nx), repL.field.reshape(nt, nzi, ny, nx)
    field = np.where((np.arange(nx) % 2 == 0)[None, None, None, :], inc, rep)
    mono = np.all(np.diff(field, axis=1) > 0, axis=1)  # make_case puts a level on a target in some columns: not every even one
    assert mono[..., 0::2].mean() > 0.5 and not mono[..., 1::2].any()
    for t in range(nt):
        waves = mono[t].reshape(-1)[:(nx * ny) // 64 * 64].reshape(-1, 64)
        assert np.all(waves.any(axis=1) & ~waves.all(axis=1))
    return data, vr.Levels(vr.FIELD, nzi, field=field), level1


@pytest.mark.parametrize("method", vr.LINEAR_FAMILY)
def test_bisecting_and_walking_columns_in_one_wave(fa, method):
    data, inL, level1 = mixed_columns(80, 53, 37, 2, 7, 11)
    got = fa.vertical_interpolate_host(method, data, _fa_levels(fa, inL), None, level1)
    _compare(method, got, *_want(method, data, inL, None, level1))


@pytest.mark.parametrize("plane", [BLOCK - 1, BLOCK, BLOCK + 1])
def test_planes_around_a_workgroup(fa, plane):
    """One column less than a workgroup's, exactly its columns and one more, two positions of the unlimited dimension: the output
    on the device between guard bytes."""
    import torch
    nt, nzi, nzo = 2, 7, 5
    data, inL, _, level1 = make_case(90 + plane, vr.HYBRID_SIGMA, None, plane, 1, nt, nzi, nzo, "dec", False)
    want = _want(vr.LIN_WEAK_EXTRA, data, inL, None, level1)[0]
    li = _fa_levels(fa, inL, device=True)
    d_in = torch.from_numpy(data).cuda()
    guard = 64
    d_out = torch.full((guard + nt * nzo * plane + guard,), -7.0, dtype=torch.float32, device="cuda")
    fa.vertical_interpolate_device(vr.LIN_WEAK_EXTRA, plane, 1, nt, d_in.data_ptr(), li, d_out.data_ptr() + 4 * guard, level1=level1,
                                   stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert np.all(raw[:guard] == -7.0) and np.all(raw[-guard:] == -7.0), "wrote outside the output"
    got = raw[guard:-guard].reshape(want.shape)
    assert cases.same(got, want), cases.describe_mismatch(got, want)


def test_errors(fa):
    import torch
    nx, ny, nt, nzi = 8, 4, 1, 3
    data = np.zeros((nt, nzi, ny, nx), np.float32)
    ps = np.full((nt, ny, nx), 1000., np.float32)
    axis = fa.VerticalLevels.from_axis([1., 2., 3.])
    l1 = [1.5, 2.5]
    with pytest.raises(fa.FimexAmdError, match="unknown vertical interpolation method"):
        fa.vertical_interpolate_host(7, data, axis, None, l1)
    with pytest.raises(fa.FimexAmdError, match="unknown vertical interpolation method"):
        fa.vertical_interpolate_host(-1, data, axis, None, l1)
    with pytest.raises(fa.FimexAmdError, match="unknown vertical level kind"):
        fa.vertical_interpolate_host(vr.LIN, data, fa.VerticalLevels(5, nzi, axis=[1., 2., 3.]), None, l1)
    with pytest.raises(fa.FimexAmdError, match="unknown vertical level kind"):
        fa.vertical_interpolate_host(vr.LIN, data, axis, fa.VerticalLevels(-1, 2), None)
    with pytest.raises(fa.FimexAmdError, match="unknown vertical level kind"):
        fa.vertical_levels_host(fa.VerticalLevels(9, nzi), nx, ny, nt)
    # NULL where the kind needs an array
    for bad in (fa.VerticalLevels(vr.AXIS, nzi), fa.VerticalLevels(vr.FIELD, nzi), fa.VerticalLevels(vr.SIGMA, nzi, ps=ps),
                fa.VerticalLevels(vr.SIGMA, nzi, sigma=[.1, .5, 1.]), fa.VerticalLevels(vr.HYBRID_SIGMA, nzi, a=[1., 2., 3.], ps=ps),
                fa.VerticalLevels(vr.HYBRID_SIGMA_AP, nzi, b=[1., 2., 3.], ps=ps), fa.VerticalLevels(vr.HYBRID_SIGMA_AP, nzi, ap=[1., 2., 3.], b=[0., 0., 0.])):
        with pytest.raises(fa.FimexAmdError, match="needs"):
            fa.vertical_interpolate_host(vr.LIN, data, bad, None, l1)
        with pytest.raises(fa.FimexAmdError, match="needs"):
            fa.vertical_levels_host(bad, nx, ny, nt)
    with pytest.raises(fa.FimexAmdError, match="level1"):
        fa.vertical_interpolate_host(vr.LIN, data, axis, None, None)
    # no levels with non-empty columns
    with pytest.raises(fa.FimexAmdError, match="nzi == 0"):
        fa.vertical_interpolate_host(vr.LIN, np.zeros((nt, 0, ny, nx), np.float32), fa.VerticalLevels(vr.AXIS, 0), None, l1)
    with pytest.raises(fa.FimexAmdError, match="nzo == 0"):
        fa.vertical_interpolate_host(vr.LIN, data, axis, None, [])
    # ... and nothing to complain about when the columns are empty
    assert fa.vertical_interpolate_host(vr.LIN, np.zeros((nt, 0, 0, nx), np.float32), fa.VerticalLevels(vr.AXIS, 0), None, []).size == 0
    # the output may not alias the input
    d = torch.zeros(nt * nzi * ny * nx, dtype=torch.float32, device="cuda")
    with pytest.raises(fa.FimexAmdError, match="overlaps"):
        fa.vertical_interpolate_device(vr.LIN, nx, ny, nt, d.data_ptr(), axis, d.data_ptr(), level1=l1)
    with pytest.raises(fa.FimexAmdError, match="overlaps"):
        fa.vertical_interpolate_device(vr.LIN, nx, ny, nt, d.data_ptr(), axis, d.data_ptr() + 4 * nx * ny, level1=l1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ working size
def _strips(fn, ny, parts=16):
    """fn(j0, j1) on row strips in threads (numpy releases the GIL on large arrays); results joined along y."""
    edges = np.linspace(0, ny, parts + 1).astype(int)
    with concurrent.futures.ThreadPoolExecutor(max_workers=parts) as ex:
        return np.concatenate(list(ex.map(lambda p: fn(edges[p], edges[p + 1]), range(parts))), axis=2)


def test_working_size_hybrid_to_pressure(fa):
    """65 hybrid levels -> 20 pressure levels on 1000 x 1000, nt = 2: every cell for the linear method, a 1-in-97 sample of
    the columns for log."""
    import torch
    nx = ny = 1000
    nt, nzi, nzo = 2, 65, 20
    rng = np.random.default_rng(2024)
    v = _profile(rng, nzi, 10.0, 1000.0, "inc")
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    terrain = 0.5 + 0.5 * np.sin(0.011 * ii) * np.cos(0.007 * jj)  # surface pressure from 600 (mountains) to 1040
    ps = np.stack([(600. + 440. * terrain + 3. * rng.normal(size=(ny, nx)) + 5. * t) for t in range(nt)]).astype(np.float32)
    level1 = np.array([10., 20., 30., 50., 70., 100., 150., 200., 250., 300., 400., 500., 600., 700., 800., 850., 900., 925., 950., 1000.])
    sample = (np.arange(ny * nx) % 97 == 0).reshape(ny, nx)
    coeff = _coefficients(vr.HYBRID_SIGMA_AP, v)
    # the log condition in the sampled columns: redraw their ps until every target is clear of every level
    for _ in range(2000):
        cols = vr.level_field(vr.Levels(vr.HYBRID_SIGMA_AP, nzi, ps=ps[:, sample][:, None, :], **coeff), nt, 1, int(sample.sum())).astype(np.float64)
        gap = np.abs(cols[:, :, None] - level1[None, None, :, None, None])  # [nt][nzi][nzo][1][n]
        bad = np.any((gap != 0) & (gap < 1e-3 * np.maximum(cols[:, :, None], level1[None, None, :, None, None])), axis=(1, 2))[:, 0]
        if not bad.any():
            break
        sub = ps[:, sample]
        sub[bad] = (sub[bad] + rng.uniform(-2., 2., int(bad.sum()))).astype(np.float32)
        ps[:, sample] = sub
    else:
        raise AssertionError("no safe surface pressure found")
    data = cases.field(nt * nzi, ny, nx, seed=77, nan_frac=0.05, extremes=False).reshape(nt, nzi, ny, nx)
    inL = vr.Levels(vr.HYBRID_SIGMA_AP, nzi, ps=ps, **coeff)
    d_in = torch.from_numpy(data).cuda()
    d_out = torch.empty((nt, nzo, ny, nx), dtype=torch.float32, device="cuda")
    li = _fa_levels(fa, inL, device=True)
    stream = torch.cuda.current_stream().cuda_stream
    x = level1[None, :, None, None]

    fa.vertical_interpolate_device(vr.LIN, nx, ny, nt, d_in.data_ptr(), li, d_out.data_ptr(), level1=level1, stream=stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    want = _strips(lambda j0, j1: vr.interpolate(vr.LIN, data[:, :, j0:j1], vr.level_field(
        vr.Levels(vr.HYBRID_SIGMA_AP, nzi, ps=ps[:, j0:j1], **coeff), nt, j1 - j0, nx), x), ny)
    assert np.count_nonzero(np.isnan(want)) > nt * ny * nx  # below-ground targets and NaN data
    assert cases.same(got, want), cases.describe_mismatch(got, want)

    fa.vertical_interpolate_device(vr.LOG, nx, ny, nt, d_in.data_ptr(), li, d_out.data_ptr(), level1=level1, stream=stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()[:, :, sample][:, :, None, :]
    n = int(sample.sum())
    sdata = np.ascontiguousarray(data[:, :, sample][:, :, None, :])
    slev = vr.level_field(vr.Levels(vr.HYBRID_SIGMA_AP, nzi, ps=ps[:, sample][:, None, :], **coeff), nt, 1, n)
    _assert_safe(slev, np.broadcast_to(x, (nt, nzo, 1, n)))
    _compare(vr.LOG, got, *vr.interpolate(vr.LOG, sdata, slev, x, details=True), label="working size, %d sampled columns" % n)


def test_zz_report_bit_identical_share_of_the_log_methods():
    """Recorded, not asserted: the share of finite cells of the log / loglog comparisons above that are bit-identical."""
    same = sum(s for s, _ in _shares)
    total = sum(n for _, n in _shares)
    print("vertical log/loglog comparisons: %d of %d finite cells bit-identical (%.4f %%)" % (same, total, 100.0 * same / max(total, 1)))
