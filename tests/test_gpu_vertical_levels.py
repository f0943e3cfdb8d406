"""The vertical level converters on the GPU (include/fimex_amd.h, 8f n6) against tests/vertical_levels_ref.py, the CPU restatement
that tests/test_vertical_levels_ref.py pins to the reference's known answers.  Every cell is compared; NaN and infinity positions
must be identical.

Tolerances, from the arithmetic (the device's log / exp are not the host's, each within about one unit in the last place of a
double):
  integration        |got - want| <= 2^-23 * sum_{j<=k} |lt_j| + 2^-23 * |want|     (+ 2^-50 * |a| with a topography term):
                     the device log can move a layer's float rounding by one float step of that layer, and the final rounding
                     by one step of the result
  ocean depth        bit-identical (no transcendental)
  standard altitude, |got - want| <= 2^-23 * |want| + 2^-50 * |value before the topography term|
  standard pressure
The share of bit-identical cells is printed (recorded in DESIGN.md 6.6, not asserted).
"""
import numpy as np
import pytest

import cases
import vertical_levels_ref as vl
import vertical_ref as vr

pytestmark = pytest.mark.gpu

G = vl.EARTH_GRAVITY


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    lib = capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    assert hasattr(lib, "fimex_amd_vertical_altitude_integrate_device")
    return capi


def _fa_levels(fa, lv, device=False):
    """vertical_ref.Levels -> capi.VerticalLevels (device=True: ps / field as torch tensors, kept alive by the result)."""
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


def _dev(a, dtype):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _compare(got, want, tol, label):
    """NaN and infinity positions identical, every finite cell within tol; prints the share of bit-identical cells."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN positions differ in %d cells" % (label, np.count_nonzero(gn != wn))
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), label + ": infinities differ"
    fin = np.isfinite(want)
    g, w = got[fin].astype(np.float64), want[fin].astype(np.float64)
    err = np.abs(g - w)
    t = np.broadcast_to(tol, want.shape)[fin]
    same = np.count_nonzero(got[fin].view(np.uint32) == want[fin].view(np.uint32))
    print("vertical levels %s: %d finite cells, %d NaN, %.4f %% bit-identical, max error / tolerance %.3f"
          % (label, g.size, np.count_nonzero(wn), 100.0 * same / max(g.size, 1), float(np.max(err / np.maximum(t, 1e-300))) if g.size else 0.0))
    bad = err > t
    assert not np.any(bad), "%s: %d cells over the tolerance; worst: got %r want %r tol %r" % (
        label, np.count_nonzero(bad), g[bad][np.argmax((err - t)[bad])], w[bad][np.argmax((err - t)[bad])], t[bad][np.argmax((err - t)[bad])])
    return same, g.size


def _integration_tolerance(want, a, spread, topo):
    with np.errstate(invalid="ignore"):
        tol = 2.0 ** -23 * spread + 2.0 ** -23 * np.abs(want.astype(np.float64))
        if topo is not None:
            tol = tol + 2.0 ** -50 * np.abs(a)
    return tol


def _topography(rng, ny, nx, which):
    """which: None, "+1", "-1" (an altitude in m) or "-1/g" (a geopotential): (topo, topoFactor)."""
    if which is None:
        return None, -1.0
    alt = rng.uniform(0.0, 2500.0, (ny, nx))
    if which == "-1/g":
        return alt * G, -1.0 / G
    return alt, float(which)


TOPOS = (None, "+1", "-1", "-1/g")


def _integrate_host(fa, lv, nx, ny, nt, T, q, sap, sgp, flag, topo, factor):
    return fa.vertical_altitude_integrate_host(_fa_levels(fa, lv), nx, ny, nt, T, sap, sgp, specificHumidity=q, surfaceFirst=flag,
                                               topo=topo, topoFactor=factor)


@pytest.mark.parametrize("humidity", [True, False], ids=["q", "dry"])
@pytest.mark.parametrize("surface_first", [True, False], ids=["up", "down"])
@pytest.mark.parametrize("kind", vr.KINDS)
def test_integration_matches_the_cpu_restatement(fa, kind, surface_first, humidity):
    """Each pressure kind, both directions (AUTO must give the bits of the explicit flag it implies), humidity on and off, the
    topography term cycling through off, +1, -1 and -1 / g; nt > 1 and nx not a multiple of 64."""
    i = kind * 4 + int(surface_first) * 2 + int(humidity)
    nx, ny, nt, nz = ((53, 37, 2, 65), (131, 9, 3, 7), (70, 11, 2, 20))[i % 3]
    lv, T, q, sap, sgp = vl.make_atmosphere(100 + i, kind, nx, ny, nt, nz, surface_first)
    if not humidity:
        q = None
    topo, factor = _topography(np.random.default_rng(i), ny, nx, TOPOS[i % 4])
    want, a, spread = vl.altitude_field(lv, nt, ny, nx, T, q, sap, sgp, int(surface_first), topo, factor)
    assert np.all(np.isfinite(want)), "the inputs keep the reference finite"
    got = _integrate_host(fa, lv, nx, ny, nt, T, q, sap, sgp, int(surface_first), topo, factor)
    auto = _integrate_host(fa, lv, nx, ny, nt, T, q, sap, sgp, fa.VORDER_AUTO, topo, factor)
    assert vl.surface_first(vr.level_field(lv, nt, ny, nx)) == surface_first
    assert cases.same(auto, got), "AUTO differs from the explicit flag"
    other = _integrate_host(fa, lv, nx, ny, nt, T, q, sap, sgp, int(not surface_first), topo, factor)
    assert not cases.same(other, got), "the direction flag has no effect"
    _compare(got, want, _integration_tolerance(want, a, spread, topo), "integration kind %d %s %s topo %s" % (
        kind, "up" if surface_first else "down", "q" if humidity else "dry", TOPOS[i % 4]))


@pytest.mark.parametrize("which", TOPOS, ids=["none", "plus", "minus", "geopotential"])
def test_integration_topography(fa, which):
    nx, ny, nt, nz = 53, 37, 3, 65
    lv, T, q, sap, sgp = vl.make_atmosphere(7, vr.HYBRID_SIGMA_AP, nx, ny, nt, nz, False)
    topo, factor = _topography(np.random.default_rng(8), ny, nx, which)
    want, a, spread = vl.altitude_field(lv, nt, ny, nx, T, q, sap, sgp, vl.AUTO, topo, factor)
    got = _integrate_host(fa, lv, nx, ny, nt, T, q, sap, sgp, fa.VORDER_AUTO, topo, factor)
    _compare(got, want, _integration_tolerance(want, a, spread, topo), "integration topo %s" % which)
    if which is not None:
        plain = _integrate_host(fa, lv, nx, ny, nt, T, q, sap, sgp, fa.VORDER_AUTO, None, 0.0)
        assert np.max(np.abs(got - plain)) > 100.0  # the term is applied


@pytest.mark.parametrize("kind", [vr.HYBRID_SIGMA_AP, vr.FIELD])
@pytest.mark.parametrize("surface_first", [True, False], ids=["up", "down"])
def test_integration_with_nan(fa, kind, surface_first):
    """2 % NaN in T and a NaN in one ps cell: NaN from that level upward, in exactly the reference's cells."""
    nx, ny, nt, nz = 53, 37, 2, 65
    lv, T, q, sap, sgp = vl.make_atmosphere(11 + kind, kind, nx, ny, nt, nz, surface_first, nan_frac=0.02)
    sap[1, 3, 5] = np.nan
    if lv.ps is not None:
        lv.ps[1, 3, 5] = np.nan
    topo, factor = _topography(np.random.default_rng(12), ny, nx, "-1")
    want, a, spread = vl.altitude_field(lv, nt, ny, nx, T, q, sap, sgp, int(surface_first), topo, factor)
    assert np.all(np.isnan(want[1, :, 3, 5])) and 0.2 < np.isnan(want).mean() < 0.9
    got = _integrate_host(fa, lv, nx, ny, nt, T, q, sap, sgp, int(surface_first), topo, factor)
    _compare(got, want, _integration_tolerance(want, a, spread, topo), "integration with NaN, kind %d" % kind)


def test_integration_one_megacolumn(fa):
    """1000 x 1000 x 65 on device buffers, hybrid levels, humidity, height above ground."""
    import torch
    nx, ny, nt, nz = 1000, 1000, 1, 65
    lv, T, q, sap, sgp = vl.make_atmosphere(21, vr.HYBRID_SIGMA_AP, nx, ny, nt, nz, False)
    topo = sgp[0].astype(np.float64)
    factor = -1.0 / G
    d = [_dev(x, np.float32) for x in (T, q, sap, sgp)]
    d_topo = _dev(topo, np.float64)
    out = torch.full((nt, nz, ny, nx), -1.0, dtype=torch.float32, device="cuda")
    levels = _fa_levels(fa, lv, device=True)
    fa.vertical_altitude_integrate_device(levels, nx, ny, nt, d[0].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), out.data_ptr(),
                                          d_specificHumidity=d[1].data_ptr(), surfaceFirst=fa.VORDER_AUTO, d_topo=d_topo.data_ptr(),
                                          topoFactor=factor, stream=_stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want, a, spread = vl.altitude_field(lv, nt, ny, nx, T, q, sap, sgp, vl.AUTO, topo, factor)
    assert np.all(np.isfinite(want)) and want.min() > 0
    _compare(got, want, _integration_tolerance(want, a, spread, topo), "integration 1000 x 1000 x 65")


@pytest.mark.parametrize("with_eta", [True, False], ids=["eta", "no_eta"])
@pytest.mark.parametrize("generation", [1, 2])
def test_ocean_depth_is_bit_identical(fa, generation, with_eta):
    rng = np.random.default_rng(30 + generation)
    for nx, ny, nt, nz in ((53, 37, 3, 35), (131, 9, 1, 3), (70, 5, 2, 1)):
        s = -np.sort(rng.uniform(0, 1, nz))[::-1]
        C = -(np.abs(s) ** 1.7)
        depth = np.exp(rng.uniform(np.log(5.0), np.log(5000.0), (ny, nx)))
        depth[0, :4] = (20.0, 20.0 * (1 + 1e-9), 20.0 * (1 - 1e-9), 19.0)  # on and next to depth_c
        eta = rng.uniform(-2.0, 2.0, (nt, ny, nx)) if with_eta else None
        if with_eta:
            eta[0, 1, 1] = np.nan
            eta[0, 1, 2] = 0.0
        want = vl.ocean_depth_field(generation, s, C, 20.0, depth, eta, nt)
        got = fa.vertical_ocean_depth_host(generation, nx, ny, nt, s, C, 20.0, depth, eta)
        assert cases.same(got, want), cases.describe_mismatch(got, want)
        assert np.isnan(want).sum() == (nz if with_eta else 0)


@pytest.mark.parametrize("which", [None, "-1", "-1/g"], ids=["none", "minus", "geopotential"])
@pytest.mark.parametrize("kind", vr.KINDS)
def test_standard_altitude(fa, kind, which):
    nx, ny, nt, nz = ((53, 37, 2, 20), (131, 9, 3, 7))[kind % 2]
    lv, _, _, _, _ = vl.make_atmosphere(40 + kind, kind, nx, ny, nt, nz, kind % 2 == 0)
    topo, factor = _topography(np.random.default_rng(41), ny, nx, which)
    want, alt = vl.standard_altitude_field(lv, nt, ny, nx, topo, factor)
    got = fa.vertical_standard_altitude_host(_fa_levels(fa, lv), nx, ny, nt, topo, factor)
    _compare(got, want, 2.0 ** -23 * np.abs(want.astype(np.float64)) + 2.0 ** -50 * np.abs(alt), "standard altitude kind %d topo %s" % (kind, which))


@pytest.mark.parametrize("which", [None, "+1"], ids=["none", "plus"])
@pytest.mark.parametrize("kind", vr.KINDS)
def test_standard_pressure(fa, kind, which):
    """Altitude (or, with the topography term, height) levels of every kind: the pressure kinds' formulas with coefficients that
    make metres."""
    nx, ny, nt, nz = ((53, 37, 2, 20), (131, 9, 3, 7))[kind % 2]
    rng = np.random.default_rng(50 + kind)
    c = np.sort(rng.uniform(0.0, 1.0, nz))
    surf = rng.uniform(0.0, 1500.0, (nt, ny, nx)).astype(np.float32)  # stands where ps stands in the formulas
    lv = {vr.FIELD: lambda: vr.Levels(vr.FIELD, nz, field=rng.uniform(-300.0, 30000.0, (nt, nz, ny, nx))),
          vr.AXIS: lambda: vr.Levels(vr.AXIS, nz, axis=np.concatenate(([10.0, 80.0, 100.0, 500.0][:min(4, nz)], 20000.0 * c[:max(nz - 4, 0)]))),
          vr.SIGMA: lambda: vr.Levels(vr.SIGMA, nz, sigma=c, ptop=20000.0, ps=surf),
          vr.HYBRID_SIGMA: lambda: vr.Levels(vr.HYBRID_SIGMA, nz, a=c, b=1 - c, p0=20000.0, ps=surf),
          vr.HYBRID_SIGMA_AP: lambda: vr.Levels(vr.HYBRID_SIGMA_AP, nz, ap=20000.0 * c, b=1 - c, ps=surf)}[kind]()
    topo, factor = _topography(rng, ny, nx, which)
    want, h = vl.standard_pressure_field(lv, nt, ny, nx, topo, factor)
    assert np.all(np.isfinite(want)) and want.min() > 0
    got = fa.vertical_standard_pressure_host(_fa_levels(fa, lv), nx, ny, nt, topo, factor)
    _compare(got, want, 2.0 ** -23 * np.abs(want.astype(np.float64)) + 2.0 ** -50 * np.abs(h), "standard pressure kind %d topo %s" % (kind, which))


def test_standard_altitude_and_pressure_invert_each_other(fa):
    nx, ny, nt = 33, 5, 1
    p = np.array([1013.25, 1000.0, 850.0, 500.0, 100.0, 10.0])
    alt = fa.vertical_standard_altitude_host(_fa_levels(fa, vr.Levels(vr.AXIS, p.size, axis=p)), nx, ny, nt)
    assert alt[0, 0, 0, 0] == 0.0 and np.all(np.diff(alt[0, :, 2, 7]) > 0)
    back = fa.vertical_standard_pressure_host(_fa_levels(fa, vr.Levels(vr.FIELD, p.size, field=alt)), nx, ny, nt)
    assert np.allclose(back[0, :, 2, 7], p, rtol=1e-5)


def test_host_entries_equal_device_entries(fa):
    import torch
    nx, ny, nt, nz = 53, 37, 2, 20
    rng = np.random.default_rng(60)
    st = _stream()
    new = lambda: torch.zeros((nt, nz, ny, nx), dtype=torch.float32, device="cuda")
    topo = rng.uniform(0.0, 2500.0, (ny, nx))
    d_topo = _dev(topo, np.float64)
    for kind in (vr.FIELD, vr.SIGMA):
        lv, T, q, sap, sgp = vl.make_atmosphere(61 + kind, kind, nx, ny, nt, nz, True, nan_frac=0.02)
        d = [_dev(x, np.float32) for x in (T, q, sap, sgp)]
        dl = _fa_levels(fa, lv, device=True)
        for use_q in (True, False):
            out = new()
            fa.vertical_altitude_integrate_device(dl, nx, ny, nt, d[0].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), out.data_ptr(),
                                                  d_specificHumidity=d[1].data_ptr() if use_q else None, surfaceFirst=fa.VORDER_AUTO,
                                                  d_topo=d_topo.data_ptr(), topoFactor=-1.0, stream=st)
            torch.cuda.synchronize()
            host = _integrate_host(fa, lv, nx, ny, nt, T, q if use_q else None, sap, sgp, fa.VORDER_AUTO, topo, -1.0)
            assert np.isnan(host).any() and cases.same(out.cpu().numpy(), host)
        out = new()
        fa.vertical_standard_altitude_device(dl, nx, ny, nt, out.data_ptr(), d_topo=d_topo.data_ptr(), topoFactor=-1.0, stream=st)
        torch.cuda.synchronize()
        assert cases.same(out.cpu().numpy(), fa.vertical_standard_altitude_host(_fa_levels(fa, lv), nx, ny, nt, topo, -1.0))
        out = new()
        fa.vertical_standard_pressure_device(dl, nx, ny, nt, out.data_ptr(), d_topo=None, stream=st)
        torch.cuda.synchronize()
        assert cases.same(out.cpu().numpy(), fa.vertical_standard_pressure_host(_fa_levels(fa, lv), nx, ny, nt))
    s, C = -np.linspace(0.98, 0.02, nz), -np.linspace(0.98, 0.02, nz) ** 2
    depth, eta = rng.uniform(5.0, 4000.0, (ny, nx)), rng.uniform(-1.0, 1.0, (nt, ny, nx))
    d_depth, d_eta = _dev(depth, np.float64), _dev(eta, np.float64)
    for gen in (1, 2):
        for e, d_e in ((eta, d_eta), (None, None)):
            out = new()
            fa.vertical_ocean_depth_device(gen, nx, ny, nt, s, C, 15.0, d_depth.data_ptr(), out.data_ptr(), d_eta=_ptr(d_e), stream=st)
            torch.cuda.synchronize()
            assert cases.same(out.cpu().numpy(), fa.vertical_ocean_depth_host(gen, nx, ny, nt, s, C, 15.0, depth, e))


def test_argument_errors(fa):
    import torch
    nx, ny, nt, nz = 8, 4, 1, 3
    vol = torch.zeros((nt, nz, ny, nx), dtype=torch.float32, device="cuda")
    out = torch.zeros_like(vol)
    pl = torch.full((nt, ny, nx), 1000.0, dtype=torch.float32, device="cuda")
    dbl = torch.zeros((nt, ny, nx), dtype=torch.float64, device="cuda")
    axis = fa.VerticalLevels.from_axis(np.array([900.0, 500.0, 100.0]))
    T, P, O = vol.data_ptr(), pl.data_ptr(), out.data_ptr()

    def raises(match, fn, *a, **kw):
        with pytest.raises(fa.FimexAmdError, match=match):
            fn(*a, **kw)
    integ = fa.vertical_altitude_integrate_device
    raises("air temperature", integ, axis, nx, ny, nt, None, P, P, O)
    raises("surface pressure", integ, axis, nx, ny, nt, T, None, P, O)
    raises("surface geopotential", integ, axis, nx, ny, nt, T, P, None, O)
    raises("output", integ, axis, nx, ny, nt, T, P, P, None)
    raises("surfaceFirst", integ, axis, nx, ny, nt, T, P, P, O, surfaceFirst=2)
    raises("surfaceFirst", integ, axis, nx, ny, nt, T, P, P, O, surfaceFirst=-2)
    raises("overlaps the air temperature", integ, axis, nx, ny, nt, T, P, P, T)
    raises("overlaps the specific humidity", integ, axis, nx, ny, nt, T, P, P, O, d_specificHumidity=O + 16)
    raises("overlaps the surface pressure", integ, axis, nx, ny, nt, T, O + 4 * nx, P, O)
    raises("overlaps the topography", integ, axis, nx, ny, nt, T, P, P, dbl.data_ptr(), d_topo=dbl.data_ptr())
    raises("nz == 0", integ, fa.VerticalLevels.from_axis(np.zeros(0)), nx, ny, nt, T, P, P, O)
    raises("unknown vertical level kind", integ, fa.VerticalLevels(9, nz), nx, ny, nt, T, P, P, O)
    raises("level field", integ, fa.VerticalLevels(fa.VLEVEL_FIELD, nz), nx, ny, nt, T, P, P, O)
    raises("overlaps the level field", integ, fa.VerticalLevels.from_field(O, nz), nx, ny, nt, T, P, P, O)
    raises("needs ps", integ, fa.VerticalLevels(fa.VLEVEL_SIGMA, nz, sigma=np.ones(nz)), nx, ny, nt, T, P, P, O)
    for fn in (fa.vertical_standard_altitude_device, fa.vertical_standard_pressure_device):
        raises("output", fn, axis, nx, ny, nt, None)
        raises("nz == 0", fn, fa.VerticalLevels.from_axis(np.zeros(0)), nx, ny, nt, O)
        raises("unknown vertical level kind", fn, fa.VerticalLevels(-3, nz), nx, ny, nt, O)
        raises("overlaps the level field", fn, fa.VerticalLevels.from_field(O, nz), nx, ny, nt, O)
        raises("overlaps ps", fn, fa.VerticalLevels.sigma(np.ones(nz), 0.0, O + 8), nx, ny, nt, O)
    s = np.array([-0.9, -0.5, -0.1])
    ocean = fa.vertical_ocean_depth_device
    raises("generation", ocean, 3, nx, ny, nt, s, s, 10.0, dbl.data_ptr(), O)
    raises("generation", ocean, 0, nx, ny, nt, s, s, 10.0, dbl.data_ptr(), O)
    raises("nz == 0", ocean, 1, nx, ny, nt, np.zeros(0), np.zeros(0), 10.0, dbl.data_ptr(), O)
    assert fa.load().fimex_amd_vertical_ocean_depth_device(1, nx, ny, nz, nt, None, None, 10.0, dbl.data_ptr(), None, O, None) == fa.ERROR
    assert b"NULL s" in fa.load().fimex_amd_last_error()
    raises("depth", ocean, 1, nx, ny, nt, s, s, 10.0, None, O)
    raises("output", ocean, 2, nx, ny, nt, s, s, 10.0, dbl.data_ptr(), None)
    raises("overlaps the depth", ocean, 2, nx, ny, nt, s, s, 10.0, O + 32, O)
    raises("overlaps eta", ocean, 2, nx, ny, nt, s, s, 10.0, dbl.data_ptr(), O, d_eta=O)
    # nothing to do is no error
    integ(axis, 0, ny, nt, None, None, None, None)
    ocean(1, nx, 0, nt, s, s, 10.0, None, None)


@pytest.mark.parametrize("method", [vr.LIN, vr.NN], ids=["linear", "nearest"])
def test_height_levels_end_to_end(fa, method):
    """Hybrid levels, T, q, ps and orography -> heights above ground on the GPU -> interpolation to fixed heights, all on device
    buffers.  The interpolation must be vertical_ref's, bit for bit, of the same GPU-made field (the field itself is compared in
    the tests above)."""
    import torch
    nx, ny, nt, nz = 131, 37, 2, 65
    lv, T, q, sap, sgp = vl.make_atmosphere(70, vr.HYBRID_SIGMA_AP, nx, ny, nt, nz, False)
    sgp[1] = sgp[0]  # the orography does not move
    topo = sgp[0].astype(np.float64)
    data = cases.field(nt * nz, ny, nx, seed=71, nan_frac=0.03).reshape(nt, nz, ny, nx)
    level1 = np.array([-100.0, 10.0, 80.0, 100.0, 500.0, 60000.0])  # the first below every lowest level, the last above every highest
    st = _stream()
    d = [_dev(x, np.float32) for x in (T, q, sap, sgp, data)]
    d_topo = _dev(topo, np.float64)
    height = torch.zeros((nt, nz, ny, nx), dtype=torch.float32, device="cuda")
    out = torch.zeros((nt, level1.size, ny, nx), dtype=torch.float32, device="cuda")
    fa.vertical_altitude_integrate_device(_fa_levels(fa, lv, device=True), nx, ny, nt, d[0].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                          height.data_ptr(), d_specificHumidity=d[1].data_ptr(), surfaceFirst=fa.VORDER_AUTO,
                                          d_topo=d_topo.data_ptr(), topoFactor=-1.0 / G, stream=st)
    fa.vertical_interpolate_device(method, nx, ny, nt, d[4].data_ptr(), fa.VerticalLevels.from_field(height.data_ptr(), nz), out.data_ptr(),
                                   level1=level1, stream=st)
    torch.cuda.synchronize()
    field = height.cpu().numpy()
    assert np.all(np.isfinite(field)) and field.min() > level1[0] and field.max() < level1[-1]
    assert field[:, -1].max() < 80.0 and field[:, 0].min() > 500.0  # 80, 100 and 500 m lie inside every column
    want = vr.interpolate(method, data, field, level1[None, :, None, None])
    got = out.cpu().numpy()
    assert cases.same(got, want), cases.describe_mismatch(got, want)
    assert np.isfinite(got[:, 2:5]).mean() > 0.8
