"""fimex_amd_regrid_apply_vector_device / _host: both components of a vector pair regridded and rotated in one call
(CDMInterpolator::getDataSlice's vector branch).  The expected result everywhere is the CPU chain: interpolate_values on u and on
v, then vector_reproject_values; compared bit for bit on defined values with identical NaN positions (cases.same).

The dispatch rule under test, `_fused`: the fused kernel runs (path 1) exactly when the plan holds an LDS-staged
form (stagedCells > 0), the method is nearest or bilinear, and the batch has four pairs or more; everything else takes the three
existing launches (path 0)."""
import functools

import numpy as np
import pytest

import cases
import oracle

pytestmark = pytest.mark.gpu

# (inX, inY, outX, outY) and the positions of the geometries
GEOMETRY = {
    # staged tiles, gather tiles, odd source width, tiles that nearly fill their slot
    "A": ((403, 301, 130, 77), lambda: cases.coherent_positions(403, 301, 130, 77, seed=21, outliers=3)),
    # a seam, several tile rows per XCD
    "B": ((1441, 721, 900, 500), lambda: cases.coherent_positions(1441, 721, 900, 500, seed=31, wrap=True, outliers=4)),
    # overshoots the source: undefined cells and all three bilinear border forms
    "border": ((400, 300, 200, 200), lambda: cases.backward_positions(400, 300, 200, 200, seed=600)),
    "coord": ((300, 200, 157, 211), lambda: cases.backward_positions(300, 200, 157, 211, seed=100 + oracle.COORD_NN)),
}
MIN_NZ = 4  # STAGED_MIN_NZ


def _scattered():
    rng = np.random.default_rng(5)  # the plan of test_bilinear_scattered_positions_fall_back_to_gather
    return rng.uniform(-3, 512 + 2, 200 * 100), rng.uniform(-3, 384 + 2, 200 * 100)


GEOMETRY["C"] = ((512, 384, 200, 100), _scattered)


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


@functools.lru_cache(maxsize=None)
def _positions(geometry):
    return GEOMETRY[geometry][1]()


@functools.lru_cache(maxsize=None)
def _case(geometry, method, nz):
    """Inputs and the CPU chain's results, computed once per case and never written to: (u, v, regridded u, regridded v, rotated
    u, rotated v, matrix)."""
    inX, inY, outX, outY = GEOMETRY[geometry][0]
    px, py = _positions(geometry)
    u = cases.field(nz, inY, inX, seed=41)
    v = cases.field(nz, inY, inX, seed=42) - 280
    m = cases.rotation_matrix(outX, outY, seed=outX)
    ru = oracle.interpolate_values(method, px, py, u, inX, inY, outX, outY)
    rv = oracle.interpolate_values(method, px, py, v, inX, inY, outX, outY)
    wu, wv = oracle.vector_reproject_values(m, ru, rv, outX, outY)
    for a in (u, v, ru, rv, wu, wv, m):
        a.setflags(write=False)
    # a comparison of mostly NaN shows nothing (1 x 1 and 2 x 2 stencils on A and B: 98 % and 92 % of the rotated cells are
    # defined), and the rotation has to spread NaN to the other component
    if geometry in ("A", "B") and method in (oracle.NEAREST, oracle.BILINEAR):
        assert (~np.isnan(wu) & ~np.isnan(wv)).mean() > 0.9
        one = np.isnan(ru) ^ np.isnan(rv)
        assert np.count_nonzero(one) >= 1 and np.isnan(wu[one]).all() and np.isnan(wv[one]).all()
    return u, v, ru, rv, wu, wv, m


def _plans(fa, geometry, method):
    inX, inY, outX, outY = GEOMETRY[geometry][0]
    px, py = _positions(geometry)
    plan = fa.RegridPlan(method, px, py, inX, inY, outX, outY)
    vec = fa.VectorPlan(cases.rotation_matrix(outX, outY, seed=outX), outX, outY)
    return plan, vec


def _fused(plan, method, nz):
    """The dispatch rule: see the module's docstring."""
    return int(plan.info()["stagedCells"] > 0 and method in (oracle.NEAREST, oracle.BILINEAR) and nz >= MIN_NZ)


def _apply(fa, plan, vec, u, v, nz, stream=None):
    """The fused entry on torch buffers pre-filled with 7.0; returns (path, uOut, vOut) still on the device."""
    import torch
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        d_u, d_v = torch.from_numpy(np.array(u)).cuda(), torch.from_numpy(np.array(v)).cuda()
        d_uo = torch.full((nz, plan.outY, plan.outX), 7.0, device="cuda")
        d_vo = torch.full_like(d_uo, 7.0)
        path = plan.apply_vector_device(vec, d_u.data_ptr(), d_v.data_ptr(), nz, d_uo.data_ptr(), d_vo.data_ptr(), st.cuda_stream)
    return path, d_uo, d_vo, (d_u, d_v)


def _chain(fa, plan, vec, u, v, nz):
    """The three existing device launches on the same inputs."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    d_u, d_v = torch.from_numpy(np.array(u)).cuda(), torch.from_numpy(np.array(v)).cuda()
    a = torch.full((nz, plan.outY, plan.outX), 7.0, device="cuda")
    b = torch.full_like(a, 7.0)
    plan.apply_device(d_u.data_ptr(), nz, a.data_ptr(), st)
    plan.apply_device(d_v.data_ptr(), nz, b.data_ptr(), st)
    vec.reproject_values_device(a.data_ptr(), b.data_ptr(), nz, st)
    torch.cuda.synchronize()
    return a.cpu().numpy(), b.cpu().numpy()


def _check(got, want, what=""):
    assert cases.same(got, want), what + cases.describe_mismatch(got, want)


def _run_and_check(fa, geometry, method, nz, against_chain=False):
    import torch
    u, v, _, _, wu, wv, _ = _case(geometry, method, nz)
    plan, vec = _plans(fa, geometry, method)
    path, d_uo, d_vo, _keep = _apply(fa, plan, vec, u, v, nz)
    torch.cuda.synchronize()
    gu, gv = d_uo.cpu().numpy(), d_vo.cpu().numpy()
    _check(gu, wu, "u: ")
    _check(gv, wv, "v: ")
    if against_chain:
        cu, cv = _chain(fa, plan, vec, u, v, nz)
        _check(gu, cu, "u against the device chain: ")
        _check(gv, cv, "v against the device chain: ")
    return path, plan


@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("geometry,nz", [("A", 1), ("A", 3), ("A", 4), ("A", 5), ("A", 26), ("A", 51), ("B", 6)])
def test_parity_and_path(fa, method, geometry, nz):
    """Below the threshold, the threshold, an odd count, two and three z chunks of uneven length (25 pairs per block)."""
    path, plan = _run_and_check(fa, geometry, method, nz, against_chain=True)
    assert plan.info()["stagedCells"] > 0, "the plan lost its staged form"
    assert path == _fused(plan, method, nz)
    if (geometry, nz) == ("A", 26):
        assert path == 1  # otherwise nothing fused is tested


@pytest.mark.parametrize("geometry,method,nz", [("A", oracle.BICUBIC, 5), ("coord", oracle.COORD_NN, 5), ("C", oracle.BILINEAR, 5),
                                                ("C", oracle.NEAREST, 5), ("A", oracle.BILINEAR, 2)],
                         ids=["bicubic", "coord_nn", "scattered_bilinear", "scattered_nearest", "two_pairs"])
def test_fallbacks_take_the_three_launches(fa, geometry, method, nz):
    path, plan = _run_and_check(fa, geometry, method, nz)
    assert path == 0
    if geometry == "C":
        assert plan.info()["stagedCells"] == 0


@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("knob,value", [("STAGE2_DEPTH", "3"), ("STAGE2_USE_ALT", "0"), ("STAGE2_USE_ALT", "1"), ("STAGE2_ZPB", "1"),
                                        ("STAGE2_ZPB", "2"), ("STAGE2_ORDER", "0"), ("VECTOR_FUSED", "0")])
def test_ring_variants(fa, monkeypatch, tuning_build, method, knob, value):
    """The three-slot ring, both workgroup shapes, chunks of one and two pairs (the loop's head and tail with nothing in between),
    chunk-major order, and the switch that sends everything to the chain."""
    monkeypatch.setenv("FIMEX_AMD_" + knob, value)
    path, plan = _run_and_check(fa, "A", method, 9)
    assert plan.info()["stagedCells"] > 0
    assert path == (0 if knob == "VECTOR_FUSED" else 1)


@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR], ids=["nearest", "bilinear"])
def test_border_branches(fa, method):
    path, plan = _run_and_check(fa, "border", method, 10)
    info = plan.info()
    assert info["undefinedCells"] > 0
    if method == oracle.BILINEAR:
        assert info["borderCells"] > 0
    assert path == _fused(plan, method, 10)


def test_repeatable_on_the_same_plan_and_buffers(fa):
    """A wrong wait count shows here as a mismatch: the same plan and buffers 20 times, allocations of other sizes in between."""
    import torch
    nz = 6
    u, v, _, _, wu, wv, _ = _case("A", oracle.BILINEAR, nz)
    plan, vec = _plans(fa, "A", oracle.BILINEAR)
    st = torch.cuda.current_stream().cuda_stream
    d_u, d_v = torch.from_numpy(np.array(u)).cuda(), torch.from_numpy(np.array(v)).cuda()
    d_uo = torch.empty((nz, plan.outY, plan.outX), device="cuda")
    d_vo = torch.empty_like(d_uo)
    rng = np.random.default_rng(5)
    junk = []
    for it in range(20):
        junk.append(torch.empty(int(rng.integers(1, 64)) * 262144, device="cuda").normal_())
        if len(junk) > 6:
            junk.pop(0)
        d_uo.fill_(7.0)
        d_vo.fill_(7.0)
        assert plan.apply_vector_device(vec, d_u.data_ptr(), d_v.data_ptr(), nz, d_uo.data_ptr(), d_vo.data_ptr(), st) == 1
        torch.cuda.synchronize()
        _check(d_uo.cpu().numpy(), wu, "iteration %d, u: " % it)
        _check(d_vo.cpu().numpy(), wv, "iteration %d, v: " % it)


def test_host_form_equals_the_device_form(fa):
    import torch
    nz = 5
    u, v, _, _, wu, wv, _ = _case("A", oracle.BILINEAR, nz)
    plan, vec = _plans(fa, "A", oracle.BILINEAR)
    hu, hv = plan.apply_vector_host(vec, u, v)
    path, d_uo, d_vo, _keep = _apply(fa, plan, vec, u, v, nz)
    torch.cuda.synchronize()
    assert path == 1 and hu.shape == (nz, plan.outY, plan.outX)
    _check(hu, d_uo.cpu().numpy(), "u: ")
    _check(hv, d_vo.cpu().numpy(), "v: ")
    _check(hu, wu)
    _check(hv, wv)
    eu, ev = plan.apply_vector_host(vec, u[:0], v[:0])
    assert eu.shape == ev.shape == (0, plan.outY, plan.outX)


def test_one_plan_on_two_streams(fa):
    import torch
    nz = 6
    u, v, _, _, wu, wv, _ = _case("A", oracle.BILINEAR, nz)
    plan, vec = _plans(fa, "A", oracle.BILINEAR)
    torch.cuda.synchronize()
    runs = [_apply(fa, plan, vec, u, v, nz, stream=torch.cuda.Stream()) for _ in range(2)]
    torch.cuda.synchronize()
    for path, d_uo, d_vo, _keep in runs:
        assert path == 1
        _check(d_uo.cpu().numpy(), wu, "u: ")
        _check(d_vo.cpu().numpy(), wv, "v: ")


@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR], ids=["nearest", "bilinear"])
def test_length_is_preserved(fa, method):
    """test/testInterpolation.cc:575-578 on the fused result, against the regridded components before their rotation."""
    import torch
    nz = 5
    u, v, ru, rv, _, _, _ = _case("A", method, nz)
    plan, vec = _plans(fa, "A", method)
    path, d_uo, d_vo, _keep = _apply(fa, plan, vec, u, v, nz)
    torch.cuda.synchronize()
    assert path == 1
    gu, gv = d_uo.cpu().numpy(), d_vo.cpu().numpy()
    ok = np.isfinite(ru) & np.isfinite(rv) & (np.abs(ru) < 1e18) & (np.abs(rv) < 1e18)
    assert ok.mean() > 0.9
    l0 = ru[ok].astype(np.float64) ** 2 + rv[ok].astype(np.float64) ** 2
    l1 = gu[ok].astype(np.float64) ** 2 + gv[ok].astype(np.float64) ** 2
    assert np.all(np.abs(l1 - l0) <= 1e-5 * l0 + 1e-3)


def test_refusals_that_need_a_plan(fa):
    """Refused with a message, nothing launched: the output buffers keep their fill."""
    import torch
    nz = 4
    inX, inY, outX, outY = GEOMETRY["A"][0]
    plan, vec = _plans(fa, "A", oracle.BILINEAR)
    st = torch.cuda.current_stream().cuda_stream
    d_in = torch.zeros((2, nz, inY, inX), device="cuda")
    d_out = torch.full((2, nz, outY, outX), 7.0, device="cuda")
    u, v, uo, vo = d_in[0].data_ptr(), d_in[1].data_ptr(), d_out[0].data_ptr(), d_out[1].data_ptr()
    fpx, fpy = cases.forward_positions(inX, inY, outX, outY, seed=11)
    forward = fa.RegridPlan(oracle.FWD_MEAN, fpx, fpy, inX, inY, outX, outY)
    with pytest.raises(fa.FimexAmdError, match="forward plan"):
        forward.apply_vector_device(vec, u, v, nz, uo, vo, st)
    other = fa.VectorPlan(cases.rotation_matrix(outY, outX, seed=1), outY, outX)  # ox and oy swapped
    with pytest.raises(fa.FimexAmdError, match="differs from the regrid plan's output grid"):
        plan.apply_vector_device(other, u, v, nz, uo, vo, st)
    with pytest.raises(fa.FimexAmdError, match="differs from the regrid plan's output grid"):
        plan.apply_vector_host(other, np.zeros((nz, inY, inX), np.float32), np.zeros((nz, inY, inX), np.float32))
    for args, names in (((u, v, uo, uo), "uOut and vOut"), ((u, v, uo, uo + 4 * (outX * outY * nz - 1)), "uOut and vOut"),
                        ((u, u, uo, vo), "u and v"), ((uo, v, uo, vo), "u and uOut"), ((u, vo, uo, vo), "v and vOut")):
        with pytest.raises(fa.FimexAmdError, match="buffers overlap: " + names):
            plan.apply_vector_device(vec, args[0], args[1], nz, args[2], args[3], st)
    assert plan.apply_vector_device(vec, 0, 0, 0, 0, 0, st) == 0  # nz == 0 succeeds and does nothing
    torch.cuda.synchronize()
    assert bool((d_out == 7.0).all())
