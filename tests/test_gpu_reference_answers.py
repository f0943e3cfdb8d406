"""The HIP path (through the C ABI) against answers of the reference's own C code, recorded in tests/golden/reference_answers.npz
(scripts/record_reference_answers.py ran the reference's unmodified sources).  Needs neither the reference nor oracle/_ref:
only tests/golden/ is read.  Each function gets the comparison it gets against the oracle in tests/test_gpu_parity.py and
tests/test_gpu_vertical.py: cases.same (bit-identical defined values, identical NaN positions), equal nChanged,
bit-identical doubles for the axis positions.  Positions the reference cannot take (divergences D1, D2 of
oracle/fimex_oracle.c; marked in the fixture, NaN in its outputs) must come out NaN here as well.
"""
import numpy as np
import pytest

import cases
import oracle
import reference_answers as ra

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


@pytest.fixture(scope="module")
def fx(golden_dir):
    return ra.load(golden_dir)


def _f32(bits):
    return bits.view(np.float32)


def test_regrid(fa, fx):
    names = fx.names("regrid")
    assert len(names) >= 2
    for name in names:
        c = fx.case(name)
        inX, inY, nz = (int(v) for v in c["shape"])
        n = c["px"].size
        for method in (oracle.NEAREST, oracle.BILINEAR, oracle.BICUBIC):
            want = _f32(c["out%d" % method]).reshape(nz, 1, n)
            assert np.all(np.isnan(want[:, 0, c["skip%d" % method].astype(bool)]))
            got = fa.RegridPlan(method, c["px"], c["py"], inX, inY, n, 1).apply_host(c["in"])
            assert cases.same(got, want), "%s method %d: %s" % (name, method, cases.describe_mismatch(got, want))


def test_fill2d(fa, fx):
    names = fx.names("fill2d")
    assert len(names) >= 2
    for name in names:
        c = fx.case(name)
        got, nch = fa.fill2d_host(c["in"], float(c["params"][0]), float(c["params"][1]), int(c["params"][2]))
        assert np.all(c["rc"] == oracle.OK)
        assert list(nch) == [int(v) for v in c["nChanged"]], name
        assert cases.same(got, _f32(c["out"])), "%s: %s" % (name, cases.describe_mismatch(got, _f32(c["out"])))


def test_creepfills(fa, fx):
    names = fx.names("creepfill2d")
    assert len(names) >= 2
    for name in names:
        c = fx.case(name)
        got, nch = fa.creepfill2d_host(c["in"], int(c["params"][0]), int(c["params"][1]))
        assert np.all(c["rc"] == oracle.OK)
        assert list(nch) == [int(v) for v in c["nChanged"]], name
        assert cases.same(got, _f32(c["out"])), "%s: %s" % (name, cases.describe_mismatch(got, _f32(c["out"])))
    names = fx.names("creepfillval2d")
    assert len(names) >= 2
    for name in names:
        c = fx.case(name)
        got, nch = fa.creepfillval2d_host(c["in"], float(c["params"][2]), int(c["params"][0]), int(c["params"][1]))
        assert np.all(c["rc"] == oracle.OK)
        assert list(nch) == [int(v) for v in c["nChanged"]], name
        assert cases.same(got, _f32(c["out"])), "%s: %s" % (name, cases.describe_mismatch(got, _f32(c["out"])))


def test_rotation(fa, fx):
    names = fx.names("rotation")
    assert names
    for name in names:
        c = fx.case(name)
        ox, oy, oz = (int(v) for v in c["shape"])
        plan = fa.VectorPlan(c["matrix"], ox, oy)
        gu, gv = plan.reproject_values_host(c["u"], c["v"])
        assert cases.same(gu, _f32(c["u_out"])), cases.describe_mismatch(gu, _f32(c["u_out"]))
        assert cases.same(gv, _f32(c["v_out"])), cases.describe_mismatch(gv, _f32(c["v_out"]))
        ga = plan.reproject_direction_host(c["angles"])
        assert cases.same(ga, _f32(c["angles_out"])), cases.describe_mismatch(ga, _f32(c["angles_out"]))


def test_points2position(fa, fx):
    names = fx.names("points2position")
    assert len(names) >= 4
    for name in names:
        c = fx.case(name)
        got = fa.points2position_host(c["points"], c["axis"], int(c["axis_type"]))
        np.testing.assert_array_equal(got, c["out"].view(np.float64), err_msg=name)  # as test_gpu_parity: equal values, NaN == NaN


def test_blends(fa, fx):
    c = fx.case("blend.a")
    seen = set()
    for k, (kind, a, b, x) in enumerate(c["kabx"]):
        rc = int(c["rc"][k])
        seen.add(rc)
        if rc != oracle.OK:
            with pytest.raises(fa.FimexAmdError):
                fa.get_values_1d_host(int(kind), c["A"], c["B"], a, b, x)
            continue
        got = fa.get_values_1d_host(int(kind), c["A"], c["B"], a, b, x)
        want = _f32(c["out"][k])
        assert cases.same(got, want), "kind %d a %g b %g x %g: %s" % (kind, a, b, x, cases.describe_mismatch(got, want))
    assert seen == {oracle.OK, oracle.ERROR}


def test_bad2nan_nan2bad(fa, fx):
    import torch
    c = fx.case("badvalue.a")
    stream = torch.cuda.current_stream().cuda_stream
    for k, bad in enumerate(_f32(c["bad"])):
        t = torch.from_numpy(c["in"].copy()).cuda()
        fa.bad2nan_device(t.data_ptr(), t.numel(), float(bad), stream)
        torch.cuda.synchronize()
        assert cases.same(t.cpu().numpy(), _f32(c["bad2nan"][k])), "bad2nan, bad value %r" % bad
        t = torch.from_numpy(c["in"].copy()).cuda()
        fa.nan2bad_device(t.data_ptr(), t.numel(), float(bad), stream)
        torch.cuda.synchronize()
        assert cases.same(t.cpu().numpy(), _f32(c["nan2bad"][k])), "nan2bad, bad value %r" % bad


def test_level_pressures(fa, fx):
    names = fx.names("levels")
    assert len(names) == 3
    for name in names:
        c = fx.case(name)
        nt, ny, nx = c["ps"].shape
        got = fa.vertical_levels_host(ra.levels_of(fa.VerticalLevels, c), nx, ny, nt)
        want = c["out"].view(np.float64).astype(np.float32)
        assert cases.same(got, want), "%s: %s" % (name, cases.describe_mismatch(got, want))
