"""Scaled conversion, theta2T, specific2relative and accumulate / deaccumulate on the GPU (include/fimex_amd.h, 8f n9) through the C ABI,
against tests/derived_ref.py, the CPU restatement that tests/test_derived_ref.py pins, and the recorded answers of
tests/golden/derived_answers.npz.

  scaled conversion         bit for bit (double arithmetic without contraction, lround).
  accumulate, deaccumulate  bit for bit (one double operation per position, in the reference's order).
  theta2T                   |T - T_ref| <= 3 * 2^-23 * |(theta + add_offset) * f|, f the powf factor: the two powf results differ by at
                            most one float ulp if the device rounds a double pow, or two with a <= 1 ulp device powf; then one rounding
                            of the product and one of the subtraction.  NaN positions identical.
  specific2relative         no element differs by more than one count, and at most 1e-4 of the elements differ at all: the device's
                            double exp moves es by one float ulp only when the double result lies within one double ulp of a float
                            rounding boundary, about 2^-29 of the elements, and that shifts 25000 * rh by under 0.005 counts.  Counts
                            are compared as the 16-bit patterns they are, so a result that wrapped is one count from its neighbour.
The shares of bit-identical elements are printed (recorded in DESIGN.md 6.9, not asserted).
"""
import functools

import numpy as np
import pytest

import cases
import derived_ref as dr
import vertical_ref as vr

pytestmark = pytest.mark.gpu

BLOCK = 256        # lanes per workgroup of every kernel here (csrc/common.hpp)
NX, NY = 67, 5     # a plane that is no multiple of the workgroup
GUARD = 32         # bytes kept untouched on either side of an output


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    lib = capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    assert hasattr(lib, "fimex_amd_convert_scaled_device")
    return capi


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dr.load_fixture(golden_dir)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _host(t, dtype, shape=None):
    a = t.cpu().numpy().view(dtype)
    return a if shape is None else a.reshape(shape)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(dr.as_bytes(a), dr.as_bytes(b))


def _same_up_to_nan_payload(a, b):
    """Bit for bit on everything but NaN, whose positions must agree (a CPU and a GPU NaN may differ in sign and payload)."""
    if a.dtype.kind != "f":
        return _same(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(dr.as_bytes(a[~na]), dr.as_bytes(b[~nb]))


def _per_lane(inType, outType):
    """Elements a lane converts per group: 16 bytes of the narrower type (csrc/scaled_convert.hip)."""
    return 16 // min(np.dtype(dr.DTYPES[inType]).itemsize, np.dtype(dr.DTYPES[outType]).itemsize)


def _run_scaled(fa, x, inType, outType, par, shift, in_place=False):
    """The device entry on x placed `shift` elements behind a 16-byte boundary, input and output alike; the bytes around the output must
    stay as they were."""
    import torch
    si, so = x.dtype.itemsize, np.dtype(dr.DTYPES[outType]).itemsize
    src = torch.zeros(x.nbytes + 16 + si, dtype=torch.uint8, device="cuda")
    src[shift * si:shift * si + x.nbytes] = _dev(x)
    if in_place:
        assert si == so
        fa.convert_scaled_device(src.data_ptr() + shift * si, inType, x.size, par[0], par[1], par[2], outType, par[3], par[4], par[5],
                                 src.data_ptr() + shift * si, stream=_stream())
        torch.cuda.synchronize()
        return _host(src[shift * si:shift * si + x.nbytes], dr.DTYPES[outType])
    dst = torch.full((2 * GUARD + x.size * so + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    first = GUARD + shift * so
    fa.convert_scaled_device(src.data_ptr() + shift * si, inType, x.size, par[0], par[1], par[2], outType, par[3], par[4], par[5],
                             dst.data_ptr() + first, stream=_stream())
    torch.cuda.synchronize()
    raw = dst.cpu().numpy()
    assert np.all(raw[:first] == 0xAB) and np.all(raw[first + x.size * so:] == 0xAB), "wrote outside the output"
    return raw[first:first + x.size * so].view(dr.DTYPES[outType])


# ------------------------------------------------------------------ scaled conversion
@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("inType", dr.TYPES)
def test_scaled_conversion_is_bit_identical(fa, inType, variant):
    """Every (IN, OUT) pair at n = 1, 7 and three workgroups of whole groups plus 5, each on 16-byte boundaries and one element behind
    them (the scalar head and tail).  Values: the fill, NaN, +-0, halves, and results past the range of an integer OUT; variant 0 has
    newScale != 1, variant 1 an oldFill that IN cannot hold."""
    for outType in dr.TYPES:
        par = dr.scaled_parameters(inType, outType, variant)
        for n in (1, 7, 3 * BLOCK * _per_lane(inType, outType) + 5):
            x = dr.scaled_values(dr.DTYPES[inType], n, 1000 * variant + 10 * inType + outType, par[0])
            want = dr.convert_scaled(x, par[0], par[1], par[2], outType, par[3], par[4], par[5])
            for shift in (0, 1):
                got = _run_scaled(fa, x, inType, outType, par, shift)
                assert _same_up_to_nan_payload(got, want), (inType, outType, variant, n, shift, int((dr.as_bytes(got) != dr.as_bytes(want)).sum()))


def test_scaled_conversion_hits_what_it_is_meant_to():
    """The generated cases do hold fills, halves and results past the output's range (a check of the test's own input)."""
    par = dr.scaled_parameters(dr.CDM_SHORT, dr.CDM_CHAR, 0)
    x = dr.scaled_values(np.int16, 3 * BLOCK * 16 + 5, 3, par[0])
    d = par[1] / par[4] * x.astype(np.float64) + (par[2] - par[5]) / par[4]
    assert (x == np.int16(par[0])).any() and (np.abs(d - np.trunc(d)) == 0.5).any() and (np.abs(d) > 128).any() and (d < 0).any()
    f = dr.scaled_values(np.float32, 4000, 3, -32767.0)
    assert np.isnan(f).any() and (f == -32767).any() and np.signbit(f[f == 0]).any() and np.isinf(f).any() and (np.abs(f) > 2.0 ** 31).any()
    assert dr.old_fill(dr.scaled_parameters(dr.CDM_SHORT, dr.CDM_FLOAT, 1)[0], np.int16) is None
    assert dr.old_fill(dr.scaled_parameters(dr.CDM_FLOAT, dr.CDM_FLOAT, 1)[0], np.float32) is None
    assert dr.scaled_parameters(dr.CDM_SHORT, dr.CDM_FLOAT, 0)[4] != 1


@pytest.mark.parametrize("pair", [(dr.CDM_SHORT, dr.CDM_FLOAT), (dr.CDM_FLOAT, dr.CDM_SHORT), (dr.CDM_UCHAR, dr.CDM_DOUBLE), (dr.CDM_DOUBLE, dr.CDM_INT64)],
                         ids=lambda p: "%d-%d" % p)
def test_scaled_conversion_strides_over_a_capped_grid(fa, monkeypatch, tuning_build, pair):
    """The grid is capped and strides: with the cap lowered to two workgroups, three workgroups of groups need a second pass."""
    monkeypatch.setenv("FIMEX_AMD_SCALED_MAX_BLOCKS", "2")
    inType, outType = pair
    par = dr.scaled_parameters(inType, outType, 0)
    x = dr.scaled_values(dr.DTYPES[inType], 3 * BLOCK * _per_lane(inType, outType) + 5, 77, par[0])
    want = dr.convert_scaled(x, par[0], par[1], par[2], outType, par[3], par[4], par[5])
    for shift in (0, 1):
        assert _same_up_to_nan_payload(_run_scaled(fa, x, inType, outType, par, shift), want), (pair, shift)


@pytest.mark.parametrize("pair", [(dr.CDM_SHORT, dr.CDM_USHORT), (dr.CDM_FLOAT, dr.CDM_INT), (dr.CDM_INT, dr.CDM_FLOAT), (dr.CDM_DOUBLE, dr.CDM_INT64),
                                  (dr.CDM_UCHAR, dr.CDM_CHAR), (dr.CDM_FLOAT, dr.CDM_FLOAT)], ids=lambda p: "%d-%d" % p)
def test_scaled_conversion_in_place(fa, pair):
    inType, outType = pair
    par = dr.scaled_parameters(inType, outType, 0)
    x = dr.scaled_values(dr.DTYPES[inType], 3 * BLOCK * _per_lane(inType, outType) + 5, 5, par[0])
    want = dr.convert_scaled(x, par[0], par[1], par[2], outType, par[3], par[4], par[5])
    for shift in (0, 1):
        assert _same_up_to_nan_payload(_run_scaled(fa, x, inType, outType, par, shift, in_place=True), want), (pair, shift)


def test_scaled_conversion_recorded_answers(fa, fixture):
    for variant in dr.RECORDED_SCALED_VARIANTS:
        for i in dr.TYPES:
            x = fixture["scaled.in.%d.v%d" % (i, variant)]
            for o in dr.TYPES:
                par = [float(v) for v in fixture["scaled.par.%d.%d.v%d" % (i, o, variant)]]
                want = fixture["scaled.out.%d.%d.v%d" % (i, o, variant)].view(dr.DTYPES[o])
                assert _same_up_to_nan_payload(_run_scaled(fa, x, i, o, par, 0), want), (i, o, variant)


def test_scaled_conversion_refusals(fa):
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    P, n = buf.data_ptr(), 64
    cs = fa.convert_scaled_device

    def raises(match, *a):
        with pytest.raises(fa.FimexAmdError, match=match):
            cs(*a)
    for bad in (dr.CDM_NAT, dr.CDM_STRING, 12, -1):
        raises("data type", P, bad, n, 0.0, 1.0, 0.0, dr.CDM_FLOAT, 0.0, 1.0, 0.0, P + 2048)
        raises("data type", P, dr.CDM_FLOAT, n, 0.0, 1.0, 0.0, bad, 0.0, 1.0, 0.0, P + 2048)
    raises("newFill", P, dr.CDM_FLOAT, n, 0.0, 1.0, 0.0, dr.CDM_SHORT, float("nan"), 1.0, 0.0, P + 2048)
    raises("newFill", P, dr.CDM_FLOAT, n, 0.0, 1.0, 0.0, dr.CDM_SHORT, 32768.0, 1.0, 0.0, P + 2048)
    raises("newFill", P, dr.CDM_FLOAT, n, 0.0, 1.0, 0.0, dr.CDM_UCHAR, -1.0, 1.0, 0.0, P + 2048)
    raises("newFill", P, dr.CDM_FLOAT, n, 0.0, 1.0, 0.0, dr.CDM_UINT64, 2.0 ** 64, 1.0, 0.0, P + 2048)
    raises("newFill", P, dr.CDM_SHORT, n, 0.0, 1.0, 0.0, dr.CDM_FLOAT, 1e39, 1.0, 0.0, P + 2048)
    raises("NULL", None, dr.CDM_FLOAT, n, 0.0, 1.0, 0.0, dr.CDM_SHORT, 0.0, 1.0, 0.0, P)
    raises("NULL", P, dr.CDM_FLOAT, n, 0.0, 1.0, 0.0, dr.CDM_SHORT, 0.0, 1.0, 0.0, None)
    raises("overlaps", P, dr.CDM_FLOAT, n, 0.0, 1.0, 0.0, dr.CDM_SHORT, 0.0, 1.0, 0.0, P)        # in place, sizes differ
    raises("overlaps", P, dr.CDM_SHORT, n, 0.0, 1.0, 0.0, dr.CDM_FLOAT, 0.0, 1.0, 0.0, P)
    raises("overlaps", P, dr.CDM_FLOAT, n, 0.0, 1.0, 0.0, dr.CDM_INT, 0.0, 1.0, 0.0, P + 4)      # same size, shifted
    raises("overlaps", P + 8, dr.CDM_FLOAT, n, 0.0, 1.0, 0.0, dr.CDM_DOUBLE, 0.0, 1.0, 0.0, P)
    # the edge of what an integer newFill may be, and nothing to do, are no errors
    cs(P, dr.CDM_FLOAT, n, 0.0, 1.0, 0.0, dr.CDM_SHORT, -32768.9, 1.0, 0.0, P + 2048)
    cs(P, dr.CDM_FLOAT, n, 0.0, 1.0, 0.0, dr.CDM_CHAR, 127.9, 1.0, 0.0, P + 2048)
    cs(P, dr.CDM_SHORT, n, 0.0, 1.0, 0.0, dr.CDM_FLOAT, float("inf"), 1.0, 0.0, P + 2048)
    cs(None, dr.CDM_FLOAT, 0, 0.0, 1.0, 0.0, dr.CDM_SHORT, 0.0, 1.0, 0.0, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ theta2T and specific2relative
def _fa_levels(fa, lv, device=False):
    keep = []

    def big(v):
        if v is None or not device:
            return v
        t = _dev(v)
        keep.append(t)
        return t.data_ptr()
    out = fa.VerticalLevels(lv.kind, lv.nz, axis=lv.axis, sigma=lv.sigma, a=lv.a, ap=lv.ap, b=lv.b, p0=lv.p0, ptop=lv.ptop,
                            ps=big(lv.ps), field=big(lv.field))
    out._tensors = keep
    return out


@functools.lru_cache(maxsize=None)
def _column_case(kind, nz, nt):
    """(levels, their float32 pressure field, theta, q, T, the restatement's theta2T factor and answers), computed once and shared;
    nobody writes to it."""
    lv = dr.pressure_levels(40 + 10 * kind + nz, kind, NX, NY, nt, nz)
    p = vr.level_field(lv, nt, NY, NX)
    rng = np.random.default_rng(900 + kind + nz)
    theta = rng.uniform(250.0, 700.0, p.shape).astype(np.float32)
    theta[0, nz - 1, 2, 5] = np.nan
    q, T = dr.humidity_inputs(500 + kind + nz, p.shape)
    off = np.float32(273.15)
    with np.errstate(all="ignore"):
        bound = 3 * 2.0 ** -23 * np.abs((theta + off).astype(np.float32).astype(np.float64) * dr.theta_factor(p).astype(np.float64))
    return lv, p, theta, q, T, off, dr.theta_to_temperature(theta, p, off), bound, dr.relative_humidity_short(q, T, p)


def _check_theta(got, want, bound, label):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN positions differ in %d cells" % (label, np.count_nonzero(gn != wn))
    assert wn.any() and not np.isinf(want).any()
    err = np.abs(got[~wn].astype(np.float64) - want[~wn].astype(np.float64))
    same = np.count_nonzero(got[~wn].view(np.uint32) == want[~wn].view(np.uint32))
    print("%s: %d cells, %.4f %% bit-identical, max error / bound %.3f" % (label, err.size, 100.0 * same / err.size, float(np.max(err / bound[~wn]))))
    assert np.all(err <= bound[~wn]), "%s: %d cells over the bound" % (label, np.count_nonzero(err > bound[~wn]))


def _check_humidity(got, want, label):
    """At most one count apart as 16-bit patterns, at most 1e-4 of the elements apart at all."""
    assert got.dtype == want.dtype == np.int16 and got.shape == want.shape
    diff = (got.view(np.uint16) - want.view(np.uint16)).view(np.int16)  # modulo 2^16
    differing = np.count_nonzero(diff)
    print("%s: %d cells, %d differ (%.6f %% bit-identical)" % (label, got.size, differing, 100.0 * (1 - differing / got.size)))
    assert np.all(np.abs(diff.astype(np.int32)) <= 1), "%s: %d cells more than one count apart" % (label, np.count_nonzero(np.abs(diff.astype(np.int32)) > 1))
    assert differing <= 1e-4 * got.size, "%s: %d of %d cells differ" % (label, differing, got.size)
    return differing


@pytest.mark.parametrize("nz", (1, 4, 5, 9))
@pytest.mark.parametrize("kind", vr.KINDS)
def test_theta_to_temperature(fa, kind, nz):
    """Every level kind; nz: a remainder alone, a group of four, both, two groups and a remainder; one and three time steps; NaN in
    theta and in the pressure; out of place and in place."""
    import torch
    for nt in (1, 3):
        lv, p, theta, _, _, off, want, bound, _ = _column_case(kind, nz, nt)
        dl = _fa_levels(fa, lv, device=True)
        d_theta = _dev(theta)
        out = torch.full(theta.shape, -7.0, dtype=torch.float32, device="cuda")
        fa.theta_to_temperature_device(dl, NX, NY, nt, d_theta.data_ptr(), float(off), out.data_ptr(), stream=_stream())
        fa.theta_to_temperature_device(dl, NX, NY, nt, d_theta.data_ptr(), float(off), d_theta.data_ptr(), stream=_stream())  # in place
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        _check_theta(got, want, bound, "theta2T kind %d nz %d nt %d" % (kind, nz, nt))
        assert _same_up_to_nan_payload(_host(d_theta, np.float32, theta.shape), got), "in place differs from out of place"


@pytest.mark.parametrize("nz", (1, 4, 5, 9))
@pytest.mark.parametrize("kind", vr.KINDS)
def test_specific_to_relative_humidity(fa, kind, nz):
    import torch
    for nt in (1, 3):
        lv, p, _, q, T, _, _, _, want = _column_case(kind, nz, nt)
        assert (want == 0).any() and np.isnan(q).any() and np.isnan(T).any() and (kind == vr.AXIS or np.isnan(p).any())
        dl = _fa_levels(fa, lv, device=True)
        d_q, d_T = _dev(q), _dev(T)
        out = torch.full(q.shape, -7, dtype=torch.int16, device="cuda")
        fa.specific_to_relative_humidity_device(dl, NX, NY, nt, d_q.data_ptr(), d_T.data_ptr(), out.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        _check_humidity(out.cpu().numpy(), want, "specific2relative kind %d nz %d nt %d" % (kind, nz, nt))


def _q_for(rh, T):
    """(q, p) in float32 for which the restatement's relative humidity is exactly the float32 rh: rh is monotonic in q, and among a few
    pressures one puts the float32 steps of q closer together than those of rh."""
    es = dr.humidity_es(np.float32(T)).astype(np.float64)
    for p in np.arange(1000.0, 300.0, -50.0, dtype=np.float32):
        q = np.float32(float(rh) * es * dr.MOL_WEIGHT_RATIO / (100.0 * float(p)))
        for _ in range(16):
            got = dr.specific_to_relative(q, np.float32(T), p)
            if got == np.float32(rh):
                return q, p
            q = np.nextafter(q, np.float32(np.inf if got < np.float32(rh) else -np.inf), dtype=np.float32)
    raise AssertionError("no float32 q gives rh = %r" % rh)


def _humidity_on_a_row(fa, q, T, p):
    """The device entry on n points as one level of an n x 1 grid, the pressure as a FIELD."""
    import torch
    d_q, d_T, d_p = _dev(q), _dev(T), _dev(p)
    out = torch.full((q.size,), -7, dtype=torch.int16, device="cuda")
    fa.specific_to_relative_humidity_device(fa.VerticalLevels.from_field(d_p.data_ptr(), 1), q.size, 1, 1, d_q.data_ptr(), d_T.data_ptr(),
                                            out.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_humidity_outside_short(fa, fixture):
    """What a short cannot hold: the low 16 bits of the int32 (rh = 1.4 -> -30536, rh = 3 -> 9464, the clamp at 100 -> 9632), NaN -> 0."""
    T0, p0 = 300.0, 1000.0
    exact = [_q_for(rh, T0) for rh in (1.4, 3.0, 1.0)]
    q = np.array([np.nan, exact[0][0], exact[1][0], 5.0, 0.01, 0.01, 0.0, exact[2][0]], np.float32)
    T = np.array([T0, T0, T0, T0, np.nan, T0, T0, T0], np.float32)
    p = np.array([p0, exact[0][1], exact[1][1], p0, p0, np.nan, p0, exact[2][1]], np.float32)
    want = dr.relative_humidity_short(q, T, p)
    assert np.array_equal(want, np.array([0, -30536, 9464, 9632, 0, 0, 0, 25000], np.int16))
    got = _humidity_on_a_row(fa, q, T, p)
    assert np.array_equal(got.reshape(-1), want), got
    # the recorded inputs, answered by the reference's object code
    rq, rt, rp = fixture["humidity.q"], fixture["humidity.t"], fixture["humidity.p"]
    got = _humidity_on_a_row(fa, rq, rt, rp)
    _check_humidity(got.reshape(-1), fixture["humidity.packed"], "specific2relative against the recorded answers of the reference's object code")


def test_pressure_conversion_refusals(fa):
    import torch
    nx, ny, nz, nt = 8, 4, 3, 1
    vol = torch.zeros((nt, nz, ny, nx), dtype=torch.float32, device="cuda")
    other = torch.zeros_like(vol)
    sh = torch.zeros((nt, nz, ny, nx), dtype=torch.int16, device="cuda")
    V, O, S = vol.data_ptr(), other.data_ptr(), sh.data_ptr()
    axis = fa.VerticalLevels.from_axis(np.array([100.0, 500.0, 900.0]))

    def raises(match, fn, *a):
        with pytest.raises(fa.FimexAmdError, match=match):
            fn(*a)
    th, hu = fa.theta_to_temperature_device, fa.specific_to_relative_humidity_device
    raises("potential temperature", th, axis, nx, ny, nt, None, 0.0, O)
    raises("output", th, axis, nx, ny, nt, V, 0.0, None)
    raises("overlaps theta", th, axis, nx, ny, nt, V, 0.0, V + 4)
    raises("overlaps the level field", th, fa.VerticalLevels.from_field(O, nz), nx, ny, nt, V, 0.0, O)
    raises("nz == 0", th, fa.VerticalLevels.from_axis(np.zeros(0)), nx, ny, nt, V, 0.0, O)
    raises("unknown vertical level kind", th, fa.VerticalLevels(9, nz), nx, ny, nt, V, 0.0, O)
    raises("specific humidity", hu, axis, nx, ny, nt, None, V, S)
    raises("air temperature", hu, axis, nx, ny, nt, V, None, S)
    raises("output", hu, axis, nx, ny, nt, V, O, None)
    raises("overlaps the specific humidity", hu, axis, nx, ny, nt, V, O, V)
    raises("overlaps the air temperature", hu, axis, nx, ny, nt, V, O, O + 2)
    th(axis, 0, ny, nt, None, 0.0, None)  # nothing to do is no error
    hu(axis, nx, ny, 0, None, None, None)


# ------------------------------------------------------------------ accumulate / deaccumulate
ACC_N = 2 * BLOCK * 1 + 3  # a lane owns one cell: two workgroups and a remainder


def _run_along_time(fa, which, x, firstPos, prev):
    import torch
    code = fa.cdm_type_of(x.dtype)
    nt, n = x.shape
    d_in = _dev(x)
    d_prev = _dev(prev) if prev is not None else None
    out = torch.full((nt * n + 2 * GUARD // 8,), -7.0, dtype=torch.float64, device="cuda")
    fn = fa.accumulate_device if which == "acc" else fa.deaccumulate_device
    fn(d_in.data_ptr(), code, n, nt, firstPos, d_prev.data_ptr() if d_prev is not None else None, out.data_ptr() + GUARD, stream=_stream())
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert np.all(raw[:GUARD // 8] == -7.0) and np.all(raw[GUARD // 8 + nt * n:] == -7.0), "wrote outside the output"
    return raw[GUARD // 8:GUARD // 8 + nt * n].reshape(nt, n)


@pytest.mark.parametrize("code", dr.RECORDED_ACCUMULATE_TYPES)
@pytest.mark.parametrize("nt", (1, 2, 5))
def test_accumulate_and_deaccumulate_are_bit_identical(fa, nt, code):
    """A whole batch from position 0, batches that start at positions 1 and 3 with the carry, and the whole batch split in two."""
    total = nt + 3
    x = dr.accumulate_input(60 + code + nt, dr.DTYPES[code], total, ACC_N)
    assert x.dtype.kind != "f" or (np.isnan(x[0]).any() and np.isnan(x[1:]).any())
    acc, de = dr.accumulate(x), dr.deaccumulate(x)
    for first in (0, 1, 3):
        part = x[first:first + nt]
        prev_acc = acc[first - 1] if first else None
        prev_de = x[first - 1] if first else None
        got = _run_along_time(fa, "acc", part, first, prev_acc)
        assert _same_up_to_nan_payload(got, acc[first:first + nt]), ("accumulate", code, nt, first)
        got = _run_along_time(fa, "de", part, first, prev_de)
        assert _same_up_to_nan_payload(got, de[first:first + nt]), ("deaccumulate", code, nt, first)
    for split in range(1, nt):  # the carry of the first half makes the second half what the whole batch gives
        whole = _run_along_time(fa, "acc", x[:nt], 0, None)
        head = _run_along_time(fa, "acc", x[:split], 0, None)
        tail = _run_along_time(fa, "acc", x[split:nt], split, head[-1])
        assert _same(np.concatenate([head, tail]), whole), ("accumulate split", code, nt, split)
        whole = _run_along_time(fa, "de", x[:nt], 0, None)
        tail = _run_along_time(fa, "de", x[split:nt], split, x[split - 1])
        assert _same(np.concatenate([whole[:split], tail]), whole), ("deaccumulate split", code, nt, split)


def test_accumulate_recorded_answers(fa, fixture):
    for code in dr.RECORDED_ACCUMULATE_TYPES:
        x = fixture["accumulate.%d.in" % code]
        assert _same_up_to_nan_payload(_run_along_time(fa, "acc", x, 0, None), fixture["accumulate.%d.acc" % code].view(np.float64))
        assert _same_up_to_nan_payload(_run_along_time(fa, "de", x, 0, None), fixture["accumulate.%d.deacc" % code].view(np.float64))


def test_accumulate_refusals(fa):
    import torch
    buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    P, n, nt = buf.data_ptr(), 16, 2
    for fn in (fa.accumulate_device, fa.deaccumulate_device):
        for first in (1, 3):
            with pytest.raises(fa.FimexAmdError, match="needs prev"):
                fn(P, dr.CDM_FLOAT, n, nt, first, None, P + 4096)
        with pytest.raises(fa.FimexAmdError, match="data type"):
            fn(P, dr.CDM_STRING, n, nt, 0, None, P + 4096)
        with pytest.raises(fa.FimexAmdError, match="NULL"):
            fn(P, dr.CDM_FLOAT, n, nt, 0, None, None)
        with pytest.raises(fa.FimexAmdError, match="overlaps the input"):
            fn(P, dr.CDM_DOUBLE, n, nt, 0, None, P + 8)
        with pytest.raises(fa.FimexAmdError, match="overlaps prev"):
            fn(P, dr.CDM_DOUBLE, n, nt, 1, P + 4096, P + 4096)
        fn(P, dr.CDM_FLOAT, n, nt, 0, P + 4096, P + 4096)  # prev is ignored at position 0
        fn(None, dr.CDM_FLOAT, 0, nt, 1, None, None)       # nothing to do is no error
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the chain
def test_packed_model_levels_to_regridded_relative_humidity(fa):
    """Packed-short T and q with scale and offset, float ps, hybrid levels -> two scaled conversions to float -> specific2relative to
    shorts -> fimex_amd_regrid_apply_typed_device(CDM_SHORT) on a small bilinear plan: nothing leaves the device in between."""
    import oracle
    import torch
    nz, nt, outX, outY = 9, 1, 23, 4
    lv = dr.pressure_levels(321, vr.HYBRID_SIGMA_AP, NX, NY, nt, nz)
    p = vr.level_field(lv, nt, NY, NX)
    rng = np.random.default_rng(322)
    t_fill, q_fill = -32767.0, -32767.0
    t_packed = rng.integers(-7300, 4700, p.shape).astype(np.int16)   # 0.01 K steps around 273.15 K: 200 to 320 K
    q_packed = rng.integers(0, 30000, p.shape).astype(np.int16)     # 1e-6 steps: 0 to 0.03
    t_packed[0, 3, 2, 7] = np.int16(t_fill)
    q_packed[0, 5, 1, 9] = np.int16(q_fill)
    t_par = (t_fill, 0.01, 273.15, dr.CDM_FLOAT, np.nan, 1.0, 0.0)
    q_par = (q_fill, 1e-6, 0.0, dr.CDM_FLOAT, np.nan, 1.0, 0.0)
    T, q = dr.convert_scaled(t_packed, *t_par), dr.convert_scaled(q_packed, *q_par)
    want_rh = dr.relative_humidity_short(q, T, p)
    px, py = cases.backward_positions(NX, NY, outX, outY, seed=4)
    rh_fill = -32767.0

    def regrid(rh):
        fl = oracle.interpolate_values(oracle.BILINEAR, px, py, oracle.data2interpolation_array(rh.reshape(nz, NY, NX), rh_fill), NX, NY, outX, outY)
        return oracle.interpolation_array2data(fl, oracle.cdm_type_of(np.int16), rh_fill)
    plan = fa.RegridPlan(fa.BILINEAR, px, py, NX, NY, outX, outY)
    dl = _fa_levels(fa, lv, device=True)
    d_tp, d_qp = _dev(t_packed), _dev(q_packed)
    d_T = torch.empty(p.shape, dtype=torch.float32, device="cuda")
    d_q = torch.empty_like(d_T)
    d_rh = torch.empty(p.shape, dtype=torch.int16, device="cuda")
    d_out = torch.empty((nz, outY, outX), dtype=torch.int16, device="cuda")
    st = _stream()
    fa.convert_scaled_device(d_tp.data_ptr(), dr.CDM_SHORT, p.size, *t_par, d_T.data_ptr(), stream=st)
    fa.convert_scaled_device(d_qp.data_ptr(), dr.CDM_SHORT, p.size, *q_par, d_q.data_ptr(), stream=st)
    fa.specific_to_relative_humidity_device(dl, NX, NY, nt, d_q.data_ptr(), d_T.data_ptr(), d_rh.data_ptr(), stream=st)
    fa.regrid_apply_typed_device(plan, d_rh.data_ptr(), dr.CDM_SHORT, nz, rh_fill, d_out.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert _same_up_to_nan_payload(d_T.cpu().numpy(), T) and _same_up_to_nan_payload(d_q.cpu().numpy(), q)
    got_rh = d_rh.cpu().numpy()
    _check_humidity(got_rh, want_rh, "chain, specific2relative")
    # 3015 cells: the cap of 1e-4 of them leaves room for none to differ, so the whole chain is the restatement's, cell for cell
    assert np.array_equal(got_rh, want_rh)
    assert np.array_equal(d_out.cpu().numpy(), regrid(want_rh).reshape(nz, outY, outX))
    plan.close()


# ------------------------------------------------------------------ host entries
def test_host_entries_equal_their_device_twins(fa):
    import torch
    # scaled conversion
    par = dr.scaled_parameters(dr.CDM_SHORT, dr.CDM_FLOAT, 0)
    x = dr.scaled_values(np.int16, 1000, 8, par[0])
    copy = x.copy()
    host = fa.convert_scaled_host(x, par[0], par[1], par[2], dr.CDM_FLOAT, par[3], par[4], par[5])
    assert np.array_equal(x, copy) and _same(host, _run_scaled(fa, x, dr.CDM_SHORT, dr.CDM_FLOAT, par, 0).reshape(host.shape))
    # theta2T and specific2relative
    nz, nt = 5, 3
    lv, p, theta, q, T, off, _, _, _ = _column_case(vr.HYBRID_SIGMA, nz, nt)
    dl = _fa_levels(fa, lv, device=True)
    d_theta, d_q, d_T = _dev(theta), _dev(q), _dev(T)
    out = torch.empty(theta.shape, dtype=torch.float32, device="cuda")
    fa.theta_to_temperature_device(dl, NX, NY, nt, d_theta.data_ptr(), float(off), out.data_ptr(), stream=_stream())
    rh = torch.empty(theta.shape, dtype=torch.int16, device="cuda")
    fa.specific_to_relative_humidity_device(dl, NX, NY, nt, d_q.data_ptr(), d_T.data_ptr(), rh.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    copies = (theta.copy(), q.copy(), T.copy())
    assert _same(fa.theta_to_temperature_host(_fa_levels(fa, lv), NX, NY, nt, theta, float(off)), out.cpu().numpy())
    assert _same(fa.specific_to_relative_humidity_host(_fa_levels(fa, lv), NX, NY, nt, q, T), rh.cpu().numpy())
    assert all(_same(a, b) for a, b in zip((theta, q, T), copies)), "a host entry changed its input"
    # accumulate and deaccumulate, with a carry
    x = dr.accumulate_input(9, np.float32, 4, ACC_N)
    prev = dr.accumulate(x[:1])[0]
    assert _same(fa.accumulate_host(x[1:], 1, prev), _run_along_time(fa, "acc", x[1:], 1, prev))
    assert _same(fa.deaccumulate_host(x[1:], 1, x[0]), _run_along_time(fa, "de", x[1:], 1, x[0]))
    assert _same(fa.accumulate_host(x), _run_along_time(fa, "acc", x, 0, None))
    # in place on the host, for types of one size
    y = x[0].copy()
    want = fa.convert_scaled_host(y, np.nan, 2.0, 1.0, dr.CDM_INT, -1.0)
    lib = fa.load()
    assert lib.fimex_amd_convert_scaled_host(y.ctypes.data, dr.CDM_FLOAT, y.size, np.nan, 2.0, 1.0, dr.CDM_INT, -1.0, 1.0, 0.0, y.ctypes.data) == fa.OK
    assert _same(y.view(np.int32), want)


def test_empty_host_calls_do_nothing(fa):
    """n == 0 (or nt == 0) with NULL wherever the checks allow NULL, and a live output pointer: OK, nothing written; the refusals of
    the device forms come from the same checks."""
    import ctypes
    lib = fa.load()
    levels = ctypes.byref(fa.VerticalLevels.from_axis([1., 2.]).struct)
    out = np.full(8, 0xA5, np.uint8)
    o = out.ctypes.data
    nan = float("nan")
    calls = {
        "fimex_amd_convert_scaled_host": (None, dr.CDM_SHORT, 0, -32767.0, 0.01, 273.15, dr.CDM_FLOAT, nan, 1.0, 0.0, o),
        "fimex_amd_theta_to_temperature_host": (levels, 4, 3, 0, None, 0.0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))),
        "fimex_amd_specific_to_relative_humidity_host": (levels, 4, 3, 0, None, None, o),
        "fimex_amd_accumulate_host": (None, dr.CDM_SHORT, 0, 2, 1, None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
        "fimex_amd_deaccumulate_host": (None, dr.CDM_SHORT, 4, 0, 0, None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
    }
    assert set(calls) == set(fa.DERIVED_HOST_SYMBOLS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == fa.OK, "%s: %s" % (name, lib.fimex_amd_last_error().decode())
        assert np.all(out == 0xA5), "%s wrote to an array" % name
    x = np.zeros((2, 4), np.float32)
    with pytest.raises(fa.FimexAmdError, match="needs prev"):
        fa.accumulate_host(x, 1)
    with pytest.raises(fa.FimexAmdError, match="newFill"):
        fa.convert_scaled_host(x, 0.0, 1.0, 0.0, dr.CDM_SHORT, nan)
    assert lib.fimex_amd_convert_scaled_host(None, dr.CDM_FLOAT, 4, 0.0, 1.0, 0.0, dr.CDM_SHORT, 0.0, 1.0, 0.0, o) == fa.ERROR
    assert b"NULL" in lib.fimex_amd_last_error() and np.all(out == 0xA5)
