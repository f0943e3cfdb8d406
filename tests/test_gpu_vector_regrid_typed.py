"""fimex_amd_regrid_apply_vector_typed_device / _host: both components of a vector pair in their stored types regridded, rotated
and packed again in one call (CDMInterpolator::getDataSlice's vector branch, src/CDMInterpolator.cc:251-285, without pre- and
post-processes).  The expected result everywhere is the CPU chain of the oracle: data2interpolation_array and interpolate_values on
u and on v, vector_reproject_values, interpolation_array2data per component with its own type and fill value; compared element for
element with np.array_equal.  With a NaN fill value the cells whose rotated value is NaN are left out ((T)NaN is undefined in C).

The dispatch rule under test, `_fused`: the kernel on the stored type runs (path 2) exactly when both components
are short or both unsigned short, the method is nearest or bilinear, the source slice is a multiple of 4 bytes and the plan tiles
(stagedCells > 0), both source pointers are 4-byte aligned and the batch has four pairs or more; everything else takes the chain of
five launches around the float pair entry (path 1 or 0).

Every case asserts, before it compares, that it compares data: enough cells defined in both components, cells that are defined
in one regridded component only (fill values in both outputs), rotated values beyond the type's range (the reference's casts
wrap them) and rotated values half-way between two integers (lround's tie rule)."""
import functools

import numpy as np
import pytest

import cases
import oracle

pytestmark = pytest.mark.gpu

MIN_NZ = 4  # STAGED_MIN_NZ
METHODS = [oracle.NEAREST, oracle.BILINEAR]
METHOD_IDS = ["nearest", "bilinear"]
FLOAT_BAD = (-999.0, 999.0)  # fill values of the floating-point components: values that the data take


def _scattered():
    rng = np.random.default_rng(5)  # the scattered plan of test_gpu_vector_regrid.py
    return rng.uniform(-3, 512 + 2, 200 * 100), rng.uniform(-3, 384 + 2, 200 * 100)


# (inX, inY, outY) and the positions for an output row length outX
GEOMETRY = {
    # overshoots the source (undefined cells, all bilinear border forms); outX 212: pair stores, 213 and 77: single stores
    "E": ((336, 97, 45), lambda outX: cases.backward_positions(336, 97, outX, 45, seed=outX)),
    # staged tiles and gather tiles; an even source slice, so the 2-byte form exists
    "A2": ((404, 301, 77), lambda outX: cases.coherent_positions(404, 301, outX, 77, seed=21, outliers=3)),
    # an odd number of source cells: no 2-byte form
    "A": ((403, 301, 77), lambda outX: cases.coherent_positions(403, 301, outX, 77, seed=21, outliers=3)),
    "coord": ((300, 200, 211), lambda outX: cases.backward_positions(300, 200, outX, 211, seed=100 + oracle.COORD_NN)),
    "C": ((512, 384, 100), lambda outX: _scattered()),
}
A2_OUTX = 130


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


@functools.lru_cache(maxsize=None)
def _positions(geometry, outX):
    return GEOMETRY[geometry][1](outX)


def _component(rng, dt, shape, full):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return rng.integers(-3000, 3001, shape).astype(dt)
    info = np.iinfo(dt)
    lo, hi = (int(info.min), int(info.max)) if full else (max(int(info.min), -3000), min(int(info.max), 3000))
    return rng.integers(lo, hi + 1, shape).astype(dt)


def _bad_values(dtU, dtV, fill):
    """uBad: the type's minimum, vBad: the type's maximum; NaN: no fill value at all."""
    if fill == "nan":
        return float("nan"), float("nan")
    if fill is None:
        return None, None
    dtU, dtV = np.dtype(dtU), np.dtype(dtV)
    return (FLOAT_BAD[0] if dtU.kind == "f" else float(np.iinfo(dtU).min)), (FLOAT_BAD[1] if dtV.kind == "f" else float(np.iinfo(dtV).max))


@functools.lru_cache(maxsize=None)
def _case(geometry, outX, method, nz, dtU, dtV, full, fill):
    """Inputs and the oracle's results, computed once per case and never written to.  fill: "ends" (uBad the type's minimum, vBad
    its maximum, 3 % of the elements each), "nan" (no fill value)."""
    inX, inY, outY = GEOMETRY[geometry][0]
    px, py = _positions(geometry, outX)
    rng = np.random.default_rng(outX + nz)
    u = _component(rng, dtU, (nz, inY, inX), full)
    v = _component(rng, dtV, (nz, inY, inX), full)
    uBad, vBad = _bad_values(dtU, dtV, fill)
    if fill == "ends":
        u.reshape(-1)[rng.random(u.size) < 0.03] = np.dtype(dtU).type(uBad)
        v.reshape(-1)[rng.random(v.size) < 0.03] = np.dtype(dtV).type(vBad)
    m = cases.rotation_matrix(outX, outY, seed=outX)
    ru = oracle.interpolate_values(method, px, py, oracle.data2interpolation_array(u, uBad), inX, inY, outX, outY)
    rv = oracle.interpolate_values(method, px, py, oracle.data2interpolation_array(v, vBad), inX, inY, outX, outY)
    wu, wv = oracle.vector_reproject_values(m, ru, rv, outX, outY)
    wantU = oracle.interpolation_array2data(wu, oracle.cdm_type_of(dtU), uBad)
    wantV = oracle.interpolation_array2data(wv, oracle.cdm_type_of(dtV), vBad)
    # without a fill value an undefined result becomes (T)NaN, which C leaves undefined: those cells are not compared
    cmpU = ~np.isnan(wu) if fill == "nan" else np.ones(wu.shape, bool)
    cmpV = ~np.isnan(wv) if fill == "nan" else np.ones(wv.shape, bool)
    both = ~np.isnan(wu) & ~np.isnan(wv)
    stats = {"both": float(both.mean()), "one": int(np.count_nonzero(np.isnan(ru) ^ np.isnan(rv))), "wrapped": 0, "ties": 0}
    for w, dt in ((wu, dtU), (wv, dtV)):
        if np.dtype(dt).kind != "f":
            d = w[~np.isnan(w)].astype(np.float64)
            stats["wrapped"] += int(np.count_nonzero((np.round(d) < np.iinfo(dt).min) | (np.round(d) > np.iinfo(dt).max)))
            stats["ties"] += int(np.count_nonzero(np.abs(d - np.trunc(d)) == 0.5))
    for a in (u, v, wantU, wantV, cmpU, cmpV):
        a.setflags(write=False)
    return {"geometry": geometry, "outX": outX, "outY": outY, "inX": inX, "inY": inY, "method": method, "nz": nz, "u": u, "v": v,
            "uBad": uBad, "vBad": vBad, "wantU": wantU, "wantV": wantV, "cmpU": cmpU, "cmpV": cmpV, "stats": stats, "full": full,
            "fill": fill}


def _assert_caps(c):
    """A comparison of mostly fill values shows nothing: the caps that the oracle's results of this case have to meet."""
    s = c["stats"]
    if c["fill"] == "ends":
        assert s["both"] >= 0.6, s
        assert s["one"] >= 1, s
    if c["full"]:
        assert s["wrapped"] >= 1, s
    # (a float of this size has 12 or 13 fraction bits left, so about one rotated value in 5 000 is a tie: a batch of fewer
    # than five pairs of the smaller geometry may hold none)
    if c["nz"] >= 5:
        assert s["ties"] >= 1, s


def _plans(fa, c):
    px, py = _positions(c["geometry"], c["outX"])
    plan = fa.RegridPlan(c["method"], px, py, c["inX"], c["inY"], c["outX"], c["outY"])
    vec = fa.VectorPlan(cases.rotation_matrix(c["outX"], c["outY"], seed=c["outX"]), c["outX"], c["outY"])
    return plan, vec


def _fused(plan, c, shifts=(0, 0, 0, 0)):
    """The dispatch rule: see the module's docstring."""
    dtU, dtV = c["u"].dtype, c["v"].dtype
    return (dtU == dtV and dtU in (np.dtype(np.int16), np.dtype(np.uint16)) and c["method"] in METHODS and (c["inX"] * c["inY"] * 2) % 4 == 0
            and plan.info()["stagedCells"] > 0 and shifts[0] % 4 == 0 and shifts[1] % 4 == 0 and c["nz"] >= MIN_NZ)


class _Buffers:
    """The four device buffers of a call, each `shift` bytes into an allocation of its own; the outputs pre-filled with 0x07."""

    def __init__(self, c, shifts=(0, 0, 0, 0)):
        import torch
        self.c, self.shifts = c, shifts
        self.t = []
        for a, shift in ((c["u"], shifts[0]), (c["v"], shifts[1])):
            t = torch.zeros(a.nbytes + 16, dtype=torch.uint8, device="cuda")
            t[shift:shift + a.nbytes] = torch.from_numpy(np.array(a).view(np.uint8).reshape(-1)).cuda()
            self.t.append(t)
        for a, shift in ((c["wantU"], shifts[2]), (c["wantV"], shifts[3])):
            self.t.append(torch.full((a.nbytes + 16,), 7, dtype=torch.uint8, device="cuda"))
        self.ptr = [t.data_ptr() + s for t, s in zip(self.t, shifts)]
        assert all(t.data_ptr() % 16 == 0 for t in self.t)

    def result(self, k):
        want = self.c["wantU"] if k == 0 else self.c["wantV"]
        raw = self.t[2 + k].cpu().numpy()
        s = self.shifts[2 + k]
        assert (raw[:s] == 7).all() and (raw[s + want.nbytes:] == 7).all(), "bytes outside the output were written"
        return raw[s:s + want.nbytes].view(want.dtype).reshape(want.shape)


def _apply(fa, plan, vec, c, shifts=(0, 0, 0, 0), stream=None):
    """The entry on fresh buffers; returns (path, buffers), the results still on the device."""
    import torch
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        b = _Buffers(c, shifts)
        path = plan.apply_vector_typed_device(vec, b.ptr[0], oracle.cdm_type_of(c["u"].dtype), c["uBad"], b.ptr[1], oracle.cdm_type_of(c["v"].dtype),
                                              c["vBad"], c["nz"], b.ptr[2], b.ptr[3], st.cuda_stream)
    return path, b


def _chain(fa, plan, vec, c):
    """The five existing device launches on the same inputs."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    b = _Buffers(c)
    nIn, nOut = c["u"].size, c["wantU"].size
    fu, fv = torch.empty(nIn, device="cuda"), torch.empty(nIn, device="cuda")
    fuo, fvo = torch.empty(nOut, device="cuda"), torch.empty(nOut, device="cuda")
    codeU, codeV = oracle.cdm_type_of(c["u"].dtype), oracle.cdm_type_of(c["v"].dtype)
    fa.data2interpolation_device(b.ptr[0], codeU, nIn, c["uBad"], fu.data_ptr(), st)
    fa.data2interpolation_device(b.ptr[1], codeV, nIn, c["vBad"], fv.data_ptr(), st)
    plan.apply_vector_device(vec, fu.data_ptr(), fv.data_ptr(), c["nz"], fuo.data_ptr(), fvo.data_ptr(), st)
    fa.interpolation2data_device(fuo.data_ptr(), nOut, codeU, c["uBad"], b.ptr[2], st)
    fa.interpolation2data_device(fvo.data_ptr(), nOut, codeV, c["vBad"], b.ptr[3], st)
    torch.cuda.synchronize()
    return b.result(0), b.result(1)


def _check(got, want, defined, what):
    bad = (got != want) & defined
    assert got.dtype == want.dtype and not bad.any(), "%s%d of %d differ; first: %s" % (
        what, int(bad.sum()), got.size, [(int(i), int(got.reshape(-1)[i]), int(want.reshape(-1)[i])) for i in np.nonzero(bad.reshape(-1))[0][:5]])
    assert np.array_equal(got[defined], want[defined])


def _run_and_check(fa, c, against_chain=False, shifts=(0, 0, 0, 0)):
    import torch
    plan, vec = _plans(fa, c)
    path, b = _apply(fa, plan, vec, c, shifts)
    torch.cuda.synchronize()
    gu, gv = b.result(0), b.result(1)
    _check(gu, c["wantU"], c["cmpU"], "u: ")
    _check(gv, c["wantV"], c["cmpV"], "v: ")
    if against_chain:
        cu, cv = _chain(fa, plan, vec, c)
        _check(gu, cu, c["cmpU"], "u against the device chain: ")
        _check(gv, cv, c["cmpV"], "v against the device chain: ")
    return path, plan


def _a2(method, nz, dt=np.int16, full=False, fill="ends"):
    return _case("A2", A2_OUTX, method, nz, np.dtype(dt), np.dtype(dt), full, fill)


# ---- 1. parity and path

@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("dt", [np.int16, np.uint16], ids=["short", "ushort"])
@pytest.mark.parametrize("outX", [212, 213, 77])
def test_parity_on_even_and_odd_rows(fa, method, dt, outX):
    """Geometry E, full-range data with fill values: even rows give pair stores, odd rows single stores with pairs that straddle
    rows."""
    c = _case("E", outX, method, 9, np.dtype(dt), np.dtype(dt), True, "ends")
    _assert_caps(c)
    path, plan = _run_and_check(fa, c, against_chain=True)
    assert _fused(plan, c) and path == 2


@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("dt,full,fill", [(np.int16, False, "ends"), (np.uint16, False, "ends"), (np.uint16, True, "ends"),
                                          (np.int16, False, "nan"), (np.uint16, False, "nan")],
                         ids=["short", "ushort", "ushort_full_range", "short_nan_fill", "ushort_nan_fill"])
def test_parity_on_staged_and_gather_tiles(fa, method, dt, full, fill):
    c = _a2(method, 5, dt, full, fill)
    _assert_caps(c)
    path, plan = _run_and_check(fa, c, against_chain=True)
    assert _fused(plan, c) and path == 2


@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("nz", [1, 3, 4, 9])
def test_batch_lengths(fa, method, nz):
    """Below the threshold, the threshold, odd counts (5 pairs: test_parity_on_staged_and_gather_tiles)."""
    c = _a2(method, nz)
    _assert_caps(c)
    path, plan = _run_and_check(fa, c, against_chain=True)
    assert plan.info()["stagedCells"] > 0, "the plan lost its staged form"
    assert (path == 2) == bool(_fused(plan, c)) and (path == 2) == (nz >= MIN_NZ)


def test_z_chunks_of_uneven_length(fa):
    """26 pairs: four z chunks of 7, 7, 6 and 6 pairs."""
    c = _a2(oracle.BILINEAR, 26)
    _assert_caps(c)
    path, _ = _run_and_check(fa, c, against_chain=True)
    assert path == 2


# ---- 2. pointers that are not 4-byte aligned

@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("shifts", [(0, 0, 2, 0), (0, 0, 0, 2), (0, 0, 2, 2), (2, 0, 0, 0), (0, 2, 0, 0)],
                         ids=["uOut", "vOut", "both_outputs", "u", "v"])
def test_pointers_off_by_one_element(fa, method, shifts):
    """An output off by one element: single stores, the same bytes.  A source off by one element: the chain, the same bytes."""
    c = _a2(method, 5)
    path, plan = _run_and_check(fa, c, shifts=shifts)
    assert (path == 2) == (shifts[0] == 0 and shifts[1] == 0) and (path == 2) == bool(_fused(plan, c, shifts))


# ---- 3. fallbacks

@pytest.mark.parametrize("dtU,dtV", [(np.int16, np.uint16), (np.int16, np.float32), (np.int8, np.int8), (np.int32, np.int32),
                                     (np.float32, np.float32), (np.float64, np.float64)],
                         ids=["short_ushort", "short_float", "int8", "int32", "float32", "float64"])
def test_other_types_take_the_chain(fa, dtU, dtV):
    c = _case("A2", A2_OUTX, oracle.BILINEAR, 5, np.dtype(dtU), np.dtype(dtV), False, "ends")
    assert c["stats"]["both"] >= 0.6 and c["stats"]["one"] >= 1
    path, plan = _run_and_check(fa, c, against_chain=True)
    assert not _fused(plan, c) and path in (0, 1)


@pytest.mark.parametrize("geometry,outX,method", [("A2", A2_OUTX, oracle.BICUBIC), ("coord", 157, oracle.COORD_NN), ("A", 130, oracle.BILINEAR),
                                                  ("A", 130, oracle.NEAREST), ("C", 200, oracle.BILINEAR), ("C", 200, oracle.NEAREST)],
                         ids=["bicubic", "coord_nn", "no_2_byte_form_bilinear", "no_2_byte_form_nearest", "scattered_bilinear",
                              "scattered_nearest"])
def test_other_plans_take_the_chain(fa, geometry, outX, method):
    c = _case(geometry, outX, method, 5, np.dtype(np.int16), np.dtype(np.int16), False, "ends")
    path, plan = _run_and_check(fa, c)
    assert path in (0, 1)
    if geometry == "C":
        assert plan.info()["stagedCells"] == 0
    else:
        assert not _fused(plan, c)


# ---- 4. ring variants

@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
@pytest.mark.parametrize("knob,value", [("STAGE2T_DEPTH", "3"), ("STAGE2T_NT", "256"), ("STAGE2T_NT", "1024"), ("STAGE2T_ZPB", "1"),
                                        ("STAGE2T_ZPB", "2"), ("STAGE2T_PAIR", "0"), ("VECTOR_FUSED", "0"), ("TYPED_STAGED2", "0")])
def test_ring_variants(fa, monkeypatch, tuning_build, method, knob, value):
    """The three-slot ring, the other workgroup shapes, chunks of one and two pairs (the loop's head and tail with nothing in
    between), single stores on even rows, and the switches that send everything to the chain."""
    monkeypatch.setenv("FIMEX_AMD_" + knob, value)
    c = _a2(method, 9)
    path, plan = _run_and_check(fa, c)
    assert plan.info()["stagedCells"] > 0
    if knob in ("VECTOR_FUSED", "TYPED_STAGED2"):
        assert path in (0, 1)
    else:
        assert path == 2


# ---- 5. to 8.

def test_repeatable_on_the_same_plan_and_buffers(fa):
    """A wrong wait count shows here as a mismatch: the same plan and buffers 20 times, allocations of other sizes in between."""
    import torch
    c = _a2(oracle.BILINEAR, 6)
    plan, vec = _plans(fa, c)
    st = torch.cuda.current_stream().cuda_stream
    b = _Buffers(c)
    code = oracle.cdm_type_of(np.int16)
    rng = np.random.default_rng(5)
    junk = []
    for it in range(20):
        junk.append(torch.empty(int(rng.integers(1, 64)) * 262144, device="cuda").normal_())
        if len(junk) > 6:
            junk.pop(0)
        b.t[2].fill_(7)
        b.t[3].fill_(7)
        assert plan.apply_vector_typed_device(vec, b.ptr[0], code, c["uBad"], b.ptr[1], code, c["vBad"], c["nz"], b.ptr[2], b.ptr[3], st) == 2
        torch.cuda.synchronize()
        _check(b.result(0), c["wantU"], c["cmpU"], "iteration %d, u: " % it)
        _check(b.result(1), c["wantV"], c["cmpV"], "iteration %d, v: " % it)


def test_one_plan_on_two_streams(fa):
    import torch
    c = _a2(oracle.BILINEAR, 6)
    plan, vec = _plans(fa, c)
    torch.cuda.synchronize()
    runs = [_apply(fa, plan, vec, c, stream=torch.cuda.Stream()) for _ in range(2)]
    torch.cuda.synchronize()
    for path, b in runs:
        assert path == 2
        _check(b.result(0), c["wantU"], c["cmpU"], "u: ")
        _check(b.result(1), c["wantV"], c["cmpV"], "v: ")


@pytest.mark.parametrize("dtU,dtV", [(np.int16, np.int16), (np.uint16, np.float32)], ids=["short", "ushort_float"])
def test_host_form_equals_the_device_form(fa, dtU, dtV):
    import torch
    c = _case("A2", A2_OUTX, oracle.BILINEAR, 5, np.dtype(dtU), np.dtype(dtV), False, "ends")
    plan, vec = _plans(fa, c)
    hu, hv = plan.apply_vector_typed_host(vec, c["u"], c["uBad"], c["v"], c["vBad"])
    path, b = _apply(fa, plan, vec, c)
    torch.cuda.synchronize()
    assert (path == 2) == (dtU == dtV) and hu.shape == hv.shape == (c["nz"], plan.outY, plan.outX)
    assert hu.dtype == np.dtype(dtU) and hv.dtype == np.dtype(dtV)
    _check(hu, b.result(0), c["cmpU"], "u against the device form: ")
    _check(hv, b.result(1), c["cmpV"], "v against the device form: ")
    _check(hu, c["wantU"], c["cmpU"], "u: ")
    _check(hv, c["wantV"], c["cmpV"], "v: ")
    eu, ev = plan.apply_vector_typed_host(vec, c["u"][:0], c["uBad"], c["v"][:0], c["vBad"])
    assert eu.shape == ev.shape == (0, plan.outY, plan.outX) and eu.dtype == np.dtype(dtU) and ev.dtype == np.dtype(dtV)


def test_refusals_that_need_a_plan(fa):
    """Refused with a message, nothing launched: the output buffers keep their fill."""
    import torch
    nz = 4
    inX, inY, outY = GEOMETRY["A2"][0]
    outX = A2_OUTX
    c = _a2(oracle.BILINEAR, 5)
    plan, vec = _plans(fa, c)
    st = torch.cuda.current_stream().cuda_stream
    code = oracle.cdm_type_of(np.int16)
    d_in = torch.zeros((2, nz, inY, inX), dtype=torch.int16, device="cuda")
    d_out = torch.full((2, nz, outY, outX), 7, dtype=torch.int16, device="cuda")
    u, v, uo, vo = d_in[0].data_ptr(), d_in[1].data_ptr(), d_out[0].data_ptr(), d_out[1].data_ptr()

    def call(p, vp, a, b, o0, o1, n=nz, tu=code, tv=code):
        return p.apply_vector_typed_device(vp, a, tu, -32768.0, b, tv, 32767.0, n, o0, o1, st)

    fpx, fpy = cases.forward_positions(inX, inY, outX, outY, seed=11)
    forward = fa.RegridPlan(oracle.FWD_MEAN, fpx, fpy, inX, inY, outX, outY)
    with pytest.raises(fa.FimexAmdError, match="forward plan"):
        call(forward, vec, u, v, uo, vo)
    other = fa.VectorPlan(cases.rotation_matrix(outY, outX, seed=1), outY, outX)  # ox and oy swapped
    with pytest.raises(fa.FimexAmdError, match="differs from the regrid plan's output grid"):
        call(plan, other, u, v, uo, vo)
    with pytest.raises(fa.FimexAmdError, match="differs from the regrid plan's output grid"):
        plan.apply_vector_typed_host(other, np.zeros((nz, inY, inX), np.int16), -32768.0, np.zeros((nz, inY, inX), np.int16), 32767.0)
    with pytest.raises(fa.FimexAmdError, match="cannot be regridded"):
        call(plan, vec, u, v, uo, vo, tu=6)
    last = 2 * (outX * outY * nz - 1)  # one element of the 2-byte type before the end
    for args, names in (((u, v, uo, uo), "uOut and vOut"), ((u, v, uo, uo + last), "uOut and vOut"), ((u, v, uo + last, uo), "uOut and vOut"),
                        ((u, u, uo, vo), "u and v"), ((uo, v, uo, vo), "u and uOut"), ((vo, v, uo, vo), "u and vOut"),
                        ((u, uo, uo, vo), "v and uOut"), ((u, vo, uo, vo), "v and vOut")):
        with pytest.raises(fa.FimexAmdError, match="buffers overlap: " + names):
            call(plan, vec, args[0], args[1], args[2], args[3])
    # sizes count each buffer's own elements: as floats (4 bytes) the u component reaches into the v component behind it
    with pytest.raises(fa.FimexAmdError, match="buffers overlap: u and v"):
        call(plan, vec, u, v, uo, vo, tu=oracle.cdm_type_of(np.float32))
    assert call(plan, vec, 0, 0, 0, 0, n=0) == 0  # nz == 0 succeeds and does nothing
    torch.cuda.synchronize()
    assert bool((d_out == 7).all())
