"""The *_host entries of the C boundary as round trips (csrc/host_call.hpp): what the helper that carries one host call can get
wrong, pinned against the *_device twin of each entry, which passes the caller's device pointers straight to the same launch.

Every comparison is bit for bit, NaN in the same cells: both forms run the same kernels on the same values, only the copies differ.
"""
import ctypes
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # a copy


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _identical(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        same = (gn & wn) | (~gn & ~wn & (_bits(got) == _bits(want)))
    else:
        same = got == want
    print("%s: %d cells, %.4f %% bit-identical" % (label, want.size, 100.0 * np.count_nonzero(same) / max(want.size, 1)))
    assert np.all(same), "%s: %d cells differ, first at %s" % (label, np.count_nonzero(~same), tuple(np.argwhere(~same)[0]))


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


# ------------------------------------------------------------------------------------ 1. data2interpolation / interpolation2data
CONVERT_TYPES = [("short", np.int16, -32767.0), ("uchar", np.uint8, 255.0), ("int", np.int32, -2147483647.0), ("float", np.float32, -999.0)]


@pytest.mark.parametrize("n", [1, 255, 1027])
@pytest.mark.parametrize("name,dtype,fill", CONVERT_TYPES, ids=[t[0] for t in CONVERT_TYPES])
def test_data2interpolation_host_is_the_device_entry(fa, name, dtype, fill, n):
    import torch
    rng = np.random.default_rng(n)
    data = rng.integers(0, 200, n).astype(dtype)
    data[::3] = dtype(fill)  # n == 1: the one value is the fill value
    code = fa.cdm_type_of(dtype)
    got = np.full(n, -7.0, np.float32)
    fa._check(fa.load().fimex_amd_data2interpolation_host(_vp(data), code, n, fill, got.ctypes.data_as(fa._F)))
    d_in, d_out = _dev(data), torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    fa.data2interpolation_device(d_in.data_ptr(), code, n, fill, d_out.data_ptr(), _stream())
    want = _host(d_out)
    assert np.isnan(want[0]) and np.count_nonzero(np.isnan(want)) == len(range(0, n, 3))
    _identical(got, want, "data2interpolation %s n %d" % (name, n))


@pytest.mark.parametrize("n", [1, 255, 1027])
@pytest.mark.parametrize("name,dtype,fill", CONVERT_TYPES, ids=[t[0] for t in CONVERT_TYPES])
def test_interpolation2data_host_is_the_device_entry(fa, name, dtype, fill, n):
    import torch
    rng = np.random.default_rng(n + 1)
    data = rng.uniform(0, 200, n).astype(np.float32)
    data[::3] = np.nan
    code = fa.cdm_type_of(dtype)
    got = np.zeros(n, dtype)
    fa._check(fa.load().fimex_amd_interpolation2data_host(data.ctypes.data_as(fa._F), n, code, fill, _vp(got)))
    d_in, d_out = _dev(data), torch.zeros((n,), dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
    fa.interpolation2data_device(d_in.data_ptr(), n, code, fill, d_out.data_ptr(), _stream())
    want = _host(d_out)
    assert want[0] == dtype(fill)
    _identical(got, want, "interpolation2data %s n %d" % (name, n))


# --------------------------------------------------------------------------------------------------------- 2. optional arrays
NX, NY, NZ, NT = 5, 4, 3, 2


def _pressure_levels(fa, ps):
    """hybrid_sigma_ap with ps a host array or a device pointer"""
    return fa.VerticalLevels.hybrid_sigma_ap([2000., 8000., 0.], [0.1, 0.5, 1.0], ps)


@pytest.mark.parametrize("optional", [False, True], ids=["bare", "humidity+topography"])
def test_altitude_integrate_host_optional_arrays(fa, optional):
    import torch
    rng = np.random.default_rng(11)
    ps = rng.normal(100000, 1500, (NT, NY, NX)).astype(np.float32)
    T = rng.normal(270, 15, (NT, NZ, NY, NX)).astype(np.float32)
    q = rng.uniform(0, 0.01, (NT, NZ, NY, NX)).astype(np.float32) if optional else None
    sgp = rng.uniform(0, 5000, (NT, NY, NX)).astype(np.float32)
    topo = rng.uniform(0, 500, (NY, NX)) if optional else None
    got = fa.vertical_altitude_integrate_host(_pressure_levels(fa, ps), NX, NY, NT, T, ps, sgp, specificHumidity=q, topo=topo)
    d_ps, d_T, d_sgp = _dev(ps), _dev(T), _dev(sgp)
    d_q, d_topo = (_dev(q), _dev(topo)) if optional else (None, None)
    d_out = torch.full((NT, NZ, NY, NX), -7.0, dtype=torch.float32, device="cuda")
    fa.vertical_altitude_integrate_device(_pressure_levels(fa, d_ps.data_ptr()), NX, NY, NT, d_T.data_ptr(), d_ps.data_ptr(), d_sgp.data_ptr(),
                                          d_out.data_ptr(), d_specificHumidity=d_q.data_ptr() if optional else None,
                                          d_topo=d_topo.data_ptr() if optional else None, stream=_stream())
    want = _host(d_out)
    assert np.count_nonzero(np.isfinite(want)) > want.size // 2
    _identical(got, want, "altitude_integrate, optional arrays %s" % optional)


@pytest.mark.parametrize("bounds", ["min", "max", "both"])
def test_vertical_interpolate_host_valid_arrays(fa, bounds):
    import torch
    rng = np.random.default_rng(12)
    data = rng.normal(280, 10, (NT, NZ, NY, NX)).astype(np.float32)
    axis, level1 = [1000., 850., 500.], np.array([925., 700., 400., 1010.])
    vmin = rng.choice([300., 600., 950.], (NY, NX)) if bounds != "max" else None  # each bound cuts some levels in some columns
    vmax = rng.choice([750., 950., 1100.], (NY, NX)) if bounds != "min" else None
    got = fa.vertical_interpolate_host(fa.VINT_METHOD_LIN, data, fa.VerticalLevels.from_axis(axis), None, level1, validMin=vmin, validMax=vmax)
    d_in, d_min, d_max = _dev(data), _dev(vmin) if vmin is not None else None, _dev(vmax) if vmax is not None else None
    d_out = torch.full((NT, level1.size, NY, NX), -7.0, dtype=torch.float32, device="cuda")
    fa.vertical_interpolate_device(fa.VINT_METHOD_LIN, NX, NY, NT, d_in.data_ptr(), fa.VerticalLevels.from_axis(axis), d_out.data_ptr(), None, level1,
                                   d_validMin=d_min.data_ptr() if d_min is not None else None,
                                   d_validMax=d_max.data_ptr() if d_max is not None else None, stream=_stream())
    want = _host(d_out)
    nan = np.count_nonzero(np.isnan(want))
    assert 0 < nan < want.size, "the bounds cut %d of %d cells" % (nan, want.size)
    _identical(got, want, "vertical_interpolate, valid %s" % bounds)


# ------------------------------------------------------------------- 3. a distinct output pointer after in-place work on the device
SX, SY, SZ = 7, 6, 2


def _two_fields(seed):
    rng = np.random.default_rng(seed)
    a, b = rng.normal(280, 5, (SZ, SY, SX)).astype(np.float32), rng.normal(280, 5, (SZ, SY, SX)).astype(np.float32)
    a[rng.random(a.shape) < 0.2] = np.nan
    b[rng.random(b.shape) < 0.2] = np.nan
    return a, b


def _unchanged(arrays, copies, label):
    for k, (a, c) in enumerate(zip(arrays, copies)):
        assert np.array_equal(_bits(a), _bits(c)), "%s: input %d was written" % (label, k)


def test_overlay_host_leaves_its_inputs(fa):
    import torch
    top, base = _two_fields(31)
    copies = (top.copy(), base.copy())
    got = fa.overlay_host(top, base)
    _unchanged((top, base), copies, "overlay_host")
    d_top, d_base, d_out = _dev(top), _dev(base), torch.full(top.shape, -7.0, dtype=torch.float32, device="cuda")
    fa.overlay_device(d_top.data_ptr(), d_base.data_ptr(), d_out.data_ptr(), top.size, _stream())
    _identical(got, _host(d_out), "overlay host against device")


def test_border_smooth_host_leaves_its_inputs(fa):
    import torch
    inner, outer = _two_fields(32)
    copies = (inner.copy(), outer.copy())
    got = fa.border_smooth_host(inner, outer, 2, 1, True)
    _unchanged((inner, outer), copies, "border_smooth_host")
    d_inner, d_outer, d_out = _dev(inner), _dev(outer), torch.full(inner.shape, -7.0, dtype=torch.float32, device="cuda")
    fa.border_smooth_device(d_inner.data_ptr(), d_outer.data_ptr(), d_out.data_ptr(), SX, SY, SZ, 2, 1, True, _stream())
    _identical(got, _host(d_out), "border_smooth host against device")


def test_omega_to_vertical_wind_host_leaves_its_inputs(fa):
    import torch
    rng = np.random.default_rng(33)
    nt, nz = SZ, 3
    ps = rng.normal(100000, 1500, (nt, SY, SX)).astype(np.float32)
    omega = rng.normal(0, 0.5, (nt, nz, SY, SX)).astype(np.float32)
    t = rng.normal(270, 15, (nt, nz, SY, SX)).astype(np.float32)
    omega[0, 1, 2, 3] = np.nan
    copies = (omega.copy(), t.copy(), ps.copy())
    got = fa.omega_to_vertical_wind_host(_pressure_levels(fa, ps), SX, SY, nt, omega, t)
    _unchanged((omega, t, ps), copies, "omega_to_vertical_wind_host")
    d_ps, d_omega, d_t, d_out = _dev(ps), _dev(omega), _dev(t), torch.full(omega.shape, -7.0, dtype=torch.float32, device="cuda")
    fa.omega_to_vertical_wind_device(_pressure_levels(fa, d_ps.data_ptr()), SX, SY, nt, d_omega.data_ptr(), d_t.data_ptr(), d_out.data_ptr(), _stream())
    _identical(got, _host(d_out), "omega_to_vertical_wind host against device")


# ------------------------------------------------------------------------------------ 4. the error path leaves the library usable
def _refused_then_served(fa):
    """a refused argument, not a device fault: the log blend with a non-positive coordinate"""
    A, B = np.array([2., 4., -6., 8., 0.], np.float32), np.array([4., 8., 2., 8., 10.], np.float32)
    out = np.full(A.size, -7.0, np.float32)
    with pytest.raises(fa.FimexAmdError, match="log blend needs positive coordinates"):
        fa._check(fa.load().fimex_amd_get_values_1d_f_host(fa.BLEND_LOG, fa._fp(A), fa._fp(B), fa._fp(out), A.size, -1.0, 10.0, 5.0))
    assert np.array_equal(_bits(out), _bits(np.full(A.size, -7.0, np.float32))), "the refused call wrote its output"
    # half way between integers with even differences: exact in float however the blend is written
    got = fa.get_values_1d_host(fa.BLEND_LINEAR, A, B, 0.0, 1.0, 0.5)
    assert np.array_equal(got, np.array([3., 6., -2., 8., 5.], np.float32)), got


def test_refused_host_call_leaves_the_library_usable(fa):
    _refused_then_served(fa)
    failure = []

    def run():  # the error channel is thread-local
        try:
            _refused_then_served(fa)
        except BaseException as e:  # noqa: B902 - handed to the main thread
            failure.append(e)

    th = threading.Thread(target=run)
    th.start()
    th.join()
    if failure:
        raise failure[0]


# ---------------------------------------------------------------------------------------------------------------- 5. empty calls
# entries whose checks demand a non-empty grid
NOT_EMPTY = {"fimex_amd_griddistance_host": "nx > 0, ny > 0 and all four arrays",
             "fimex_amd_grid_distance_host": "orgX * orgY > 0 and all three pointers"}
GEO, STERE = b"+proj=latlong +R=6371000", b"+proj=stere +lat_0=90 +lon_0=0 +lat_ts=60 +a=6371000 +e=0"


def test_empty_host_calls(fa):
    """n == 0 (nz, nt, size: whatever makes the call empty) with NULL wherever the checks allow NULL: OK, and nothing written"""
    lib = fa.load()
    plan = fa.RegridPlan(fa.NEAREST_NEIGHBOR, np.tile(np.arange(4.), 3), np.repeat(np.arange(3.), 4), 4, 3, 4, 3)
    vec = fa.VectorPlan(np.tile([1., 0., 0., 1.], 12), 4, 3)
    merge = fa.MergePlan(plan, plan, plan)
    levels = ctypes.byref(fa.VerticalLevels.from_axis([1., 2.]).struct)
    out = np.full(4, -7.0, np.float32)  # for the entries whose NULL output means something else (the size query)
    n = ctypes.c_size_t(99)
    one = np.ones(9, np.float32)
    coeff = np.ones(1)
    # a live output pointer with nothing to write, wherever the checks allow one: a zero-length copy back must stay one
    f_out, d_out, b_out = np.full(4, -7.0, np.float32), np.full(4, -7.0), np.full(8, 0xA5, np.uint8)
    fo, do, bo = fa._fp(f_out), fa._dp(d_out), _vp(b_out)
    calls = {
        "fimex_amd_regrid_apply_host": (plan._h, None, 0, fa._fp(out), out.size, ctypes.byref(n)),
        "fimex_amd_regrid_slice_host": (plan._h, None, 0, NAN, None, 0, None, NAN, None, 0, None, 0, fa._fp(out), out.size, ctypes.byref(n)),
        "fimex_amd_regrid_slice_typed_host": (plan._h, None, fa.CDM_SHORT, 0, -32767.0, None, 0, None, fa.CDM_SHORT, -32767.0, None, 0, None, 0,
                                              _vp(out), out.size, ctypes.byref(n)),
        "fimex_amd_vector_reproject_values_host": (vec._h, fo, fo, 0),
        "fimex_amd_vector_reproject_direction_host": (vec._h, fo, 0),
        "fimex_amd_vector_reproject_direction_scaled_host": (vec._h, fo, 0, 1.0, 0.0),
        "fimex_amd_rotate_vector_typed_host": (vec._h, None, fa.CDM_SHORT, -32767.0, None, fa.CDM_SHORT, -32767.0, 0, 1, fa.CDM_SHORT, -32767.0, bo),
        "fimex_amd_fill2d_host": (4, 3, 0, fo, 4e-3, 1.6, 100, None),
        "fimex_amd_creepfill2d_host": (4, 3, 0, fo, 20, b"\x02", None),
        "fimex_amd_creepfillval2d_host": (4, 3, 0, fo, 0.0, 20, b"\x02", None),
        "fimex_amd_points2position_host": (do, 0, None, 0, fa.PROJ_AXIS),
        "fimex_amd_data2interpolation_host": (None, fa.CDM_SHORT, 0, -32767.0, fo),
        "fimex_amd_interpolation2data_host": (None, 0, fa.CDM_SHORT, -32767.0, bo),
        "fimex_amd_get_values_1d_f_host": (fa.BLEND_LINEAR, None, None, fo, 0, 0.0, 1.0, 0.5),
        "fimex_amd_vertical_interpolate_host": (fa.VINT_METHOD_LIN, 4, 3, 0, None, levels, None, None, 0, None, None, NAN, NAN, fo),
        "fimex_amd_vertical_levels_host": (levels, 4, 3, 0, fo),
        "fimex_amd_vertical_altitude_integrate_host": (levels, 4, 3, 0, None, None, None, None, fa.VORDER_AUTO, None, -1.0, fo),
        "fimex_amd_vertical_standard_altitude_host": (levels, 4, 3, 0, None, -1.0, fo),
        "fimex_amd_vertical_standard_pressure_host": (levels, 4, 3, 0, None, 1.0, fo),
        "fimex_amd_vertical_ocean_depth_host": (1, 4, 3, 2, 0, None, None, 10.0, None, None, fo),
        # the grid, its distances and the coefficients are demanded whatever nt is
        "fimex_amd_vertical_velocity_host": (3, 3, 1, 0, 1000.0, 1000.0, fa._fp(one), fa._fp(one), fa._dp(coeff), fa._dp(coeff), None, None, None, None,
                                             None, fo),
        "fimex_amd_omega_to_vertical_wind_host": (levels, 4, 3, 0, None, None, fo),
        "fimex_amd_border_smooth_host": (None, None, fo, 4, 3, 0, 5, 2, 1),
        "fimex_amd_overlay_host": (None, None, fo, 0),
        "fimex_amd_merge_apply_host": (merge._h, None, None, 0, fo),
        "fimex_amd_project_values_host": (GEO, STERE, do, do, 0),
        "fimex_amd_project_axes_host": (GEO, STERE, None, None, 0, 0, do, do),
        "fimex_amd_get_vector_reproject_matrix_host": (GEO, STERE, None, None, fa.PROJ_AXIS, fa.PROJ_AXIS, 0, 0, do),
        "fimex_amd_get_vector_reproject_matrix_field_host": (GEO, STERE, None, None, 0, 0, do),
        "fimex_amd_get_vector_reproject_matrix_points_host": (GEO, STERE, 0, None, None, 0, do),
        "fimex_amd_coord_nearest_host": (do, do, 0, None, None, 0, 0),
        "fimex_amd_coord_kdtree_host": (1000.0, do, do, 0, None, None, 0, 0),
    }
    host_entries = {name for name in fa.SYMBOLS if name.endswith("_host")}
    assert host_entries == set(calls) | set(NOT_EMPTY), sorted(host_entries ^ (set(calls) | set(NOT_EMPTY)))
    for name, args in calls.items():
        rc = getattr(lib, name)(*args)
        assert rc == fa.OK, "%s: %s" % (name, lib.fimex_amd_last_error().decode())
        assert np.all(out == -7.0) and np.all(one == 1.0) and np.all(f_out == -7.0) and np.all(d_out == -7.0) and np.all(b_out == 0xA5), \
            "%s wrote to an array" % name
    assert n.value == 0  # the three regrid entries report the size of nothing
    merge.close()


# --------------------------------------------------------------------------------------------------- 6. the pinned-ring threshold
def test_overlay_host_over_the_staged_copy_threshold(fa):
    """4 Mi + 3 floats, just over the 16 MiB from which host_to_device / device_to_host stage through the pinned ring"""
    n = 4 * 1024 * 1024 + 3
    rng = np.random.default_rng(6)
    top, base = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
    top[rng.random(n) < 0.4] = np.nan
    base[rng.random(n) < 0.1] = np.nan
    top[-3:] = [np.nan, 1.5, np.nan]  # the three cells past 4 Mi
    copies = (top.copy(), base.copy())
    got = fa.overlay_host(top, base)
    _unchanged((top, base), copies, "overlay_host, 16 MiB + 12 bytes")
    _identical(got, np.where(np.isnan(top), base, top), "overlay_host, 16 MiB + 12 bytes")
