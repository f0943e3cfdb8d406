"""Time-axis interpolation and quality masking on the GPU (include/fimex_amd.h, 8f n10) through the C ABI, against
tests/time_quality_ref.py, the CPU restatement that tests/test_time_quality_ref.py pins.

  time interpolation  bit for bit on everything but NaN, whose positions must agree (a CPU and a GPU NaN that arithmetic made may
                      differ in sign and payload); output steps beyond the weak extrapolation hold the bits of MIFI_UNDEFINED_F;
                      copies (f == 0, f == 1) of float input are bit for bit, NaN included; and bit for bit, NaN included, against
                      the chain of fimex_amd_get_values_1d_f_device calls it replaces.
  quality mask        bit for bit: every byte of the data, and the bytes around it untouched.
"""
import ctypes

import numpy as np
import pytest

import time_quality_ref as tq

pytestmark = pytest.mark.gpu

BLOCK = 256   # lanes per workgroup of every kernel here (csrc/common.hpp)
GUARD = 32    # bytes kept untouched on either side of an output
NAN = np.nan


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    lib = capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    assert hasattr(lib, "fimex_amd_time_interpolate_device") and hasattr(lib, "fimex_amd_quality_mask_device")
    return capi


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _bytes(a):
    import torch
    return torch.from_numpy(tq.as_bytes(a).copy())


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(tq.as_bytes(a), tq.as_bytes(b))


def _same_up_to_nan_payload(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(tq.as_bytes(a[~na]), tq.as_bytes(b[~nb]))


# ------------------------------------------------------------------ time interpolation
def _run_time(fa, x, old, new, in_shift=0, out_shift=0):
    """The device entry on x[nOld][n] placed in_shift elements behind a 16-byte boundary, the output out_shift floats behind one; the
    bytes around the output must stay as they were.  float32 [nNew][n]."""
    import torch
    si, n, nNew = x.dtype.itemsize, x[0].size, len(new)
    src = torch.zeros(x.nbytes + 16 + si, dtype=torch.uint8, device="cuda")
    src[in_shift * si:in_shift * si + x.nbytes] = _bytes(x).cuda()
    dst = torch.full((2 * GUARD + nNew * n * 4 + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    first = GUARD + out_shift * 4
    fa.time_interpolate_device(src.data_ptr() + in_shift * si, fa.cdm_type_of(x.dtype), n, old, new, dst.data_ptr() + first, stream=_stream())
    torch.cuda.synchronize()
    raw = dst.cpu().numpy()
    assert np.all(raw[:first] == 0xAB) and np.all(raw[first + nNew * n * 4:] == 0xAB), "wrote outside the output"
    return raw[first:first + nNew * n * 4].view(np.float32).reshape(nNew, n)


def _check_time(got, x, old, new, where):
    want = tq.time_interpolate(x, old, new)
    assert _same_up_to_nan_payload(got, want), (where, int((tq.as_bytes(got) != tq.as_bytes(want)).sum()))
    und = tq.undefined_positions(old, new)
    assert np.all(got[und].view(np.uint32) == tq.UNDEFINED_F_BITS), where
    if x.dtype == np.float32:  # the copies of float input carry every bit over
        t1, t2 = tq.time_mapping(old, new)
        for i, (a, b) in enumerate(zip(t1, t2)):
            branch = tq.blend_factor(old[int(a)], old[int(b)], new[i])[1]
            if branch in (tq.COPY_A, tq.COPY_B):
                assert _same(got[i], x[int(a) if branch == tq.COPY_A else int(b)]), (where, i)


@pytest.mark.parametrize("code", tq.TYPES)
def test_time_every_type_and_size(fa, code):
    """n = 1 and 3 (one by one), 4 (one group), 63 and 64 * 4 + 1 (no multiple of four: every cell one by one, more than one wave),
    5000 (groups over five workgroups); the 29-step axis with every branch.  1- and 2-byte types also one element behind a 16-byte
    boundary, where the groups start a few cells in or nothing is aligned."""
    old, new = tq.AXES["fine"]
    dtype = np.dtype(tq.DTYPES[code])
    for n in (1, 3, 4, 63, 64 * 4 + 1, 5000):
        x = tq.series(100 * code + n % 97, dtype, old.size, n)
        for in_shift in ((0, 1) if dtype.itemsize <= 2 else (0,)):
            _check_time(_run_time(fa, x, old, new, in_shift), x, old, new, (code, n, in_shift))
    x = tq.series(7, dtype, old.size, 40)
    _check_time(_run_time(fa, x, old, new, 0, out_shift=1), x, old, new, (code, "output one float behind a boundary"))


@pytest.mark.parametrize("axis", ("coarse", "backwards", "single"))
def test_time_other_axes(fa, axis):
    old, new = tq.AXES[axis]
    for code in (tq.CDM_SHORT, tq.CDM_FLOAT, tq.CDM_DOUBLE):
        for n in (63, 260):
            x = tq.series(200 + code, tq.DTYPES[code], old.size, n)
            _check_time(_run_time(fa, x, old, new), x, old, new, (axis, code, n))


def test_time_copies_do_not_leak_nan(fa):
    """A NaN in B where f == 0 and a NaN in A where f == 1: the copy holds the other slice's value, bit for bit."""
    x = np.arange(3 * 24, dtype=np.float32).reshape(3, 24) + 1
    x[1, ::2] = NAN   # B of (0, 1) at x = 0; A of (1, 2) at x = 12
    x[0, 5] = NAN
    old, new = np.array([0.0, 6.0, 12.0]), np.array([0.0, 6.0, 12.0, 3.0])
    t1, t2 = tq.time_mapping(old, new)
    assert list(zip(t1.tolist(), t2.tolist())) == [(0, 1), (0, 1), (1, 2), (1, 2)]  # 3 is searched from position 2 on
    got = _run_time(fa, x, old, new)
    assert _same(got[0], x[0]) and _same(got[1], x[1]) and _same(got[2], x[2])
    assert np.array_equal(np.isnan(got[3]), np.isnan(x[1]) | np.isnan(x[2]))  # f = -0.5: a blend takes either NaN
    _check_time(got, x, old, new, "nan")


def _chunk_axis(fa):
    """300 steps over 10 slices: the launch boundary at step 128 lies inside the run on (1, 2), the one at 256 is where (3, 4) takes
    over from (2, 3); the 32-step chunk boundaries of a split launch lie inside runs and, at 256, on that change."""
    assert fa.TIME_LAUNCH_STEPS == 128 and fa.TIME_CHUNK_STEPS == 32
    old = np.arange(10.0)
    new = np.concatenate([np.linspace(0.005, 1.0, 100), np.linspace(1.005, 2.0, 100), np.linspace(2.01, 3.0, 56), np.linspace(3.01, 9.9, 44)])
    t1, t2 = tq.time_mapping(old, new)
    assert new.size == 300 and (t1[127], t2[127]) == (t1[128], t2[128]) == (1, 2) and (t1[255], t2[255]) == (2, 3) and (t1[256], t2[256]) == (3, 4)
    assert (t1[31], t1[32], t1[63], t1[64], t1[95], t1[96]) == (0,) * 6
    return old, new


def test_time_more_steps_than_a_launch(fa):
    old, new = _chunk_axis(fa)
    for code, n in ((tq.CDM_SHORT, 68), (tq.CDM_FLOAT, 67)):
        x = tq.series(300 + code, tq.DTYPES[code], old.size, n)
        _check_time(_run_time(fa, x, old, new), x, old, new, (code, n))


@pytest.mark.parametrize("split", (1, 2))
def test_time_capped_grid_and_forced_split(fa, tuning_build, monkeypatch, split):
    """The tuning build with two workgroups at most (5000 cells are five workgroups of groups: the grid strides three times) and the
    steps split over gridDim.y (1) or never (2), which the product library decides from n."""
    monkeypatch.setenv("FIMEX_AMD_TIME_MAX_BLOCKS", "2")
    monkeypatch.setenv("FIMEX_AMD_TIME_SPLIT_Y", str(split))
    old, new = _chunk_axis(fa)
    for code, n in ((tq.CDM_SHORT, 5000), (tq.CDM_FLOAT, 2 * BLOCK * 3 + 1)):
        x = tq.series(400 + code, tq.DTYPES[code], old.size, n)
        _check_time(_run_time(fa, x, old, new), x, old, new, (split, code, n))


def test_time_every_branch_on_either_side_of_a_chunk_boundary(fa):
    """Copy A, copy B, blend and undefined in turn, 80 steps: every branch inside one launch, and the 32-step chunk boundaries of the
    split launch (few cells: the product library splits) have all four within two steps on either side."""
    old = tq.OLD_TIMES
    new = np.tile([0.0, 6.0, 3.0, -100.0], 20)
    t1, t2 = tq.time_mapping(old, new)
    branch = [tq.blend_factor(old[int(a)], old[int(b)], x)[1] for a, b, x in zip(t1, t2, new)]
    for edge in (fa.TIME_CHUNK_STEPS, 2 * fa.TIME_CHUNK_STEPS):
        assert set(branch[edge - 2:edge + 2]) == {tq.COPY_A, tq.COPY_B, tq.BLEND, tq.UNDEFINED}
    for code, n in ((tq.CDM_FLOAT, 67), (tq.CDM_SHORT, 68), (tq.CDM_DOUBLE, 300)):
        x = tq.series(500 + code, tq.DTYPES[code], old.size, n)
        _check_time(_run_time(fa, x, old, new), x, old, new, (code, n))


def test_time_equals_the_chain_of_pair_blends(fa):
    """Bit for bit, NaN included, with one fimex_amd_get_values_1d_f_device(LINEAR_WEAK_EXTRAPOL) call per output step on float input."""
    import torch
    old, new = tq.AXES["fine"]
    n = 1000
    x = tq.series(500, np.float32, old.size, n)
    got = _run_time(fa, x, old, new)
    d_x = torch.from_numpy(x).cuda()
    d_out = torch.zeros((new.size, n), dtype=torch.float32, device="cuda")
    t1, t2 = fa.time_mapping(old, new)
    for i in range(new.size):
        a, b = int(t1[i]), int(t2[i])
        fa.get_values_1d_device(fa.BLEND_LINEAR_WEAK_EXTRAPOL, d_x[a].data_ptr(), d_x[b].data_ptr(), d_out[i].data_ptr(), n, old[a], old[b], new[i],
                                stream=_stream())
    torch.cuda.synchronize()
    assert _same(got, d_out.cpu().numpy())


def test_time_host_form_equals_the_device_form(fa):
    for axis, code, n in (("fine", tq.CDM_SHORT, 260), ("backwards", tq.CDM_DOUBLE, 63), ("single", tq.CDM_UCHAR, 5)):
        old, new = tq.AXES[axis]
        x = tq.series(600 + code, tq.DTYPES[code], old.size, n)
        before = x.copy()
        got = fa.time_interpolate_host(x, old, new)
        assert _same(got, _run_time(fa, x, old, new)) and _same(x, before)


def test_time_overlap_is_refused(fa):
    import torch
    buf = torch.zeros(4 * 64 * 4 + 2 * 64 * 4, dtype=torch.uint8, device="cuda")
    old, new = [0.0, 1.0, 2.0, 3.0], [0.5, 1.5]
    for off in (0, 4 * 64 * 4 - 4, 8):
        with pytest.raises(fa.FimexAmdError, match="overlaps"):
            fa.time_interpolate_device(buf.data_ptr(), fa.CDM_FLOAT, 64, old, new, buf.data_ptr() + off, stream=_stream())
    fa.time_interpolate_device(buf.data_ptr(), fa.CDM_FLOAT, 64, old, new, buf.data_ptr() + 4 * 64 * 4, stream=_stream())  # behind it: fine
    torch.cuda.synchronize()
    assert np.all(buf.cpu().numpy() == 0)


# ------------------------------------------------------------------ quality mask
def _run_mask(fa, data, status, mode, fill, kw, d_shift=0, s_shift=0):
    """The device entry in place on data placed d_shift elements behind a 16-byte boundary (the status s_shift); status=None: the data
    is its own status.  The bytes around the data must stay as they were."""
    import torch
    sd = data.dtype.itemsize
    buf = torch.full((2 * GUARD + data.nbytes + 16 + sd,), 0xAB, dtype=torch.uint8, device="cuda")
    first = GUARD + d_shift * sd
    buf[first:first + data.nbytes] = _bytes(data).cuda()
    if status is None:
        d_status, sType, nStatus = buf.data_ptr() + first, fa.cdm_type_of(data.dtype), data.size
    else:
        ss = status.dtype.itemsize
        st = torch.zeros(status.nbytes + 16 + ss, dtype=torch.uint8, device="cuda")
        st[s_shift * ss:s_shift * ss + status.nbytes] = _bytes(status).cuda()
        d_status, sType, nStatus = st.data_ptr() + s_shift * ss, fa.cdm_type_of(status.dtype), status.size
    fa.quality_mask_device(buf.data_ptr() + first, fa.cdm_type_of(data.dtype), data.size, d_status, sType, nStatus, mode, fill, stream=_stream(), **kw)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert np.all(raw[:first] == 0xAB) and np.all(raw[first + data.nbytes:] == 0xAB), "wrote outside the data"
    if status is not None:
        assert np.array_equal(st.cpu().numpy()[s_shift * ss:s_shift * ss + status.nbytes], tq.as_bytes(status)), "wrote to the status"
    return raw[first:first + data.nbytes].view(data.dtype).reshape(data.shape)


def _check_mask(fa, data, status, mode, fill, kw, where, **shifts):
    want = tq.quality_mask(data, status, mode, fill, **kw)
    got = _run_mask(fa, data, status, mode, fill, kw, **shifts)
    assert _same(got, want), (where, int((tq.as_bytes(got) != tq.as_bytes(want)).sum()))
    return want


MASK_DATA = (tq.CDM_CHAR, tq.CDM_SHORT, tq.CDM_INT, tq.CDM_FLOAT, tq.CDM_DOUBLE, tq.CDM_UINT64)
MASK_STATUS = (tq.CDM_UCHAR, tq.CDM_SHORT, tq.CDM_FLOAT, tq.CDM_DOUBLE)


@pytest.mark.parametrize("mode", tq.MODES)
def test_mask_every_mode_and_type(fa, mode):
    """Six data types against four status types, the status once and three times along the data; 16 * 63 status cells, so that the
    repeats of every type start on a 16-byte boundary and the groups run, over one to four workgroups."""
    kw = tq.mode_arguments(mode)
    for s in MASK_STATUS:
        status = tq.status_values(700 + s, tq.DTYPES[s], 16 * 63)
        for c in MASK_DATA:
            for ratio in (1, 3):
                data = tq.data_values(710 + c, tq.DTYPES[c], (ratio, status.size))
                want = _check_mask(fa, data, status, mode, 77.0, kw, (mode, c, s, ratio))
                assert 0 < (want != data).sum() < data.size


@pytest.mark.parametrize("nStatus", (1, 5, 16, 4097))
def test_mask_sizes_and_offsets(fa, nStatus):
    """One cell, fewer cells than a group, one group of the narrowest type, 4097 (an odd repeat length: with three repeats every cell
    goes one by one, over seventeen workgroups); data and status on 16-byte boundaries and one element behind them."""
    for c, s in ((tq.CDM_SHORT, tq.CDM_UCHAR), (tq.CDM_DOUBLE, tq.CDM_FLOAT), (tq.CDM_CHAR, tq.CDM_SHORT)):
        status = tq.status_values(720 + nStatus % 89, tq.DTYPES[s], nStatus, nan_share=0.3)
        for ratio in (1, 3):
            data = tq.data_values(730 + c, tq.DTYPES[c], (ratio, nStatus))
            for d_shift, s_shift in ((0, 0), (1, 0), (0, 1), (1, 1)):
                _check_mask(fa, data, status, tq.MAX, -3.5, {"limit": 4.0, "statusFill": 0.0}, (nStatus, c, s, ratio, d_shift, s_shift),
                            d_shift=d_shift, s_shift=s_shift)


def test_mask_lane_cases(fa):
    """Groups of a lane's 16 bytes with every cell masked (one store), none (no access) and some (load, merge, store), for 2-byte and
    8-byte data, over 3, 4 and 9 repeats."""
    for c, per in ((tq.CDM_SHORT, 8), (tq.CDM_DOUBLE, 2)):
        pattern = np.concatenate([np.full(per, 9), np.full(per, 1), np.arange(per) % 2 * 8 + 1, np.full(per, 1), np.full(per, 9)])  # 9: the fill
        status = np.tile(pattern, 40).astype(np.uint8)  # 1600 or 400 cells
        m = tq.masked_status(status, tq.ALL, statusFill=9.0).reshape(-1, per)
        assert m.all(axis=1).any() and (~m).all(axis=1).any() and (m.any(axis=1) & ~m.all(axis=1)).any()
        for repeats in (3, 4, 9):
            data = tq.data_values(740, tq.DTYPES[c], (repeats, status.size))
            _check_mask(fa, data, status, tq.ALL, 77.0, {"statusFill": 9.0}, (c, repeats, "lanes"))
    # nothing masked at all, everything masked
    status = np.full(2000, 3, np.int16)
    data = tq.data_values(741, np.float32, (3, 2000))
    assert _same(_check_mask(fa, data, status, tq.ALL, NAN, {}, "none"), data)
    assert np.isnan(_check_mask(fa, data, status, tq.ALL, NAN, {"validMax": 2.0}, "all")).all()


def test_mask_value_lists(fa):
    """One value, and more values than travel as kernel arguments (unsorted, with repeats), through the binary search on the device."""
    status = tq.status_values(750, np.float64, 3000)
    status[::7] += 0.5  # no listed value
    status[5], status[6] = -0.0, 1e300
    data = tq.data_values(751, np.int32, (2, 3000))
    long_list = [9.0, 0.0, 4.0, 4.0, 2.0, 7.0, 1e300, -5.0, 3.0, 100.0, 8.0, 6.5, 1.0, 1e-300, -1e300, 12.0, 11.0, 10.0, 13.0, 5.0]
    for values in ([3.0], [3.0, 1.0], long_list[:8], long_list[:9], long_list):
        want = _check_mask(fa, data, status, tq.VALUES, -1.0, {"values": values, "validMin": 100.0, "statusFill": 3.0}, len(values))
        assert 0 < (want != data).sum() < data.size
    many = np.arange(300.0)[::-1] * 0.5  # three uploads of kernel arguments
    _check_mask(fa, data, status, tq.VALUES, -1.0, {"values": many}, "300 values")


def test_mask_own_status(fa):
    for dtype in (np.float32, np.int16, np.float64):
        x = tq.status_values(760, dtype, 1999, nan_share=0.2)
        for d_shift in (0, 1):
            want = _check_mask(fa, x, None, tq.MAX, -1.0, {"limit": 6.0, "validMin": 1.0}, (dtype, d_shift), d_shift=d_shift)
            assert 0 < (want != x).sum() < x.size
    import torch
    buf = torch.zeros(64, dtype=torch.int16, device="cuda")
    for args in ((buf.data_ptr(), fa.CDM_SHORT, 64, buf.data_ptr(), fa.CDM_SHORT, 32), (buf.data_ptr(), fa.CDM_SHORT, 64, buf.data_ptr(), fa.CDM_USHORT, 64),
                 (buf.data_ptr(), fa.CDM_SHORT, 32, buf.data_ptr() + 2, fa.CDM_SHORT, 32)):
        with pytest.raises(fa.FimexAmdError, match="own status|overlaps"):
            fa.quality_mask_device(*args, fa.QUALITY_ALL, 0.0, stream=_stream())


@pytest.mark.parametrize("mode", (tq.HIGHEST, tq.LOWEST))
def test_mask_extreme(fa, mode):
    """The extreme in the last cell of a status that four workgroups reduce; among values the valid range and the fill take out; in
    the first cell; with no defined status at all."""
    n = 3 * BLOCK + 200
    extreme, outside, fill = (50.0, 60.0, 55.0) if mode == tq.HIGHEST else (-50.0, -60.0, -55.0)
    kw = {"validMin": -58.0, "validMax": 58.0, "statusFill": fill}
    for dtype in (np.float32, np.int16):
        for where in (n - 1, 0, n // 2):
            status = tq.status_values(770, dtype, n, nan_share=0.1)
            status[where] = extreme
            status[3], status[n - 2] = outside, fill  # more extreme, but undefined
            data = tq.data_values(771, np.int16, (3, n))
            want = _check_mask(fa, data, status, mode, -32767.0, kw, (mode, dtype, where))
            assert np.array_equal(np.flatnonzero((want == data).all(axis=0)), [where])
        none = np.full(n, outside, dtype)
        if np.dtype(dtype).kind == "f":
            none[::3] = NAN
        want = _check_mask(fa, data, none, mode, -32767.0, kw, (mode, dtype, "none defined"))
        assert np.all(want == -32767)


def test_mask_host_form_equals_the_device_form(fa):
    status = tq.status_values(780, np.uint8, 1000)
    for mode in tq.MODES:
        data = tq.data_values(781, np.int16, (3, 1000))
        before = data.copy()
        kw = tq.mode_arguments(mode)
        got = fa.quality_mask_host(data, status, mode, -32767.0, **kw)
        assert _same(got, _run_mask(fa, data, status, mode, -32767.0, kw)) and _same(data, before)
    x = tq.status_values(782, np.float32, 777, nan_share=0.2)
    assert _same(fa.quality_mask_host(x, None, tq.MIN, -1.0, limit=4.0), _run_mask(fa, x, None, tq.MIN, -1.0, {"limit": 4.0}))


def test_empty_host_calls(fa):
    """n == 0, nNew == 0, nData == 0 with NULL wherever the checks allow NULL: OK, and nothing written (the rows of these two entries
    for tests/test_gpu_host_entries.py::test_empty_host_calls, which spells out the *_host names of capi.SYMBOLS alone)."""
    lib = fa.load()
    f_out, b_out = np.full(4, -7.0, np.float32), np.full(8, 0xA5, np.uint8)
    old, new = np.array([0.0, 1.0]), np.array([0.5])
    calls = {
        "fimex_amd_time_interpolate_host": [(None, fa.CDM_SHORT, 0, fa._dp(old), 2, fa._dp(new), 1, fa._fp(f_out)),
                                            (None, fa.CDM_SHORT, 4, fa._dp(old), 2, None, 0, fa._fp(f_out))],
        "fimex_amd_quality_mask_host": [(b_out.ctypes.data, fa.CDM_SHORT, 0, None, fa.CDM_UCHAR, 0, fa.QUALITY_ALL, None, 0, NAN, NAN, NAN, NAN, 0.0),
                                        (b_out.ctypes.data, fa.CDM_SHORT, 0, None, fa.CDM_UCHAR, 7, fa.QUALITY_HIGHEST, None, 0, NAN, NAN, NAN, NAN, 0.0)],
    }
    assert set(calls) == set(fa.TIME_QUALITY_HOST_SYMBOLS)
    for name, rows in calls.items():
        for args in rows:
            assert getattr(lib, name)(*args) == fa.OK, "%s: %s" % (name, lib.fimex_amd_last_error().decode())
            assert np.all(f_out == -7.0) and np.all(b_out == 0xA5), "%s wrote to an array" % name
    s = ctypes.c_void_p(_stream())
    assert lib.fimex_amd_time_interpolate_device(None, fa.CDM_SHORT, 0, fa._dp(old), 2, fa._dp(new), 1, None, s) == fa.OK
    assert lib.fimex_amd_quality_mask_device(None, fa.CDM_SHORT, 0, None, fa.CDM_UCHAR, 0, fa.QUALITY_ALL, None, 0, NAN, NAN, NAN, NAN, 0.0, s) == fa.OK
