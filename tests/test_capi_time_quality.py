"""The (8f n10) entries at the C boundary: both libraries export the five symbols, include/fimex_amd_time_quality_host.h is plain C and
names exactly what the binding's table names, and what can be refused without a device is refused with a message.  CPU only: nothing
is computed on a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from fimex_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "fimex_amd_time_quality_host.h"
NAMES = ("fimex_amd_time_mapping", "fimex_amd_time_interpolate_device", "fimex_amd_time_interpolate_host", "fimex_amd_quality_mask_device",
         "fimex_amd_quality_mask_host")
NAN = float("nan")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fimex_amd_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    declared = _declared(HEADER)
    assert declared == sorted(n for n in NAMES if n.endswith("_host"))
    assert sorted(capi.TIME_QUALITY_HOST_SYMBOLS) == declared
    assert not set(declared) & (set(capi.SYMBOLS) | set(capi.DERIVED_HOST_SYMBOLS))
    twins = set(_declared("fimex_amd.h"))
    assert all(name[:-len("_host")] + "_device" in twins for name in declared)
    assert set(NAMES) - set(declared) <= set(capi.SYMBOLS)


def test_both_libraries_export_the_five_symbols():
    for path in (capi.LIB_PATH, capi.TUNING_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(lib, name), "missing export in %s: %s" % (os.path.basename(path), name)


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\nint main(void){return FIMEX_AMD_QUALITY_LOWEST == 5 ? 0 : 1;}\n' % HEADER)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_constants_agree_with_the_header():
    text = open(os.path.join(ROOT, "include", "fimex_amd.h")).read()
    assert int(re.search(r"#define FIMEX_AMD_TIME_LAUNCH_STEPS (\d+)", text).group(1)) == capi.TIME_LAUNCH_STEPS
    assert int(re.search(r"#define FIMEX_AMD_TIME_CHUNK_STEPS (\d+)", text).group(1)) == capi.TIME_CHUNK_STEPS
    assert (capi.QUALITY_VALUES, capi.QUALITY_ALL, capi.QUALITY_MAX, capi.QUALITY_MIN, capi.QUALITY_HIGHEST, capi.QUALITY_LOWEST) == tuple(range(6))


def _refused(call, *args, match):
    with pytest.raises(capi.FimexAmdError, match=match):
        call(*args)


@pytest.mark.parametrize("old", ([0.0, 2.0, 1.0], [1.0, 1.0], [0.0, NAN], [NAN], []))
def test_bad_old_times_are_refused_without_a_device(old):
    x = np.zeros((max(len(old), 1), 4), np.int16)
    out = np.zeros((1, 4), np.float32)
    match = "nOld == 0" if not old else "ascending|NaN"
    _refused(capi.time_mapping, old, [0.5], match=match)
    # 1 is no device pointer: the times are checked before any pointer is looked at, on host and device form alike
    _refused(capi.time_interpolate_device, 1, capi.CDM_SHORT, 4, old, [0.5], 1, match=match)
    lib = capi.load()
    o = np.asarray(old, np.float64)
    rc = lib.fimex_amd_time_interpolate_host(x.ctypes.data, capi.CDM_SHORT, 4, capi._dp(o) if o.size else None, o.size, capi._dp(np.array([0.5])), 1,
                                             capi._fp(out.reshape(-1)))
    assert rc == capi.ERROR and re.search(match, lib.fimex_amd_last_error().decode())
    assert np.all(out == 0)


def test_mask_refusals_need_no_device():
    data, status = np.zeros(12, np.int16), np.zeros(5, np.uint8)
    _refused(capi.quality_mask_host, data, status, capi.QUALITY_ALL, 0.0, match="incompatible sizes")
    _refused(capi.quality_mask_host, data, np.zeros(0, np.uint8), capi.QUALITY_ALL, 0.0, match="incompatible sizes")
    _refused(capi.quality_mask_host, data, status[:4], capi.QUALITY_VALUES, 0.0, (1.0, NAN), match="NaN among")
    _refused(capi.quality_mask_host, data, status[:4], capi.QUALITY_VALUES, 0.0, match="no status values")
    _refused(capi.quality_mask_host, data, status[:4], 6, 0.0, match="unknown quality mode")
    _refused(capi.quality_mask_host, data, status[:4], capi.QUALITY_ALL, 32767.5, match="not representable")
    _refused(capi.quality_mask_host, data.astype(np.uint8), status[:4], capi.QUALITY_ALL, -1.0, match="not representable")
    _refused(capi.quality_mask_device, 1, capi.CDM_SHORT, 12, 2, capi.CDM_UCHAR, 5, capi.QUALITY_ALL, 0.0, match="incompatible sizes")
    _refused(capi.quality_mask_device, 1, capi.CDM_SHORT, 12, 2, 6, 4, capi.QUALITY_ALL, 0.0, match="data type 6")  # a string status has no double form
    # the data under its own address as the status needs one type and one size
    _refused(capi.quality_mask_device, 16, capi.CDM_SHORT, 12, 16, capi.CDM_SHORT, 4, capi.QUALITY_ALL, 0.0, match="own status")
    _refused(capi.quality_mask_device, 16, capi.CDM_SHORT, 12, 20, capi.CDM_SHORT, 4, capi.QUALITY_ALL, 0.0, match="overlaps")


def test_overlapping_series_is_refused_without_a_device():
    # input: 4 slices of 8 shorts at address 4096; an output of 2 x 8 floats that starts inside it
    for d_out in (4096, 4096 + 63, 4096 - 63):
        _refused(capi.time_interpolate_device, 4096, capi.CDM_SHORT, 8, [0.0, 1.0, 2.0, 3.0], [0.5, 1.5], d_out, match="overlaps")


def test_empty_calls_need_no_device():
    """The empty call returns OK after the checks of the times and the rule, with NULL data pointers, on a machine without a GPU too."""
    lib = capi.load()
    old, new = np.array([0.0, 1.0]), np.array([0.5])
    for n, nNew in ((0, 1), (4, 0)):
        assert lib.fimex_amd_time_interpolate_device(None, capi.CDM_SHORT, n, capi._dp(old), 2, capi._dp(new), nNew, None, None) == capi.OK
        assert lib.fimex_amd_time_interpolate_host(None, capi.CDM_SHORT, n, capi._dp(old), 2, capi._dp(new), nNew, None) == capi.OK
    assert lib.fimex_amd_quality_mask_device(None, capi.CDM_SHORT, 0, None, capi.CDM_UCHAR, 0, capi.QUALITY_ALL, None, 0, NAN, NAN, NAN, NAN, 0.0,
                                             None) == capi.OK
    assert lib.fimex_amd_quality_mask_host(None, capi.CDM_SHORT, 0, None, capi.CDM_UCHAR, 5, capi.QUALITY_ALL, None, 0, NAN, NAN, NAN, NAN,
                                           0.0) == capi.OK
