"""The (8f n5b) entries at the C boundary: both libraries export the eight symbols, the binding mirrors the two headers, and everything
that can be refused without a device is refused with a message before one is touched.  CPU only: nothing is computed on a device.
(The refusals of an apply that need a plan are in tests/test_gpu_vertical_plan.py: a plan cannot be made without a device.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from fimex_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_NAMES = ("fimex_amd_vertical_plan_create_device", "fimex_amd_vertical_plan_destroy", "fimex_amd_vertical_plan_info",
                "fimex_amd_vertical_plan_apply_device")
HOST_NAMES = ("fimex_amd_vertical_plan_create_host", "fimex_amd_vertical_plan_apply_host", "fimex_amd_vertical_plan_read_host")
HOST_HEADER = "fimex_amd_vertical_plan_host.h"
NX, NY, NT = 8, 4, 1


def _header(name="fimex_amd.h"):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared(text):
    return set(re.findall(r"\b(fimex_amd_[a-z0-9_]+)\s*\(", text))


def test_both_libraries_export_the_symbols():
    for path in (capi.LIB_PATH, capi.TUNING_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in DEVICE_NAMES + HOST_NAMES:
            assert hasattr(lib, name), "missing export in %s: %s" % (os.path.basename(path), name)


def test_headers_and_binding_agree():
    text, host = _header(), _header(HOST_HEADER)
    assert sorted(_declared(host)) == sorted(HOST_NAMES) == sorted(capi.VERTICAL_PLAN_HOST_SYMBOLS)
    assert sorted(n for n in _declared(text) if n.startswith("fimex_amd_vertical_plan_")) == sorted(DEVICE_NAMES)
    assert set(DEVICE_NAMES) <= set(capi.SYMBOLS) and not set(HOST_NAMES) & set(capi.SYMBOLS)
    body = re.search(r"typedef struct fimex_amd_vertical_info \{(.*?)\} fimex_amd_vertical_info;", text, flags=re.S).group(1)
    fields = [f for decl in body.split(";") for f in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert fields == [name for name, _ in capi.VerticalInfo._fields_]
    for name in DEVICE_NAMES + HOST_NAMES:
        table = capi.VERTICAL_PLAN_HOST_SYMBOLS if name in HOST_NAMES else capi.SYMBOLS
        args = re.search(r"\b%s\s*\((.*?)\)" % name, host if name in HOST_NAMES else text, flags=re.S).group(1)
        assert len(args.split(",")) == len(table[name][1]), name


def test_host_header_is_plain_c(tmp_path):
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\nint main(void){fimex_amd_vertical_info i; i.nzo = 0; return (int)i.nzo;}\n' % HOST_HEADER)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def _axis(n=3):
    return capi.VerticalLevels.from_axis(np.arange(1., n + 1))


def _create(device, method, inLevels, outLevels=None, level1=None, **kw):
    return capi.VerticalPlan(method, NX, NY, NT, inLevels, outLevels, level1, device=device, **kw)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_bad_plans_are_refused_without_a_device(device):
    ps = np.full((NT, NY, NX), 1000., np.float32)
    l1 = [1.5, 2.5]

    def refused(match, *args, **kw):
        with pytest.raises(capi.FimexAmdError, match=match):
            _create(device, *args, **kw)

    refused("unknown vertical interpolation method 7", 7, _axis(), None, l1)
    refused("unknown vertical interpolation method -1", -1, _axis(), None, l1)
    refused("unknown vertical level kind 5", capi.VINT_METHOD_LIN, capi.VerticalLevels(5, 3, axis=[1., 2., 3.]), None, l1)
    refused("unknown vertical level kind -1", capi.VINT_METHOD_LIN, _axis(), capi.VerticalLevels(-1, 2), None)
    # NULL where the kind needs an array
    for bad in (capi.VerticalLevels(capi.VLEVEL_AXIS, 3), capi.VerticalLevels(capi.VLEVEL_FIELD, 3), capi.VerticalLevels(capi.VLEVEL_SIGMA, 3, ps=ps),
                capi.VerticalLevels(capi.VLEVEL_SIGMA, 3, sigma=[.1, .5, 1.]), capi.VerticalLevels(capi.VLEVEL_HYBRID_SIGMA, 3, a=[1., 2., 3.], ps=ps),
                capi.VerticalLevels(capi.VLEVEL_HYBRID_SIGMA_AP, 3, b=[1., 2., 3.], ps=ps),
                capi.VerticalLevels(capi.VLEVEL_HYBRID_SIGMA_AP, 3, ap=[1., 2., 3.], b=[0., 0., 0.])):
        refused("needs", capi.VINT_METHOD_LIN, bad, None, l1)
        refused("needs", capi.VINT_METHOD_LOG, _axis(), bad, None)
    refused("level1", capi.VINT_METHOD_LIN, _axis(), None, None)
    refused("nzi == 0", capi.VINT_METHOD_LIN, capi.VerticalLevels(capi.VLEVEL_AXIS, 0), None, l1)
    refused("nzo == 0", capi.VINT_METHOD_LIN, _axis(), None, [])
    refused("nzi > 65535", capi.VINT_METHOD_NN, _axis(65536), None, l1)


def test_nzo_must_be_the_templates():
    lib = capi.load()
    plan = ctypes.c_void_p()
    rc = lib.fimex_amd_vertical_plan_create_host(capi.VINT_METHOD_LIN, NX, NY, NT, ctypes.byref(_axis().struct), ctypes.byref(_axis(2).struct), None, 3,
                                                 None, None, ctypes.byref(plan))
    assert rc == capi.ERROR and "nzo differs from the template's number of levels" in lib.fimex_amd_last_error().decode()


def test_null_arguments_are_refused_without_a_device():
    lib = capi.load()
    info, plan = capi.VerticalInfo(), ctypes.c_void_p()

    def refused(rc, match):
        assert rc == capi.ERROR and re.search(match, lib.fimex_amd_last_error().decode()), lib.fimex_amd_last_error().decode()

    axis = _axis()
    l1 = (ctypes.c_double * 2)(1.5, 2.5)
    refused(lib.fimex_amd_vertical_plan_create_device(0, NX, NY, NT, ctypes.byref(axis.struct), None, l1, 2, None, None, None, None), "NULL argument")
    refused(lib.fimex_amd_vertical_plan_create_host(0, NX, NY, NT, ctypes.byref(axis.struct), None, l1, 2, None, None, None), "NULL argument")
    refused(lib.fimex_amd_vertical_plan_create_device(0, NX, NY, NT, None, None, l1, 2, None, None, None, ctypes.byref(plan)),
            "NULL input level description")
    refused(lib.fimex_amd_vertical_plan_info(None, ctypes.byref(info)), "NULL argument")
    one = (ctypes.c_void_p * 1)(1)  # 1 is no pointer: the plan is looked at first
    bad, lim = (ctypes.c_double * 1)(0.0), (ctypes.c_float * 1)(0.0)
    refused(lib.fimex_amd_vertical_plan_apply_device(None, 1, one, capi.CDM_SHORT, bad, lim, lim, one, None), "NULL vertical plan")
    refused(lib.fimex_amd_vertical_plan_apply_host(None, 1, one, capi.CDM_SHORT, bad, lim, lim, one), "NULL vertical plan")
    refused(lib.fimex_amd_vertical_plan_read_host(None, None, None, None), "NULL vertical plan")
    assert lib.fimex_amd_vertical_plan_destroy(None) == capi.OK


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_without_a_device_a_valid_create_fails_loudly(device):
    """No CPU fallback: a plan lives on a gfx950 device; with one, the same call succeeds."""
    field = np.ones((NT, 3, NY, NX), np.float32)
    if capi.device_count() > 0:
        plan = _create(False, capi.VINT_METHOD_LIN, _axis(), None, [1.5, 2.5])
        assert (plan.info.nzi, plan.info.nzo, plan.info.entryBytes) == (3, 2, NX * NY * NT * 2 * 8)
        return
    with pytest.raises(capi.FimexAmdError, match="no HIP device|gfx950"):
        _create(device, capi.VINT_METHOD_LIN, _axis(), None, [1.5, 2.5])
    if not device:
        with pytest.raises(capi.FimexAmdError, match="no HIP device|gfx950"):
            _create(device, capi.VINT_METHOD_LOG, capi.VerticalLevels.from_field(field, 3), _axis(2), None)
