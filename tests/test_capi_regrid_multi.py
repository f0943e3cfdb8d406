"""A list of variables regridded in one call at the C boundary (fimex_amd_regrid_apply_multi_device / _typed_device and their *_host
forms): both libraries export the four symbols, headers and binding agree (the host forms have a header and a table of their own, as
the other late *_host entries have), the host header is plain C, empty lists are answered without a device, and what can be refused
without one is refused with a message.  CPU only: nothing is computed.  (The refusals that look into a plan -- overlapping buffers
-- are in tests/test_gpu_regrid_multi.py: a plan cannot be made without a device.)"""
import ctypes
import os
import re
import subprocess

from fimex_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = ["fimex_amd_regrid_apply_multi_device", "fimex_amd_regrid_apply_multi_typed_device"]
HOST = ["fimex_amd_regrid_apply_multi_host", "fimex_amd_regrid_apply_multi_typed_host"]
HOST_HEADER = "fimex_amd_regrid_multi_host.h"
I, V, Z, D = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double)
VP, ZP, IP = ctypes.POINTER(V), ctypes.POINTER(Z), ctypes.POINTER(ctypes.c_int)


def _header(name="fimex_amd.h"):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared(name, header):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(header), flags=re.S)
    assert m, name + " is not declared"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_both_libraries_export_the_symbols():
    for path in (capi.LIB_PATH, capi.TUNING_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in DEVICE + HOST:
            assert hasattr(lib, name), "missing export in %s: %s" % (os.path.basename(path), name)


def test_header_and_binding_agree():
    assert _declared(DEVICE[0], "fimex_amd.h") == ["const fimex_amd_regrid_plan* plan", "size_t nvar", "const float* const* d_in", "const size_t* nz",
                                                   "float* const* d_out", "void* stream", "int* path"]
    assert _declared(DEVICE[1], "fimex_amd.h") == ["const fimex_amd_regrid_plan* plan", "size_t nvar", "const void* const* d_in", "int cdmType",
                                                   "const size_t* nz", "const double* badValue", "void* const* d_out", "void* stream", "int* path"]
    assert _declared(HOST[0], HOST_HEADER) == ["const fimex_amd_regrid_plan* plan", "size_t nvar", "const float* const* in", "const size_t* nz",
                                               "float* const* out", "int* path"]
    assert _declared(HOST[1], HOST_HEADER) == ["const fimex_amd_regrid_plan* plan", "size_t nvar", "const void* const* in", "int cdmType",
                                               "const size_t* nz", "const double* badValue", "void* const* out", "int* path"]
    assert capi.SYMBOLS[DEVICE[0]] == (I, [V, Z, VP, ZP, VP, V, IP])
    assert capi.SYMBOLS[DEVICE[1]] == (I, [V, Z, VP, I, ZP, D, VP, V, IP])
    assert capi.REGRID_MULTI_HOST_SYMBOLS == {HOST[0]: (I, [V, Z, VP, ZP, VP, IP]), HOST[1]: (I, [V, Z, VP, I, ZP, D, VP, IP])}
    assert re.findall(r"\b(fimex_amd_[a-z0-9_]+)\s*\(", _header(HOST_HEADER)) == HOST and not set(HOST) & set(capi.SYMBOLS)
    m = re.search(r"#define\s+FIMEX_AMD_REGRID_MULTI_MAX_VARS\s+(\d+)", _header())
    assert m and int(m.group(1)) == capi.REGRID_MULTI_MAX_VARS == 64
    assert callable(capi.RegridPlan.apply_multi_device) and callable(capi.RegridPlan.apply_multi_host)


def test_host_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\nint main(void){return FIMEX_AMD_REGRID_MULTI_MAX_VARS > 0 && FIMEX_AMD_OK == 1 ? 0 : 1;}\n' % HOST_HEADER)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def _calls(lib, plan, n, ins, nz, bad, outs, path):
    """the four entries on one list; cdmType 2: short"""
    p = ctypes.byref(path) if path is not None else None
    return [lambda: lib.fimex_amd_regrid_apply_multi_device(plan, n, ins, nz, outs, None, p),
            lambda: lib.fimex_amd_regrid_apply_multi_typed_device(plan, n, ins, 2, nz, bad, outs, None, p),
            lambda: lib.fimex_amd_regrid_apply_multi_host(plan, n, ins, nz, outs, p),
            lambda: lib.fimex_amd_regrid_apply_multi_typed_host(plan, n, ins, 2, nz, bad, outs, p)]


def test_empty_lists_are_answered_without_a_device():
    lib = capi.load()
    one = 1  # no plan behind it: an empty list must not make the entry look at the plan, let alone at a device
    three = (V * 3)(None, None, None)
    zeros, bad = (Z * 3)(0, 0, 0), (ctypes.c_double * 3)(0, 0, 0)
    for call in _calls(lib, one, 0, None, None, None, None, None):
        assert call() == capi.OK, lib.fimex_amd_last_error().decode()
    path = ctypes.c_int(7)
    for call in _calls(lib, one, 3, three, zeros, bad, three, path):
        path.value = 7
        assert call() == capi.OK, lib.fimex_amd_last_error().decode()
        assert path.value == 0


def test_null_arguments_are_refused_without_a_device():
    lib = capi.load()

    def refused(rc, match):
        msg = lib.fimex_amd_last_error().decode()
        assert rc == capi.ERROR and re.search(match, msg), msg

    one = 1
    buf = (ctypes.c_float * 4)()
    here = ctypes.addressof(buf)
    nz, bad = (Z * 2)(1, 1), (ctypes.c_double * 2)(0, 0)
    full = (V * 2)(here, here)
    path = ctypes.c_int(7)
    for call in _calls(lib, None, 2, full, nz, bad, full, path):
        path.value = 7
        refused(call(), "NULL plan")
        assert path.value == 0
    for call in _calls(lib, one, 2, None, nz, bad, full, None) + _calls(lib, one, 2, full, None, bad, full, None) + \
            _calls(lib, one, 2, full, nz, bad, None, None):
        refused(call(), "NULL argument")
    for call in _calls(lib, one, 2, full, nz, None, full, None)[1::2]:
        refused(call(), "NULL argument")
    # a NULL entry of a variable that has slices, in either table
    hole = (V * 2)(here, None)
    for call in _calls(lib, one, 2, hole, nz, bad, full, None) + _calls(lib, one, 2, full, nz, bad, hole, None):
        refused(call(), "NULL buffer of variable 1")
    refused(lib.fimex_amd_regrid_apply_multi_typed_device(one, 2, full, 6, nz, bad, full, None, None), "")  # CDM_STRING: no float form


def test_abi_version_is_unchanged():
    assert capi.load().fimex_amd_abi_version() == 131
