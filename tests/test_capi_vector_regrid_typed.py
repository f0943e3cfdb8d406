"""The regrid of a vector pair in its stored types at the C boundary (fimex_amd_regrid_apply_vector_typed_device / _host): both
libraries export the two symbols, headers and binding agree (the host form has a header and a table of its own, as the other late
*_host entries have), and what can be refused without a device is refused with a message before one is touched.  CPU only: nothing
is computed.  (The refusals that look into a plan -- a forward plan, a vector plan on another grid, overlapping buffers -- are in
tests/test_gpu_vector_regrid_typed.py: a plan cannot be made without a device.)"""
import ctypes
import os
import re

from fimex_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE, HOST = "fimex_amd_regrid_apply_vector_typed_device", "fimex_amd_regrid_apply_vector_typed_host"
V, Z, I, D = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double
HOST_HEADER = "fimex_amd_vector_regrid_typed_host.h"
SHORT = 2  # CDM_SHORT


def _header(name="fimex_amd.h"):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_both_libraries_export_the_symbols():
    for path in (capi.LIB_PATH, capi.TUNING_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in (DEVICE, HOST):
            assert hasattr(lib, name), "missing export in %s: %s" % (os.path.basename(path), name)


def test_header_and_binding_agree():
    declared = {}
    for name in (DEVICE, HOST):
        text = _header(HOST_HEADER if name == HOST else "fimex_amd.h")
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
        assert m, name + " is not declared"
        declared[name] = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert declared[DEVICE] == ["const fimex_amd_regrid_plan* plan", "const fimex_amd_vector_plan* vec", "const void* d_u", "int uType",
                                "double uBad", "const void* d_v", "int vType", "double vBad", "size_t nz", "void* d_uOut", "void* d_vOut",
                                "void* stream", "int* path"]
    assert declared[HOST] == ["const fimex_amd_regrid_plan* plan", "const fimex_amd_vector_plan* vec", "const void* u", "int uType",
                              "double uBad", "const void* v", "int vType", "double vBad", "size_t size", "void* uOut", "void* vOut",
                              "size_t outCapacity", "size_t* newSize"]
    assert capi.SYMBOLS[DEVICE] == (I, [V, V, V, I, D, V, I, D, Z, V, V, V, ctypes.POINTER(I)])
    assert capi.VECTOR_REGRID_TYPED_HOST_SYMBOLS == {HOST: (I, [V, V, V, I, D, V, I, D, Z, V, V, Z, ctypes.POINTER(Z)])}
    assert re.findall(r"\b(fimex_amd_[a-z0-9_]+)\s*\(", _header(HOST_HEADER)) == [HOST] and HOST not in capi.SYMBOLS
    assert callable(capi.RegridPlan.apply_vector_typed_device) and callable(capi.RegridPlan.apply_vector_typed_host)


def test_host_header_is_plain_c(tmp_path):
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\nint main(void){return FIMEX_AMD_OK == 1 ? 0 : 1;}\n' % HOST_HEADER)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_null_arguments_are_refused_without_a_device():
    lib = capi.load()

    def refused(rc, match):
        msg = lib.fimex_amd_last_error().decode()
        assert rc == capi.ERROR and re.search(match, msg), msg

    one = 1  # no pointer: the NULL checks come before anything is looked at
    buf = (ctypes.c_short * 4)()
    path, n = ctypes.c_int(7), ctypes.c_size_t(0)
    device, host = lib.fimex_amd_regrid_apply_vector_typed_device, lib.fimex_amd_regrid_apply_vector_typed_host
    refused(device(None, one, one, SHORT, 0.0, one, SHORT, 0.0, 1, one, one, None, ctypes.byref(path)), "NULL regrid plan")
    assert path.value == 0
    path.value = 7
    refused(device(one, None, one, SHORT, 0.0, one, SHORT, 0.0, 1, one, one, None, ctypes.byref(path)), "NULL vector plan")
    assert path.value == 0
    for hole in range(4):
        ptrs = [None if k == hole else one for k in range(4)]
        path.value = 7
        refused(device(one, one, ptrs[0], SHORT, 0.0, ptrs[1], SHORT, 0.0, 1, ptrs[2], ptrs[3], None, ctypes.byref(path)), "NULL device buffer")
        assert path.value == 0
    for bad_type in (0, 6):  # CDM_NAT, CDM_STRING: no element size
        assert device(one, one, one, bad_type, 0.0, one, SHORT, 0.0, 1, one, one, None, None) == capi.ERROR
        assert device(one, one, one, SHORT, 0.0, one, bad_type, 0.0, 1, one, one, None, None) == capi.ERROR
        assert host(one, one, buf, SHORT, 0.0, buf, bad_type, 0.0, 4, buf, buf, 4, ctypes.byref(n)) == capi.ERROR
    refused(host(None, one, buf, SHORT, 0.0, buf, SHORT, 0.0, 4, buf, buf, 4, ctypes.byref(n)), "NULL regrid plan")
    refused(host(one, None, buf, SHORT, 0.0, buf, SHORT, 0.0, 4, buf, buf, 4, ctypes.byref(n)), "NULL vector plan")
    refused(host(one, one, buf, SHORT, 0.0, buf, SHORT, 0.0, 4, buf, buf, 4, None), "NULL argument")


def test_abi_version_is_unchanged():
    assert capi.load().fimex_amd_abi_version() == 131
