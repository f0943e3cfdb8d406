"""The regrid of a vector pair with its rotation at the C boundary (fimex_amd_regrid_apply_vector_device / _host): both libraries
export the two symbols, headers and binding agree (the host form has a header and a table of its own, as the other late *_host
entries have), and what can be refused without a device is refused with a message before one
is touched.  CPU only: nothing is computed.  (The refusals that look into a plan -- a forward plan, a vector plan on another grid,
overlapping buffers -- are in tests/test_gpu_vector_regrid.py: a plan cannot be made without a device.)"""
import ctypes
import os
import re

from fimex_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE, HOST = "fimex_amd_regrid_apply_vector_device", "fimex_amd_regrid_apply_vector_host"
V, F, Z = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_size_t
HOST_HEADER = "fimex_amd_vector_regrid_host.h"


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
    assert declared[DEVICE] == ["const fimex_amd_regrid_plan* plan", "const fimex_amd_vector_plan* vec", "const float* d_u", "const float* d_v",
                                "size_t nz", "float* d_uOut", "float* d_vOut", "void* stream", "int* path"]
    assert declared[HOST] == ["const fimex_amd_regrid_plan* plan", "const fimex_amd_vector_plan* vec", "const float* u", "const float* v",
                              "size_t size", "float* uOut", "float* vOut", "size_t outCapacity", "size_t* newSize"]
    assert capi.SYMBOLS[DEVICE] == (ctypes.c_int, [V, V, V, V, Z, V, V, V, ctypes.POINTER(ctypes.c_int)])
    assert capi.VECTOR_REGRID_HOST_SYMBOLS == {HOST: (ctypes.c_int, [V, V, F, F, Z, F, F, Z, ctypes.POINTER(Z)])}
    assert re.findall(r"\b(fimex_amd_[a-z0-9_]+)\s*\(", _header(HOST_HEADER)) == [HOST] and HOST not in capi.SYMBOLS
    assert callable(capi.RegridPlan.apply_vector_device) and callable(capi.RegridPlan.apply_vector_host)


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
    buf = (ctypes.c_float * 4)()
    path, n = ctypes.c_int(7), ctypes.c_size_t(0)
    refused(lib.fimex_amd_regrid_apply_vector_device(None, one, one, one, 1, one, one, None, ctypes.byref(path)), "NULL regrid plan")
    assert path.value == 0
    refused(lib.fimex_amd_regrid_apply_vector_device(one, None, one, one, 1, one, one, None, None), "NULL vector plan")
    for hole in range(4):
        ptrs = [None if k == hole else one for k in range(4)]
        refused(lib.fimex_amd_regrid_apply_vector_device(one, one, ptrs[0], ptrs[1], 1, ptrs[2], ptrs[3], None, None), "NULL device buffer")
    refused(lib.fimex_amd_regrid_apply_vector_host(None, one, buf, buf, 4, buf, buf, 4, ctypes.byref(n)), "NULL regrid plan")
    refused(lib.fimex_amd_regrid_apply_vector_host(one, None, buf, buf, 4, buf, buf, 4, ctypes.byref(n)), "NULL vector plan")
    refused(lib.fimex_amd_regrid_apply_vector_host(one, one, buf, buf, 4, buf, buf, 4, None), "NULL argument")


def test_abi_version_is_unchanged():
    assert capi.load().fimex_amd_abi_version() == 131
