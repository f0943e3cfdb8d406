"""Grid merging on stored types at the C boundary: both libraries export the seven symbols, headers and bindings agree (the host
forms have a header and a table of their own, as the other late *_host entries have), and what can be refused without a device is
refused with a message before one is touched.  CPU only: nothing is computed.  (The refusals that look into a plan -- overlapping
buffers, an output fill value the type does not hold -- are in tests/test_gpu_merge_typed.py: a plan cannot be made without a
device.)"""
import ctypes
import os
import re

from fimex_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = ["fimex_amd_border_smooth_typed_device", "fimex_amd_overlay_typed_device", "fimex_amd_merge_apply_typed_device",
          "fimex_amd_merge_apply_typed_chain_device"]
HOST = ["fimex_amd_border_smooth_typed_host", "fimex_amd_overlay_typed_host", "fimex_amd_merge_apply_typed_host"]
HOST_HEADER = "fimex_amd_merge_typed_host.h"
V, Z, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
P = ctypes.POINTER(capi.Packing)
SHORT = 2  # CDM_SHORT


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


def test_headers_and_bindings_agree():
    smooth = ["const void* %s", "const fimex_amd_packing* innerPacking", "const void* %s", "const fimex_amd_packing* outerPacking", "void* %s",
              "size_t nx", "size_t ny", "size_t nz", "size_t transitionWidth", "size_t borderWidth", "int useOuterIfInnerUndefined"]
    overlay = ["const void* %s", "const fimex_amd_packing* topPacking", "const void* %s", "const fimex_amd_packing* basePacking", "void* %s",
               "size_t n"]
    merge = ["const fimex_amd_merge_plan* plan", "const void* %s", "const fimex_amd_packing* innerPacking", "const void* %s",
             "const fimex_amd_packing* outerPacking", "size_t nz", "void* %s"]

    def named(args, names):
        it = iter(names)
        return [a % next(it) if "%s" in a else a for a in args]

    assert _declared(DEVICE[0], "fimex_amd.h") == named(smooth, ["d_inner", "d_outerOnInner", "d_out"]) + ["void* stream"]
    assert _declared(DEVICE[1], "fimex_amd.h") == named(overlay, ["d_top", "d_base", "d_out"]) + ["void* stream"]
    assert _declared(DEVICE[2], "fimex_amd.h") == named(merge, ["d_inner", "d_outer", "d_out"]) + ["void* stream", "int* path"]
    assert _declared(DEVICE[3], "fimex_amd.h") == named(merge, ["d_inner", "d_outer", "d_out"]) + ["void* stream"]
    assert _declared(HOST[0], HOST_HEADER) == named(smooth, ["inner", "outerOnInner", "out"])
    assert _declared(HOST[1], HOST_HEADER) == named(overlay, ["top", "base", "out"])
    assert _declared(HOST[2], HOST_HEADER) == named(merge, ["inner", "outer", "out"])
    assert capi.SYMBOLS[DEVICE[0]] == (I, [V, P, V, P, V, Z, Z, Z, Z, Z, I, V])
    assert capi.SYMBOLS[DEVICE[1]] == (I, [V, P, V, P, V, Z, V])
    assert capi.SYMBOLS[DEVICE[2]] == (I, [V, V, P, V, P, Z, V, V, ctypes.POINTER(I)])
    assert capi.SYMBOLS[DEVICE[3]] == (I, [V, V, P, V, P, Z, V, V])
    assert capi.MERGE_TYPED_HOST_SYMBOLS == {HOST[0]: (I, [V, P, V, P, V, Z, Z, Z, Z, Z, I]), HOST[1]: (I, [V, P, V, P, V, Z]),
                                             HOST[2]: (I, [V, V, P, V, P, Z, V])}
    assert re.findall(r"\b(fimex_amd_[a-z0-9_]+)\s*\(", _header(HOST_HEADER)) == HOST and not set(HOST) & set(capi.SYMBOLS)
    # the struct as the header lays it out
    m = re.search(r"typedef struct fimex_amd_packing \{(.*?)\} fimex_amd_packing;", _header(), flags=re.S)
    assert m and [re.sub(r"\s+", " ", f).strip() for f in m.group(1).split(";") if f.strip()] == ["int type", "double fill", "double scale",
                                                                                                   "double offset"]
    assert [(n, t) for n, t in capi.Packing._fields_] == [("type", I), ("fill", ctypes.c_double), ("scale", ctypes.c_double),
                                                          ("offset", ctypes.c_double)]
    for fn in (capi.border_smooth_typed_device, capi.border_smooth_typed_host, capi.overlay_typed_device, capi.overlay_typed_host,
               capi.MergePlan.apply_typed_device, capi.MergePlan.apply_typed_chain_device, capi.MergePlan.apply_typed_host):
        assert callable(fn)


def test_host_header_is_plain_c(tmp_path):
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\nint main(void){fimex_amd_packing p = {2, -32768.0, 0.01, 273.15}; return p.type == 2 && FIMEX_AMD_OK == 1 ? 0 : 1;}\n'
                   % HOST_HEADER)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_null_and_type_refusals_arrive_without_a_device():
    lib = capi.load()

    def refused(rc, match):
        msg = lib.fimex_amd_last_error().decode()
        assert rc == capi.ERROR and re.search(match, msg), msg

    one = 1  # no pointer: these checks come before anything is looked at
    buf = (ctypes.c_short * 4)()
    ok = ctypes.byref(capi.Packing(SHORT, -32768.0, 0.01, 273.15))
    smooth_d, overlay_d = lib.fimex_amd_border_smooth_typed_device, lib.fimex_amd_overlay_typed_device
    merge_d, chain_d = lib.fimex_amd_merge_apply_typed_device, lib.fimex_amd_merge_apply_typed_chain_device
    smooth_h, overlay_h, merge_h = lib.fimex_amd_border_smooth_typed_host, lib.fimex_amd_overlay_typed_host, lib.fimex_amd_merge_apply_typed_host
    path = ctypes.c_int(7)

    # NULL plan, NULL packings
    refused(merge_d(None, one, ok, one, ok, 1, one, None, ctypes.byref(path)), "NULL plan")
    assert path.value == 0
    refused(chain_d(None, one, ok, one, ok, 1, one, None), "NULL plan")
    refused(merge_h(None, buf, ok, buf, ok, 1, buf), "NULL plan")
    for a, b in ((None, ok), (ok, None)):
        path.value = 7
        refused(merge_d(one, one, a, one, b, 1, one, None, ctypes.byref(path)), "NULL packing")
        assert path.value == 0
        refused(chain_d(one, one, a, one, b, 1, one, None), "NULL packing")
        refused(merge_h(one, buf, a, buf, b, 1, buf), "NULL packing")
        refused(smooth_d(one, a, one, b, one, 2, 2, 1, 5, 2, 1, None), "NULL packing")
        refused(smooth_h(buf, a, buf, b, buf, 2, 2, 1, 5, 2, 1), "NULL packing")
        refused(overlay_d(one, a, one, b, one, 4, None), "NULL packing")
        refused(overlay_h(buf, a, buf, b, buf, 4), "NULL packing")
    # types without element size, on either side
    for bad_type in (0, 6):  # CDM_NAT, CDM_STRING
        bad = ctypes.byref(capi.Packing(bad_type, 0.0, 1.0, 0.0))
        for a, b in ((bad, ok), (ok, bad)):
            assert merge_d(one, one, a, one, b, 1, one, None, None) == capi.ERROR
            assert chain_d(one, one, a, one, b, 1, one, None) == capi.ERROR
            assert merge_h(one, buf, a, buf, b, 1, buf) == capi.ERROR
            assert smooth_d(one, a, one, b, one, 2, 2, 1, 5, 2, 1, None) == capi.ERROR
            assert smooth_h(buf, a, buf, b, buf, 2, 2, 1, 5, 2, 1) == capi.ERROR
            assert overlay_d(one, a, one, b, one, 4, None) == capi.ERROR
            assert overlay_h(buf, a, buf, b, buf, 4) == capi.ERROR
    # an output fill value that the inner's type does not hold
    wide = ctypes.byref(capi.Packing(SHORT, 1e9, 1.0, 0.0))
    refused(overlay_d(one, wide, one, ok, one, 4, None), "not representable")
    refused(smooth_h(buf, wide, buf, ok, buf, 2, 2, 1, 5, 2, 1), "not representable")
    refused(merge_d(one, one, wide, one, ok, 1, one, None, None), "not representable")
    assert overlay_h(buf, ok, buf, wide, buf, 0) == capi.OK  # the outer's fill value is only read: one the type lacks matches nothing
    # NULL buffers, the smoothing's parameters, overlapping buffers: addresses only
    for hole in range(3):
        ptrs = [None if k == hole else one for k in range(3)]
        refused(merge_d(one, ptrs[0], ok, ptrs[1], ok, 1, ptrs[2], None, None), "NULL data buffer")
        refused(smooth_d(ptrs[0], ok, ptrs[1], ok, ptrs[2], 2, 2, 1, 5, 2, 1, None), "NULL data buffer")
        refused(overlay_d(ptrs[0], ok, ptrs[1], ok, ptrs[2], 4, None), "NULL data buffer")
    refused(smooth_d(one, ok, one, ok, one, 2, 2, 1, 0, 2, 1, None), "transitionWidth == 0")
    refused(smooth_d(one, ok, one, ok, one, 0, 2, 1, 5, 2, 1, None), "empty grid")
    base = ctypes.addressof(buf)
    refused(overlay_h(base, ok, base + 16, ok, base + 2, 4), "overlaps")
    as_int = ctypes.byref(capi.Packing(3, -1.0, 1.0, 0.0))  # CDM_INT against short: in place on the base needs one element size
    refused(overlay_d(4096, as_int, 8192, ok, 8192, 4, None), "overlaps")
    # nothing to do is no error
    assert overlay_d(None, ok, None, ok, None, 0, None) == capi.OK
    assert smooth_d(None, ok, None, ok, None, 2, 2, 0, 5, 2, 1, None) == capi.OK
    assert merge_d(one, None, ok, None, ok, 0, None, None, ctypes.byref(path)) == capi.OK and path.value == 0


def test_abi_version_is_unchanged():
    assert capi.load().fimex_amd_abi_version() == 131
