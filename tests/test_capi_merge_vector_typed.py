"""Grid merging of an x/y vector pair in its stored types at the C boundary: both libraries export the three symbols, headers and
bindings agree (the host form has a header and a table of its own, as the other late *_host entries have), and what can be refused
without a device is refused with a message before one is touched.  CPU only: nothing is computed.  (The refusals that look into a
plan -- a vector plan on the wrong grid, overlapping buffers -- are in tests/test_gpu_merge_vector_typed.py: a plan cannot be made
without a device.)"""
import ctypes
import os
import re

from fimex_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED, CHAIN = "fimex_amd_merge_apply_vector_typed_device", "fimex_amd_merge_apply_vector_typed_chain_device"
HOST = "fimex_amd_merge_apply_vector_typed_host"
HOST_HEADER = "fimex_amd_merge_vector_typed_host.h"
V, Z, I, PK = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(capi.Packing)
CDM_NAT, CDM_STRING = 0, 6  # fimex_amd_datatype's two members without an element size


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
        for name in (FUSED, CHAIN, HOST):
            assert hasattr(lib, name), "missing export in %s: %s" % (os.path.basename(path), name)


def test_headers_and_bindings_agree():
    plans = ["const fimex_amd_merge_plan* plan", "const fimex_amd_vector_plan* outerToInnerVec", "const fimex_amd_vector_plan* innerToTargetVec",
             "const fimex_amd_vector_plan* outerToTargetVec"]

    def buffers(prefix):
        fields = [a for n in ("innerU", "innerV", "outerU", "outerV") for a in ("const void* %s%s" % (prefix, n), "const fimex_amd_packing* %sPacking" % n)]
        return fields + ["size_t nz", "void* %soutU" % prefix, "void* %soutV" % prefix]

    fields = [V, PK] * 4
    assert _declared(FUSED, "fimex_amd.h") == plans + buffers("d_") + ["void* stream", "int* path"]
    assert capi.SYMBOLS[FUSED] == (I, [V] * 4 + fields + [Z, V, V, V, ctypes.POINTER(I)])
    assert _declared(CHAIN, "fimex_amd.h") == plans + buffers("d_") + ["void* stream"]
    assert capi.SYMBOLS[CHAIN] == (I, [V] * 4 + fields + [Z, V, V, V])
    assert _declared(HOST, HOST_HEADER) == plans + buffers("")
    assert capi.MERGE_VECTOR_TYPED_HOST_SYMBOLS == {HOST: (I, [V] * 4 + fields + [Z, V, V])}
    assert re.findall(r"\b(fimex_amd_[a-z0-9_]+)\s*\(", _header(HOST_HEADER)) == [HOST] and HOST not in capi.SYMBOLS
    for fn in (capi.MergePlan.apply_vector_typed_device, capi.MergePlan.apply_vector_typed_chain_device, capi.MergePlan.apply_vector_typed_host):
        assert callable(fn)


def test_host_header_is_plain_c(tmp_path):
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\nint main(void){int (*f)(const fimex_amd_merge_plan*, const fimex_amd_vector_plan*, const fimex_amd_vector_plan*, '
                   'const fimex_amd_vector_plan*, const void*, const fimex_amd_packing*, const void*, const fimex_amd_packing*, const void*, '
                   'const fimex_amd_packing*, const void*, const fimex_amd_packing*, size_t, void*, void*) = '
                   'fimex_amd_merge_apply_vector_typed_host; return f != 0 && FIMEX_AMD_OK == 1 ? 0 : 1;}\n' % HOST_HEADER)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_null_and_empty_refusals_arrive_without_a_device():
    lib = capi.load()

    def refused(rc, match):
        msg = lib.fimex_amd_last_error().decode()
        assert rc == capi.ERROR and re.search(match, msg), msg

    one = 1  # no pointer: these checks come before anything is looked at
    short = capi.Packing(capi.CDM_SHORT, -32768.0, 0.01, 0.0)
    fused_d, chain_d, host = (getattr(lib, n) for n in (FUSED, CHAIN, HOST))
    path = ctypes.c_int(7)

    def call(fn, plans, bufs, packings, nz=1):
        fields = [a for b, p in zip(bufs[:4], packings) for a in (b, ctypes.byref(p) if p is not None else None)]
        tail = [None, ctypes.byref(path)] if fn is fused_d else [None] if fn is chain_d else []
        return fn(*plans, *fields, nz, *bufs[4:], *tail)

    all_plans, all_bufs, all_packings = [one] * 4, [one] * 6, [short] * 4
    for fn in (fused_d, chain_d, host):
        refused(call(fn, [None, one, one, one], all_bufs, all_packings), "NULL plan")
        for hole in (1, 2, 3):  # an interpolator without a rotation is not served here
            plans = [None if k == hole else one for k in range(4)]
            refused(call(fn, plans, all_bufs, all_packings), "NULL vector plan")
            refused(call(fn, plans, all_bufs, all_packings, nz=0), "NULL vector plan")
        for hole in range(4):
            packings = [None if k == hole else short for k in range(4)]
            refused(call(fn, all_plans, all_bufs, packings), "NULL packing")
            refused(call(fn, all_plans, all_bufs, packings, nz=0), "NULL packing")
            for bad in (CDM_NAT, CDM_STRING):  # types without element size
                packings = [capi.Packing(bad, 0.0, 1.0, 0.0) if k == hole else short for k in range(4)]
                refused(call(fn, all_plans, all_bufs, packings), r"data type %d cannot be regridded \(CDM_STRING / CDM_NAT" % bad)
        for hole in (0, 1):  # an inner fill value that its type cannot hold; an outer one only sends the call to the chain
            packings = [capi.Packing(capi.CDM_SHORT, 40000.0, 0.01, 0.0) if k == hole else short for k in range(4)]
            refused(call(fn, all_plans, all_bufs, packings), "not representable")
        for hole in range(6):  # a NULL buffer with nz > 0
            bufs = [None if k == hole else one for k in range(6)]
            refused(call(fn, all_plans, bufs, all_packings), "NULL data buffer")
        # nothing to do is no error, with or without buffers
        assert call(fn, all_plans, [None] * 6, all_packings, nz=0) == capi.OK
        assert call(fn, all_plans, all_bufs, all_packings, nz=0) == capi.OK
    assert path.value == 0  # written as 0 before any check


def test_abi_version_is_unchanged():
    assert capi.load().fimex_amd_abi_version() == 131
