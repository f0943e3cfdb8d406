"""Grid merging of an x/y vector pair at the C boundary: both libraries export the three symbols, headers and bindings agree (the
host form has a header and a table of its own, as the other late *_host entries have), and what can be refused without a device is
refused with a message before one is touched.  CPU only: nothing is computed.  (The refusals that look into a plan -- a vector
plan on the wrong grid, overlapping buffers -- are in tests/test_gpu_merge_vector.py: a plan cannot be made without a device.)"""
import ctypes
import os
import re

from fimex_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = ["fimex_amd_merge_apply_vector_device", "fimex_amd_merge_apply_vector_chain_device"]
HOST = ["fimex_amd_merge_apply_vector_host"]
HOST_HEADER = "fimex_amd_merge_vector_host.h"
V, Z, I, F = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_float)


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
    plans = ["const fimex_amd_merge_plan* plan", "const fimex_amd_vector_plan* outerToInnerVec", "const fimex_amd_vector_plan* innerToTargetVec",
             "const fimex_amd_vector_plan* outerToTargetVec"]

    def buffers(prefix):
        return ["const float* %s%s" % (prefix, n) for n in ("innerU", "innerV", "outerU", "outerV")] + ["size_t nz"] + [
            "float* %s%s" % (prefix, n) for n in ("outU", "outV")]

    for name in DEVICE:
        assert _declared(name, "fimex_amd.h") == plans + buffers("d_") + ["void* stream"]
        assert capi.SYMBOLS[name] == (I, [V, V, V, V, V, V, V, V, Z, V, V, V])
    assert _declared(HOST[0], HOST_HEADER) == plans + buffers("")
    assert capi.MERGE_VECTOR_HOST_SYMBOLS == {HOST[0]: (I, [V, V, V, V, F, F, F, F, Z, F, F])}
    assert re.findall(r"\b(fimex_amd_[a-z0-9_]+)\s*\(", _header(HOST_HEADER)) == HOST and not set(HOST) & set(capi.SYMBOLS)
    for fn in (capi.MergePlan.apply_vector_device, capi.MergePlan.apply_vector_chain_device, capi.MergePlan.apply_vector_host):
        assert callable(fn)


def test_host_header_is_plain_c(tmp_path):
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\nint main(void){int (*f)(const fimex_amd_merge_plan*, const fimex_amd_vector_plan*, const fimex_amd_vector_plan*, '
                   'const fimex_amd_vector_plan*, const float*, const float*, const float*, const float*, size_t, float*, float*) = '
                   'fimex_amd_merge_apply_vector_host; return f != 0 && FIMEX_AMD_OK == 1 ? 0 : 1;}\n' % HOST_HEADER)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_null_and_empty_refusals_arrive_without_a_device():
    lib = capi.load()

    def refused(rc, match):
        msg = lib.fimex_amd_last_error().decode()
        assert rc == capi.ERROR and re.search(match, msg), msg

    one = 1  # no pointer: these checks come before anything is looked at
    buf = (ctypes.c_float * 4)()
    fused_d, chain_d, host = (getattr(lib, n) for n in DEVICE + HOST)

    def device(fn, plans, bufs, nz=1):
        return fn(*plans, *bufs[:4], nz, *bufs[4:], None)

    def on_host(plans, bufs, nz=1):
        return host(*plans, *[buf if b else None for b in bufs[:4]], nz, *[buf if b else None for b in bufs[4:]])

    all_plans, all_bufs = [one] * 4, [one] * 6
    for fn in (fused_d, chain_d):
        refused(device(fn, [None, one, one, one], all_bufs), "NULL plan")
    refused(on_host([None, one, one, one], all_bufs), "NULL plan")
    for hole in (1, 2, 3):  # an interpolator without a rotation is not served here
        plans = [None if k == hole else one for k in range(4)]
        for fn in (fused_d, chain_d):
            refused(device(fn, plans, all_bufs), "NULL vector plan")
            refused(device(fn, plans, all_bufs, nz=0), "NULL vector plan")
        refused(on_host(plans, all_bufs), "NULL vector plan")
    for hole in range(6):  # a NULL buffer with nz > 0
        bufs = [None if k == hole else one for k in range(6)]
        for fn in (fused_d, chain_d):
            refused(device(fn, all_plans, bufs), "NULL data buffer")
        refused(on_host(all_plans, bufs), "NULL data buffer")
    # nothing to do is no error, with or without buffers
    for fn in (fused_d, chain_d):
        assert device(fn, all_plans, [None] * 6, nz=0) == capi.OK
        assert device(fn, all_plans, all_bufs, nz=0) == capi.OK
    assert on_host(all_plans, [None] * 6, nz=0) == capi.OK


def test_abi_version_is_unchanged():
    assert capi.load().fimex_amd_abi_version() == 131
