"""include/fimex_amd_derived_host.h, the *_host forms of the (8f n9) entries: the header is plain C, the binding's table names exactly
what it declares, both libraries export it, and every form has a *_device twin in include/fimex_amd.h.  CPU only: nothing is computed."""
import ctypes
import os
import re
import subprocess

from fimex_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fimex_amd_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    declared = _declared("fimex_amd_derived_host.h")
    assert len(declared) == 5 and all(name.endswith("_host") for name in declared)
    assert sorted(capi.DERIVED_HOST_SYMBOLS) == declared
    assert not set(declared) & set(capi.SYMBOLS)
    twins = set(_declared("fimex_amd.h"))
    assert all(name[:-len("_host")] + "_device" in twins for name in declared)


def test_both_libraries_export_the_host_forms():
    for path in (capi.LIB_PATH, capi.TUNING_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in _declared("fimex_amd_derived_host.h"):
            assert hasattr(lib, name), "missing export in %s: %s" % (os.path.basename(path), name)


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "fimex_amd_derived_host.h"\nint main(void){return FIMEX_AMD_OK == 1 ? 0 : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])
