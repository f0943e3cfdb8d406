"""fimex_amd/csrc/slice_list.hpp on the CPU: tests/slice_list_host.cc compiled with g++ into a temporary directory and called through
ctypes (the way tests/staged_layout_host.py wraps staged_layout.hpp)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    d = tempfile.mkdtemp(prefix="slice_list_")
    so = os.path.join(d, "libslice_list_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "fimex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "slice_list_host.cc"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    u32, u64, ptr = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    lib.sl_max_vars.argtypes = []
    lib.sl_max_vars.restype = u32
    lib.sl_build.argtypes = [ptr, u64, ptr, ptr, ptr, ptr]
    lib.sl_build.restype = ctypes.c_int
    lib.sl_walk.argtypes = [ptr, u64, u32, u32, u32, ptr, ptr, ptr, ptr, ptr]
    lib.sl_walk.restype = ctypes.c_int
    lib.sl_list_slices.argtypes = [ptr, u64]
    lib.sl_list_slices.restype = u64
    lib.sl_launches.argtypes = [ptr, u64, ptr, ptr, ptr, ctypes.c_int]
    lib.sl_launches.restype = ctypes.c_int
    _lib = lib
    return lib


def build(lib, nz):
    """(accepted, ends, index, total) of the table build_slice_ends makes of nz."""
    nz = np.ascontiguousarray(nz, dtype=np.uint64)
    k = lib.sl_max_vars()
    ends, index = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
    held, total = ctypes.c_uint32(0), ctypes.c_uint64(0)
    ok = lib.sl_build(nz.ctypes.data, len(nz), ends.ctypes.data, index.ctypes.data, ctypes.byref(held), ctypes.byref(total))
    return bool(ok), ends[:held.value].copy(), index[:held.value].copy(), int(total.value)


def list_slices(lib, nz):
    nz = np.ascontiguousarray(nz, dtype=np.uint64)
    return int(lib.sl_list_slices(nz.ctypes.data, len(nz)))


def launches(lib, nz):
    """The launches for_list_launches cuts nz into, as rows of (first, count, whether build_slice_ends takes that run)."""
    nz = np.ascontiguousarray(nz, dtype=np.uint64)
    room = len(nz) + 1
    first, count, ok = np.zeros(room, np.uint64), np.zeros(room, np.uint64), np.zeros(room, np.int32)
    made = lib.sl_launches(nz.ctypes.data, len(nz), first.ctypes.data, count.ctypes.data, ok.ctypes.data, room)
    assert made >= 0
    return [(int(f), int(c), bool(a)) for f, c, a in zip(first[:made], count[:made], ok[:made])]


def walk(lib, nz, z0, z1, depth):
    """One workgroup's walk over [z0, z1): (fetches as rows of (variable, level, trip), slices worked on as rows of (variable, level)),
    or None when a cursor left the list."""
    nz = np.ascontiguousarray(nz, dtype=np.uint64)
    n = z1 - z0
    f = np.full((3, n), -7, np.int32)
    w = np.full((2, n), -7, np.int32)
    got = lib.sl_walk(nz.ctypes.data, len(nz), z0, z1, depth, f[0].ctypes.data, f[1].ctypes.data, f[2].ctypes.data, w[0].ctypes.data,
                      w[1].ctypes.data)
    if got < 0:
        return None
    return f[:, :got].T.copy(), w.T.copy()
