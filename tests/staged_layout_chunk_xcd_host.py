"""The chunk-per-XCD launch order of fimex_amd/csrc/staged_layout.hpp on the CPU: tests/staged_layout_chunk_xcd_host.cc compiled with
g++ into a temporary directory and called through ctypes (as tests/staged_layout_host.py does for the rest of that header).
tests/test_staged_layout_chunk_xcd.py and scripts/model_fetch.py use it."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMAX = 31  # kMaxZChunks
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    d = tempfile.mkdtemp(prefix="staged_layout_chunk_xcd_")
    so = os.path.join(d, "libstaged_layout_chunk_xcd_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "fimex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "staged_layout_chunk_xcd_host.cc"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    u32, u64, ptr = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    lib.scx_order.argtypes = [u64, ptr, ptr, ptr, u32, u32, u32, ptr, ptr]
    lib.scx_order.restype = None
    lib.scx_decode.argtypes = [u32, u32, u32, ptr, ptr]
    lib.scx_decode.restype = None
    lib.scx_chunk_count.argtypes = [u64, u32]
    lib.scx_chunk_count.restype = u32
    lib.scx_launch_order.argtypes = [ctypes.c_int, ctypes.c_int, u64, u32]
    lib.scx_launch_order.restype = ctypes.c_int
    lib.scx_z_chunks.argtypes = [u64, ctypes.c_int, u32, ptr, ptr]
    lib.scx_z_chunks.restype = ctypes.c_int
    _lib = lib
    return lib


def order_of(lib, x0, w, band, tileW, by, bx):
    """chunk_xcd_order of tiles (x0, w, band): the table every XCD walks and the cohort of every entry"""
    x0, w, band = (np.ascontiguousarray(v, dtype=np.uint32) for v in (x0, w, band))
    order, cohort = np.zeros(len(x0), np.uint32), np.zeros(len(x0), np.uint32)
    lib.scx_order(len(x0), x0.ctypes.data, w.ctypes.data, band.ctypes.data, tileW, by, bx, order.ctypes.data, cohort.ctypes.data)
    return order.astype(np.int64), cohort.astype(np.int64)


def decode(lib, grid, n, mode):
    """(slot, z chunk) of every workgroup of a flat grid; mode 1: chunk-per-XCD, 0: tile-major"""
    slot, zc = np.zeros(grid, np.uint32), np.zeros(grid, np.uint32)
    lib.scx_decode(grid, n, mode, slot.ctypes.data, zc.ctypes.data)
    return slot.astype(np.int64), zc.astype(np.int64)


def z_chunks(lib, nz, order, zpb):
    """float_z_chunks: (ok, zStart, n)"""
    zs, n = np.zeros(KMAX + 1, np.uint32), ctypes.c_uint32(0)
    ok = lib.scx_z_chunks(nz, order, zpb, zs.ctypes.data, ctypes.byref(n))
    return ok, zs.astype(np.int64), int(n.value)
