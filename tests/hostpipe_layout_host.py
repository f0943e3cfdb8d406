"""fimex_amd/csrc/hostpipe_layout.hpp on the CPU: tests/hostpipe_layout_host.cc compiled with g++ into a temporary directory and
called through ctypes (the way tests/slice_list_host.py wraps slice_list.hpp).  Sizes travel as (slot, piece, float scratch,
staged-copy threshold) in bytes.  build_copier() compiles tests/hostpipe_copier_main.cc, the stand-alone program that drives the
header's ParallelCopier; it is run as a program, never loaded."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fimex_amd", "csrc")
LIMITS = ("pinned in", "pinned out", "float in", "float out")
PIN_IN, PIN_OUT, FLOAT_IN, FLOAT_OUT = range(4)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    d = tempfile.mkdtemp(prefix="hostpipe_layout_")
    so = os.path.join(d, "libhostpipe_layout_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-pthread", "-I", CSRC,
                    os.path.join(ROOT, "tests", "hostpipe_layout_host.cc"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    u64, ptr = ctypes.c_uint64, ctypes.c_void_p
    lib.hp_constants.argtypes = [ptr]
    lib.hp_constants.restype = None
    lib.hp_refused.argtypes = [ptr]
    lib.hp_refused.restype = ctypes.c_int
    lib.hp_slices_per_chunk.argtypes = [ptr, u64, u64, u64, u64, ptr, ptr]
    lib.hp_slices_per_chunk.restype = u64
    lib.hp_slice_chunks.argtypes = [u64, u64, u64, ptr, ptr]
    lib.hp_slice_chunks.restype = u64
    lib.hp_byte_chunks.argtypes = [ptr, u64, u64, ptr, ptr]
    lib.hp_byte_chunks.restype = u64
    lib.hp_pieces.argtypes = [u64, u64, u64, ptr, ptr]
    lib.hp_pieces.restype = u64
    lib.hp_drain_before.argtypes = [u64, u64, ptr]
    lib.hp_drain_before.restype = ctypes.c_int64
    _lib = lib
    return lib


def _sizes(sizes):
    s = np.ascontiguousarray(sizes, dtype=np.uint64)
    assert s.shape == (4,), s.shape
    return s


def constants(lib):
    """{slot, piece, float, staged_min, slots, pieces}: what the product build works with."""
    out = np.zeros(6, np.uint64)
    lib.hp_constants(out.ctypes.data)
    return dict(zip(("slot", "piece", "float", "staged_min", "slots", "pieces"), (int(v) for v in out)))


def production_sizes(lib):
    c = constants(lib)
    return (c["slot"], c["piece"], c["float"], c["staged_min"])


def refused(lib, sizes):
    return bool(lib.hp_refused(_sizes(sizes).ctypes.data))


def slices_per_chunk(lib, sizes, in_slice_bytes, out_slice_bytes, in_slice_floats, out_slice_floats):
    """(slices per chunk or 0 for "does not fit", the four counts the limits allow, the index of the binding limit)."""
    s, each, binding = _sizes(sizes), np.zeros(4, np.uint64), ctypes.c_int(-1)
    fit = lib.hp_slices_per_chunk(s.ctypes.data, in_slice_bytes, out_slice_bytes, in_slice_floats, out_slice_floats, each.ctypes.data,
                                  ctypes.addressof(binding))
    return int(fit), [int(v) for v in each], binding.value


def _chunks(call, room=4096):
    first, units = np.zeros(room, np.uint64), np.zeros(room, np.uint64)
    n = int(call(room, first.ctypes.data, units.ctypes.data))
    assert n <= room, n
    return [(int(first[c]), int(units[c])) for c in range(n)]


def slice_chunks(lib, nz, fit):
    """[(first slice, slices)] per chunk."""
    return _chunks(lambda room, f, u: lib.hp_slice_chunks(nz, fit, room, f, u))


def byte_chunks(lib, sizes, nbytes):
    """[(first byte, bytes)] per chunk of a plain copy."""
    s = _sizes(sizes)
    return _chunks(lambda room, f, u: lib.hp_byte_chunks(s.ctypes.data, nbytes, room, f, u))


def pieces(lib, nbytes, piece_bytes):
    """[(offset, length)] per piece of a chunk."""
    return _chunks(lambda room, f, u: lib.hp_pieces(nbytes, piece_bytes, room, f, u))


def drain_before(lib, c, slots):
    """(the chunk to drain before chunk c starts or None, the slot of chunk c)."""
    slot = ctypes.c_uint64(0)
    d = lib.hp_drain_before(c, slots, ctypes.addressof(slot))
    return (None if d < 0 else int(d)), int(slot.value)


def build_copier(flags=()):
    """The stand-alone copier program built with the host compiler and `flags`; returns its path, or None where the compiler
    cannot link with them (no runtime of that sanitizer on this machine), with the compiler's words."""
    d = tempfile.mkdtemp(prefix="hostpipe_copier_")
    exe = os.path.join(d, "hostpipe_copier")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", CSRC] + list(flags) +
                       [os.path.join(ROOT, "tests", "hostpipe_copier_main.cc"), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        return None, r.stderr
    return exe, ""
