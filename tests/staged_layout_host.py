"""fimex_amd/csrc/staged_layout.hpp on the CPU: tests/staged_layout_host.cc compiled with g++ into a temporary directory and called
through ctypes (the way tests/test_creep_rects.py wraps creep_rects.hpp), and the tile-cutting loop of build_shape (staged2_plan.hip)
with the tile scan as a Python function."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_LARGE = 0xFFFFFFFF  # kTileTooLarge
NONE = 0xFFFFFFFF       # padding of the workgroup -> tile table
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    d = tempfile.mkdtemp(prefix="staged_layout_")
    so = os.path.join(d, "libstaged_layout_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "fimex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "staged_layout_host.cc"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    u32, u64, ptr = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    lib.sl_flat_workgroup.argtypes = [u32, u32, ptr, ptr]
    lib.sl_flat_workgroup.restype = None
    lib.sl_first_form_grid.argtypes = [u32, u32, u32]
    lib.sl_first_form_grid.restype = u32
    lib.sl_first_form_tiles.argtypes = [u32, u32, u32, u32, ptr]
    lib.sl_first_form_tiles.restype = None
    lib.sl_xcd_order.argtypes = [ptr, u64, u32, u32, ptr, u64]
    lib.sl_xcd_order.restype = u64
    lib.sl_cut_new.argtypes = [u32, u32, u32, u32]
    lib.sl_cut_new.restype = ptr
    lib.sl_cut_free.argtypes = [ptr]
    lib.sl_cut_free.restype = None
    lib.sl_cut_step.argtypes = [ptr]
    lib.sl_cut_step.restype = u32
    lib.sl_cut_count.argtypes = [ptr]
    lib.sl_cut_count.restype = u64
    lib.sl_cut_tiles.argtypes = [ptr, ptr]
    lib.sl_cut_tiles.restype = None
    lib.sl_cut_refine.argtypes = [ptr, ptr]
    lib.sl_cut_finish.argtypes = [ptr, ptr]
    lib.sl_float_z_chunks.argtypes = [u32, u32, ctypes.c_int, u32, u32, ptr, ptr, ptr]
    lib.sl_float_z_chunks.restype = None
    lib.sl_typed_z_chunks.argtypes = [u32, u32, u32, ptr, ptr]
    lib.sl_typed_z_chunks.restype = None
    lib.sl_first_form_z.argtypes = [u32, u32, u32, ptr, ptr]
    lib.sl_first_form_z.restype = None
    lib.sl_tile_chunk_cap.argtypes = [u32, u32, u32, u32, u32]
    lib.sl_tile_chunk_cap.restype = u32
    _lib = lib
    return lib


def xcd_order(lib, band_of, n_bands, stripe):
    band_of = np.ascontiguousarray(band_of, dtype=np.uint32)
    out = np.zeros(8 * (len(band_of) + 1), np.uint32)
    n = lib.sl_xcd_order(band_of.ctypes.data, len(band_of), n_bands, stripe, out.ctypes.data, len(out))
    assert n <= len(out)
    return out[:n].copy()


class Tile:
    def __init__(self, v):
        self.x0, self.y0, self.w, self.chunks, self.chunk_base, self.gather, self.band, self.band_w = (int(x) for x in v)


def cut_tiles(lib, outX, outY, tileW, tileH, scan, most_passes=64):
    """The loop of build_shape: scan(tiles) returns per tile the 16-byte chunks it stages, or TOO_LARGE for one that does not fit a
    slot (gather tiles are in the list; what is returned for them does not count).  Returns the passes as lists of Tile (the last
    one holds the final tiles, with chunk_base when the form is kept), whether the form is kept, and the chunk total."""
    cut = lib.sl_cut_new(outX, outY, tileW, tileH)
    try:
        passes = []
        while True:
            assert len(passes) <= most_passes, "the cutting does not end"
            n = lib.sl_cut_count(cut)
            raw = np.zeros((n, 8), np.uint32)
            lib.sl_cut_tiles(cut, raw.ctypes.data)
            tiles = [Tile(v) for v in raw]
            counts = np.array(scan(tiles), dtype=np.uint32)
            assert len(counts) == n
            for t, c in zip(tiles, counts):
                t.chunks = 0 if t.gather else int(c)
            passes.append(tiles)
            if not lib.sl_cut_refine(cut, counts.ctypes.data):
                break
        total = ctypes.c_uint64(0)
        given_up = lib.sl_cut_finish(cut, ctypes.byref(total))
        lib.sl_cut_tiles(cut, raw.ctypes.data)
        passes[-1] = [Tile(v) for v in raw]
        return passes, given_up == 0, int(total.value)
    finally:
        lib.sl_cut_free(cut)
