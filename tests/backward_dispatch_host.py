"""fimex_amd/csrc/backward_dispatch.hpp on the CPU: tests/backward_dispatch_host.cc compiled with g++ into a temporary directory and
called through ctypes (the way tests/slice_list_host.py wraps slice_list.hpp).  Every call answers for the whole cross product of
its tables: switches [S][8], plans [P][9], calls [C][6] (the columns: backward_dispatch_ref.py)."""
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
    d = tempfile.mkdtemp(prefix="backward_dispatch_")
    so = os.path.join(d, "libbackward_dispatch_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "fimex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "backward_dispatch_host.cc"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    u64, ptr = ctypes.c_uint64, ctypes.c_void_p
    lib.bd_columns.argtypes = [ctypes.c_int]
    lib.bd_columns.restype = ctypes.c_int
    lib.bd_plan_build.argtypes = [ptr, u64, ptr, u64, ptr]
    lib.bd_plan_build.restype = None
    for f in (lib.bd_float, lib.bd_typed):
        f.argtypes = [ptr, u64, ptr, u64, ptr, u64, ptr]
        f.restype = None
    _lib = lib
    return lib


def _table(lib, which, rows):
    t = np.ascontiguousarray(rows, dtype=np.int64)
    assert t.ndim == 2 and t.shape[1] == lib.bd_columns(which), t.shape
    return t


def plan_build(lib, switches, plans):
    """[S][P][2]: builds_first, builds_second."""
    s, p = _table(lib, 0, switches), _table(lib, 1, plans)
    out = np.full((len(s), len(p), 2), -7, np.int8)
    lib.bd_plan_build(s.ctypes.data, len(s), p.ctypes.data, len(p), out.ctypes.data)
    return out


def _cross(lib, fn, width, switches, plans, calls):
    s, p, c = _table(lib, 0, switches), _table(lib, 1, plans), _table(lib, 2, calls)
    out = np.full((len(s), len(p), len(c), width), -7, np.int8)
    fn(s.ctypes.data, len(s), p.ctypes.data, len(p), c.ctypes.data, len(c), out.ctypes.data)
    return out


def float_answers(lib, switches, plans, calls):
    """[S][P][C][4]: float_apply (0 second, 1 first, 2 gather), tune_has_choice, float_list, vector_fused."""
    return _cross(lib, lib.bd_float, 4, switches, plans, calls)


def typed_answers(lib, switches, plans, calls):
    """[S][P][C][6]: the candidates of typed_apply in four slots (0 second, 1 first, 2 gather, 3 three passes, -1 beyond the list),
    typed_list, vector_typed_fused."""
    return _cross(lib, lib.bd_typed, 6, switches, plans, calls)
