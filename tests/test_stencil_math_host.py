"""The backward stencil rules the HIP kernels compile (fimex_amd/csrc/stencil_math.hpp: which cells an output reads, the plan-entry
encoding, the bilinear forms and their selection, the bicubic accumulation) run here on the CPU: tests/stencil_math_host.hip uses
the header the way the kernels do -- classify, encode, decode, gather, combine -- and fimex_amd/build.py compiles it for the host
only.  Every point must equal the oracle's mifi_get_values_f / _bilinear_f / _bicubic_f bit for bit, with NaN in the same places,
and a plan entry must decode to the cells classify named.  No GPU is involved."""
import ctypes

import numpy as np
import pytest

import cases
import oracle
from fimex_amd import build as fb

SHAPES = [((37, 29), (41, 33)), ((8, 8), (16, 16))]
SEEDS = [100, 101, 102]
NZ = 3
INTERIOR, LINEAR_X, LINEAR_Y, NEAREST_BOTH, UNDEFINED = range(5)
ENTRY = {oracle.NEAREST: "stencil_math_nearest", oracle.BILINEAR: "stencil_math_bilinear", oracle.BICUBIC: "stencil_math_bicubic"}


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(fb.build_stencil_host())
    for name in ENTRY.values():
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def run(shim, method, f, px, py, ix, iy):
    out = np.empty((px.size, NZ), dtype=np.float32)
    cls = np.empty(px.size, dtype=np.int32)
    getattr(shim, ENTRY[method])(f.ctypes.data, ix, iy, NZ, px.ctypes.data, py.ctypes.data, px.size, out.ctypes.data, cls.ctypes.data)
    return out, cls


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % (s[0] + s[1]))
@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR, oracle.BICUBIC], ids=["nearest", "bilinear", "bicubic"])
def test_the_kernels_stencil_header_matches_the_oracle_point_by_point(shim, method, shape, seed):
    (ix, iy), (ox, oy) = shape
    px, py = (np.ascontiguousarray(a, dtype=np.float64) for a in cases.backward_positions(ix, iy, ox, oy, seed))
    f = np.ascontiguousarray(cases.field(NZ, iy, ix, seed + 1000))
    got, cls = run(shim, method, f, px, py, ix, iy)
    want = np.stack([oracle.get_values(method, f, px[p], py[p], ix, iy, NZ) for p in range(px.size)])
    assert cases.same(got, want), cases.describe_mismatch(got, want)
    assert (cls >= 0).all(), "a plan entry decodes to other cells than classify named: points %s" % np.nonzero(cls < 0)[0][:5]
    counts = np.bincount(cls, minlength=5)
    print("classes (interior, linear in x, linear in y, nearest in both, undefined):", counts.tolist())
    # an undefined point is NaN in every slice (a defined one may be, from the field's NaNs)
    assert np.isnan(got[cls == UNDEFINED]).all()
    if method == oracle.BILINEAR:
        assert (counts > 0).all(), "a class of the bilinear rules does not occur: %s" % counts.tolist()
    else:
        assert counts[INTERIOR] > 0 and counts[UNDEFINED] > 0 and counts[1:4].sum() == 0
