"""The per-cell arithmetic of the merge on a vector pair that the HIP kernels compile (fimex_amd/csrc/merge_vector_math.hpp: the
rotation, the smoothing of a pair and the overlay of a pair) run here on the CPU: tests/merge_vector_math_host.cc uses the header
the way merge_vector.hip does and fimex_amd/build.py compiles it with g++, without any HIP header.  Every result must equal the
restatement of tests/merge_vector_ref.py bit for bit.  All three grids are one 15 x 17 grid and the regrids are nearest-neighbour
at the cells' own positions, so the restatement's regrids are copies and everything else of it is compared.  No GPU is involved."""
import ctypes

import numpy as np
import pytest

import merge_ref as mr
import merge_vector_ref as mv
import oracle
from fimex_amd import build as fb

NX, NY, NZ = 15, 17, 2
WIDTHS = [(5, 2), (1, 0), (3, 4), (9, 20)]


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(fb.build_merge_vector_math_host())
    V, Z = ctypes.c_void_p, ctypes.c_size_t
    lib.merge_vector_math_rotate.argtypes = [V, V, V, Z, Z]
    lib.merge_vector_math_smooth.argtypes = [V, V, V, V, V, V, V, Z, Z, Z, Z, Z, ctypes.c_int, ctypes.POINTER(Z)]
    lib.merge_vector_math_overlay.argtypes = [V, V, V, V, V, V, V, V, Z, Z, ctypes.POINTER(Z)]
    return lib


def _same(got, want, label):
    gn, wn = np.isnan(got), np.isnan(want)
    same = (gn & wn) | (~gn & ~wn & (got.view(np.uint32) == want.view(np.uint32)))
    assert same.all(), "%s: %d cells differ, first at %s" % (label, np.count_nonzero(~same), tuple(np.argwhere(~same)[0]))


def _fields(seed):
    """four fields with 10 % NaN each, placed independently, and three rotation fields with a few NaN cells, exact 0 and exact 90 degrees"""
    rng = np.random.default_rng(seed)
    fields = []
    for _ in range(4):
        f = rng.normal(0, 8, (NZ, NY, NX)).astype(np.float32)
        f[rng.random(f.shape) < 0.1] = np.nan
        fields.append(f)
    fields[0][0, 8, 8], fields[2][0, 8, 8] = 3.5, 3.5  # diff == 0 where the rotation is by nothing
    matrices = []
    for k in range(3):
        phi = rng.uniform(-4, 4, (NY, NX))
        phi[8, 8] = 0.0
        phi[3, 3] = np.pi / 2
        phi[rng.random(phi.shape) < 0.05] = np.nan
        matrices.append(mv.angle_matrix(phi))
    return fields, matrices


def test_rotation(shim):
    (Iu, Iv, _, _), (R, _, _) = _fields(1)
    u, v = Iu.copy(), Iv.copy()
    assert shim.merge_vector_math_rotate(R.ctypes.data, u.ctypes.data, v.ctypes.data, NX * NY, NZ) == 0
    wu, wv = oracle.vector_reproject_values(R, Iu, Iv, NX, NY)
    _same(u, wu, "rotated u")
    _same(v, wv, "rotated v")
    assert np.array_equal(np.isnan(u), np.isnan(v)) and np.isnan(u).sum() > np.isnan(Iu).sum()  # a NaN in either makes both NaN


@pytest.mark.parametrize("use_outer", [True, False], ids=["outer1", "outer0"])
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "tw%d-bw%d" % w)
def test_pair_cells_equal_the_restatement(shim, widths, use_outer):
    tw, bw = widths
    (Iu, Iv, Ou, Ov), R = _fields(100 * tw + bw)
    j, i = np.meshgrid(np.arange(NY, dtype=np.float64), np.arange(NX, dtype=np.float64), indexing="ij")
    here = (i.ravel(), j.ravel())
    wantU, wantV, wSu, wSv = mv.merge_vector(Iu, Iv, Ou, Ov, (here, here, here), ((NY, NX),) * 3, R, oracle.NEAREST, oracle.NEAREST, tw, bw, use_outer)
    asked = ctypes.c_size_t(0)
    Su, Sv = np.empty_like(Iu), np.empty_like(Iu)
    assert shim.merge_vector_math_smooth(Iu.ctypes.data, Iv.ctypes.data, Ou.ctypes.data, Ov.ctypes.data, R[0].ctypes.data, Su.ctypes.data, Sv.ctypes.data,
                                         NX, NY, NZ, tw, bw, int(use_outer), ctypes.byref(asked)) == 0
    _same(Su, wSu, "Su tw %d bw %d useOuter %d" % (tw, bw, use_outer))
    _same(Sv, wSv, "Sv tw %d bw %d useOuter %d" % (tw, bw, use_outer))
    # the outer pair is asked for exactly where one of the components reads it: not where both inner values are defined inside
    kind, _ = mr._alpha_planes(NX, NY, tw, bw)
    nu, nv = np.isnan(Iu), np.isnan(Iv)
    needs = ((nu | nv) & use_outer) | ((~nu | ~nv) & (kind != 1)[None])
    assert asked.value == np.count_nonzero(needs)
    outU, outV = np.empty_like(Iu), np.empty_like(Iu)
    assert shim.merge_vector_math_overlay(Su.ctypes.data, Sv.ctypes.data, R[1].ctypes.data, Ou.ctypes.data, Ov.ctypes.data, R[2].ctypes.data,
                                          outU.ctypes.data, outV.ctypes.data, NX * NY, NZ, ctypes.byref(asked)) == 0
    _same(outU, wantU, "outU tw %d bw %d useOuter %d" % (tw, bw, use_outer))
    _same(outV, wantV, "outV tw %d bw %d useOuter %d" % (tw, bw, use_outer))
    STu, STv = oracle.vector_reproject_values(R[1], wSu, wSv, NX, NY)
    assert asked.value == np.count_nonzero(np.isnan(STu) | np.isnan(STv)) and 0 < asked.value < Iu.size
    if (tw, bw) == (5, 2):  # the case holds what it is meant to hold
        assert np.isnan(wantU).any() and np.isfinite(wantU).mean() > 0.5 and (nu ^ nv).any()
