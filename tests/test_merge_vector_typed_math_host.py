"""The per-cell arithmetic of the merge on a packed vector pair that the HIP kernels compile
(fimex_amd/csrc/merge_vector_typed_math.hpp: smooth_pair_typed and regrid_overlay_pair_typed) run here on the CPU:
tests/merge_vector_typed_math_host.cc uses the header the way merge_vector_typed.hip does and fimex_amd/build.py compiles it with
g++, without any HIP header.  Every result must equal the restatement of tests/merge_vector_typed_ref.py byte for byte.  All three
grids are one 15 x 17 grid and the regrids are nearest-neighbour at the cells' own positions, so the restatement's regrids are
copies and everything else of it is compared.  The two callables are counted: the outer pair is evaluated exactly where a
component reads it, and the base pair likewise.  No GPU is involved."""
import ctypes

import numpy as np
import pytest

import merge_ref as mr
import merge_typed_ref as mt
import merge_vector_ref as mv
import merge_vector_typed_ref as mvt
import oracle
from fimex_amd import build as fb

NX, NY, NZ = 15, 17, 2
WIDTHS = [(5, 2), (1, 0), (3, 4), (9, 20)]
TYPES = {"short": "w", "ushort": "u"}  # the shim's instance -> the packings it runs with


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(fb.build_merge_vector_typed_math_host())
    V, Z = ctypes.c_void_p, ctypes.c_size_t
    for t in TYPES:
        getattr(lib, "merge_vector_typed_math_smooth_" + t).argtypes = [V, V, V, V, V, V, V, V, Z, Z, Z, Z, Z, ctypes.c_int, ctypes.POINTER(Z)]
        getattr(lib, "merge_vector_typed_math_overlay_" + t).argtypes = [V, V, V, V, V, V, V, V, V, Z, Z, ctypes.POINTER(Z)]
    return lib


def _same(got, want, label):
    assert got.dtype == want.dtype and got.shape == want.shape, label
    same = got == want
    assert same.all(), "%s: %d cells differ, first at %s" % (label, np.count_nonzero(~same), tuple(np.argwhere(~same)[0]))


def _fields(seed, key):
    """four packed fields with 10 % fill values each, placed independently, raw counts from the whole range of the type in 3 % of
    the cells (the same cells in all four, so that a rotated pair of them leaves the range), and three rotation fields with a few
    NaN cells, exact 0 and exact 90 degrees"""
    rng = np.random.default_rng(seed)
    packed = []
    wild = rng.random((NZ, NY, NX)) < 0.03
    for p in mvt.PACKINGS[key]:
        f = rng.normal(0, 8, (NZ, NY, NX))
        f[rng.random(f.shape) < 0.1] = np.nan
        raw = mt.as_packed(f, p)
        info = np.iinfo(raw.dtype)
        raw[wild] = rng.integers(info.min, info.max, size=int(wild.sum()), endpoint=True).astype(raw.dtype)
        packed.append((raw, p))
    matrices = []
    for k in range(3):
        phi = rng.uniform(-4, 4, (NY, NX))
        phi[8, 8] = 0.0
        phi[3, 3] = np.pi / 2
        phi[rng.random(phi.shape) < 0.05] = np.nan
        matrices.append(mv.angle_matrix(phi))
    return packed, matrices


def _counts(a, p):
    return oracle.data2interpolation_array(a, p.fill)


@pytest.mark.parametrize("ctype", sorted(TYPES))
@pytest.mark.parametrize("use_outer", [True, False], ids=["outer1", "outer0"])
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "tw%d-bw%d" % w)
def test_pair_cells_equal_the_restatement(shim, widths, use_outer, ctype):
    tw, bw = widths
    key = TYPES[ctype]
    ((Iu, pIu), (Iv, pIv), (Ou, pOu), (Ov, pOv)), R = _fields(100 * tw + bw, key)
    j, i = np.meshgrid(np.arange(NY, dtype=np.float64), np.arange(NX, dtype=np.float64), indexing="ij")
    here = (i.ravel(), j.ravel())
    want = mvt.merge_vector_typed(Iu, pIu, Iv, pIv, Ou, pOu, Ov, pOv, (here, here, here), ((NY, NX),) * 3, R, oracle.NEAREST, oracle.NEAREST, tw,
                                  bw, use_outer)
    packings = np.array([[p.fill, p.scale, p.offset] for p in (pIu, pIv, pOu, pOv)], np.float64)
    label = "%s tw %d bw %d useOuter %d" % (ctype, tw, bw, use_outer)
    asked = ctypes.c_size_t(0)
    fOu, fOv = _counts(Ou, pOu), _counts(Ov, pOv)
    Su, Sv = np.empty_like(Iu), np.empty_like(Iv)
    assert getattr(shim, "merge_vector_typed_math_smooth_" + ctype)(
        Iu.ctypes.data, Iv.ctypes.data, fOu.ctypes.data, fOv.ctypes.data, R[0].ctypes.data, packings.ctypes.data, Su.ctypes.data, Sv.ctypes.data, NX,
        NY, NZ, tw, bw, int(use_outer), ctypes.byref(asked)) == 0
    _same(Su, want.Su, "Su " + label)
    _same(Sv, want.Sv, "Sv " + label)
    # the outer pair is asked for exactly where one of the components reads it: not where both inner values are defined inside
    kind, _ = mr._alpha_planes(NX, NY, tw, bw)
    nu, nv = np.isnan(mt.unpack(Iu, pIu)), np.isnan(mt.unpack(Iv, pIv))
    needs = ((nu | nv) & use_outer) | ((~nu | ~nv) & (kind != 1)[None])
    assert asked.value == np.count_nonzero(needs)
    fSu, fSv = _counts(Su, pIu), _counts(Sv, pIv)
    outU, outV = np.empty_like(Iu), np.empty_like(Iv)
    assert getattr(shim, "merge_vector_typed_math_overlay_" + ctype)(
        fSu.ctypes.data, fSv.ctypes.data, R[1].ctypes.data, fOu.ctypes.data, fOv.ctypes.data, R[2].ctypes.data, packings.ctypes.data,
        outU.ctypes.data, outV.ctypes.data, NX * NY, NZ, ctypes.byref(asked)) == 0
    _same(outU, want.outU, "outU " + label)
    _same(outV, want.outV, "outV " + label)
    # the base pair is asked for exactly where a rounded component of the top pair is its fill value
    STu = oracle.interpolation_array2data(want.ST_float[0], pIu.type, pIu.fill)
    STv = oracle.interpolation_array2data(want.ST_float[1], pIv.type, pIv.fill)
    base_read = np.isnan(mt.unpack(STu, pIu)) | np.isnan(mt.unpack(STv, pIv))
    assert asked.value == np.count_nonzero(base_read) and 0 < asked.value < Iu.size
    if (tw, bw) == (5, 2):  # the case holds what it is meant to hold
        fills = np.isnan(mt.unpack(want.outU, pIu))
        assert fills.any() and (~fills).mean() > 0.5 and (nu ^ nv).any()
        wrapped = sum(mvt.out_of_range(r, p) for r, p in zip(want.OI_float + want.ST_float + want.OT_float, (pOu, pOv, pIu, pIv, pOu, pOv)))
        assert wrapped >= 1, "no rotated count leaves the range of its type"
