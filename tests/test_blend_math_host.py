"""The 1-D blends the library compiles (fimex_amd/csrc/blend_math.hpp: the factor, the log coordinates, the branch a factor
selects and the value on that branch) run here on the CPU: tests/blend_math_host.cc uses the header the way convert.hip does
(classify, then evaluate over n elements) and the way vertical_plan.hip does (fold to an entry, evaluate from the stored factor),
and fimex_amd/build.py compiles it with g++, without any HIP header.  Every result must equal the oracle's orc_get_values_1d_f,
which tests/test_oracle_vs_reference.py pins to the reference's own C, bit for bit, with NaN in the same places and the same
return code.  No GPU is involved."""
import ctypes

import numpy as np
import pytest

import oracle
import time_quality_ref as tq
from fimex_amd import build as fb
from test_oracle_vs_reference import ABX

COPY_A, COPY_B, BLEND, UNDEFINED, ERROR = range(5)
KINDS = range(7)
KIND_IDS = ["nearest", "linear", "weak_extrapol", "no_extrapol", "const_extrapol", "log", "log_log"]
LOG_KINDS = (oracle.BLEND_LOG, oracle.BLEND_LOG_LOG)
SENTINEL = np.float32(-12345.0)  # oracle.get_values_1d prefills its output with it
UNDEFINED_BITS = 0x7FC00000

N = 16
NAN_IN_A, NAN_IN_B = 1, 2  # A is NaN and B is not, B is NaN and A is not


def _fields():
    """(A, B): NaN on either side and on both, infinities and zeros of both signs at known indices."""
    rng = np.random.default_rng(5)
    A = rng.uniform(-300.0, 300.0, N).astype(np.float32)
    B = rng.uniform(-300.0, 300.0, N).astype(np.float32)
    A[NAN_IN_A], B[NAN_IN_B] = np.nan, np.nan
    A[3], B[4], A[5], B[5] = np.inf, -np.inf, np.inf, np.inf
    A[6], B[6], A[7], B[7] = 0.0, -0.0, -0.0, 0.0
    A[8], B[8] = -np.inf, np.inf
    A[9], B[9] = np.nan, np.nan
    return A, B


A, B = _fields()


def _ulps(v):
    """v as a float and one float ulp on either side, as doubles."""
    v = np.float32(v)
    return [float(v), float(np.nextafter(v, np.float32(np.inf))), float(np.nextafter(v, np.float32(-np.inf)))]


def _triples(kind):
    t = list(ABX)
    t += [(2., 2., 2.), (3., 7., 3.), (3., 7., 7.), (7., 3., 7.), (7., 3., 3.)]  # a == b, x == a, x == b
    for fv in (-1., 0., 1., 2.):
        for x in _ulps(fv):
            t.append((0., 1., x))  # f is x itself
        t.append((2., 4., 2. + 2. * fv))  # f exactly fv from other coordinates
        t.append((10., 6., 10. - 4. * fv))
        for x in _ulps(fv):  # positive coordinates for the log kinds: f is the float of ln x
            t.append((1., np.e, float(np.exp(x))))
    t += [(0., 1., 1.), (1., 0., 1.), (1., 1., 0.), (0., 0., 0.), (-1., 1., 1.), (1., -1., 1.), (1., 1., -1.), (-2., -3., -4.),
          (-0., 2., 3.), (1e-320, 2., 3.), (-np.e, 1., 2.), (1. - np.e, 2., 3.), (-np.inf, 1., 2.), (np.inf, 1., 2.)]  # zero and negative
    t += [(np.nan, 1., 2.), (1., np.nan, 2.), (1., 2., np.nan), (np.nan, np.nan, np.nan), (np.nan, np.nan, 1.)]
    rng = np.random.default_rng(100 + kind)
    r = rng.uniform(-5., 10., (2000, 3)) if kind not in LOG_KINDS else np.exp(rng.uniform(-8., 8., (2000, 3)))
    r[::50, 1] = r[::50, 0]   # a == b
    r[1::50, 2] = r[1::50, 0]  # x == a
    r[2::50, 2] = r[2::50, 1]  # x == b
    if kind in LOG_KINDS:
        rows = np.arange(3, r.shape[0], 50)
        r[rows, rng.integers(0, 3, rows.size)] *= -1.0
    return t + [tuple(row) for row in r]


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(fb.build_blend_math_host())
    V, Z, D, F = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.POINTER(ctypes.c_float)
    lib.blend_math_classify.argtypes = [ctypes.c_int, D, D, D, F]
    lib.blend_math_direct_f.argtypes = [ctypes.c_int, V, V, V, Z, D, D, D]
    lib.blend_math_entry_f.argtypes = [ctypes.c_int, V, V, V, Z, D, D, D, F]
    lib.blend_math_linear_d.argtypes = [V, V, V, Z, D, D, D]
    return lib


def _classify(shim, kind, a, b, x):
    f = ctypes.c_float()
    return shim.blend_math_classify(kind, a, b, x, ctypes.byref(f)), np.float32(f.value)


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _same(got, want):
    """bit for bit, NaN in the same places (a NaN's payload is the adder's business)"""
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(_bits(got)[~gn], _bits(want)[~wn])


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_direct_and_entry_forms_match_the_oracle(shim, kind):
    seen = set()
    for a, b, x in _triples(kind):
        label = "kind %d a %r b %r x %r" % (kind, a, b, x)
        want, wrc = oracle.get_values_1d(kind, A, B, a, b, x)
        got = np.full(N, SENTINEL, np.float32)
        grc = shim.blend_math_direct_f(kind, A.ctypes.data, B.ctypes.data, got.ctypes.data, N, a, b, x)
        assert grc == wrc, label
        assert _same(got, want), "%s: got %r want %r" % (label, got, want)
        cls, f = _classify(shim, kind, a, b, x)
        seen.add(cls)
        if cls == COPY_A:
            assert _bits(got)[NAN_IN_B] == _bits(A)[NAN_IN_B], label  # no 0 * NaN from the other field
        if cls == COPY_B:
            assert _bits(got)[NAN_IN_A] == _bits(B)[NAN_IN_A], label
        if cls == ERROR:
            assert np.all(got == SENTINEL), label  # nothing written
        # the entry form: the bits of the direct form, an undefined cell where the direct form reports an error
        ent = np.full(N, SENTINEL, np.float32)
        fe = ctypes.c_float()
        defined = shim.blend_math_entry_f(kind, A.ctypes.data, B.ctypes.data, ent.ctypes.data, N, a, b, x, ctypes.byref(fe))
        assert defined == (cls in (COPY_A, COPY_B, BLEND)), label
        if cls in (UNDEFINED, ERROR):
            assert np.all(_bits(ent) == UNDEFINED_BITS) and fe.value == 0.0, label
        else:
            assert np.array_equal(_bits(ent), _bits(got)), "%s: entry %r direct %r" % (label, ent, got)
            if cls == BLEND:
                assert _bits(np.float32([fe.value]))[0] == _bits(np.float32([f]))[0], label
            else:
                assert fe.value == (0.0 if cls == COPY_A else 1.0), label
    want_seen = {oracle.BLEND_NEAREST: {COPY_A}, oracle.BLEND_LINEAR: {COPY_A, COPY_B, BLEND},
                 oracle.BLEND_LINEAR_CONST_EXTRAPOL: {COPY_A, COPY_B, BLEND}, oracle.BLEND_LOG: {COPY_A, COPY_B, BLEND, ERROR},
                 oracle.BLEND_LOG_LOG: {COPY_A, COPY_B, BLEND, ERROR}}.get(kind, {COPY_A, COPY_B, BLEND, UNDEFINED})
    assert seen == want_seen


def test_linear_blend_of_doubles(shim):
    Ad, Bd = A.astype(np.float64) * 1.0000001, B.astype(np.float64) * 0.9999999
    Ad[10], Bd[10] = 5e-324, -1e308
    for a, b, x in _triples(oracle.BLEND_LINEAR):
        want = oracle.get_values_linear_d(Ad, Bd, a, b, x)
        got = np.full(N, -12345.0)
        assert shim.blend_math_linear_d(Ad.ctypes.data, Bd.ctypes.data, got.ctypes.data, N, a, b, x) == oracle.OK
        assert _same(got, want), "a %r b %r x %r: got %r want %r" % (a, b, x, got, want)


@pytest.mark.parametrize("axis", sorted(tq.AXES))
def test_weak_extrapol_class_is_the_time_axis_branch(shim, axis):
    old, new = tq.AXES[axis]
    t1, t2 = tq.time_mapping(old, new)
    seen = set()
    for i, x in enumerate(new):
        a, b = float(old[int(t1[i])]), float(old[int(t2[i])])
        wf, wbranch = tq.blend_factor(a, b, float(x))
        cls, f = _classify(shim, oracle.BLEND_LINEAR_WEAK_EXTRAPOL, a, b, float(x))
        assert (tq.COPY_A, tq.COPY_B, tq.BLEND, tq.UNDEFINED) == (COPY_A, COPY_B, BLEND, UNDEFINED)
        assert cls == wbranch and _bits(np.float32(f).reshape(1))[0] == _bits(np.float32(wf).reshape(1))[0], (axis, i)
        seen.add(cls)
    if axis == "fine":
        assert seen == {COPY_A, COPY_B, BLEND, UNDEFINED}
