"""The level search of the vertical kernels (fimex_amd/csrc/vertical_search.hpp: Column::level, monotonic_pair and walk_pairs,
in the kernels' loop) run here on the CPU: tests/vertical_search_host.hip calls the functions the kernels call, one
column after another, and fimex_amd/build.py compiles it for the host only.  Every pair must equal
vertical_ref.find_closest_neighbor_distinct_elements, the sequential restatement of include/fimex/Utils.h:251-290 with its
fallback (tests/test_vertical_ref.py checks it against known answers) -- with the bisection allowed, where monotonic_pair decides
which targets it may answer, and with every column walked.  No GPU is involved."""
import collections
import ctypes

import numpy as np
import pytest

import vertical_ref as vr
from fimex_amd import build as fb

ORDERS = ("inc", "dec", "shuf", "rep", "nan")
NZI = (1, 2, 3, 7, 19)
NCOL, NX = 8, 21  # 5 orders x 5 sizes x 5 kinds x 8 columns x 21 targets = 21 000 pairs
DBL_MAX = float(np.finfo(np.float64).max)


def _sequence(rng, order, nzi):
    """nzi values in 1 .. 1000 in the given order; shuf is never monotonic from three values on (two distinct values always are)."""
    s = np.sort(rng.uniform(1., 1000., nzi))
    if order == "dec":
        s = s[::-1].copy()
    if order in ("shuf", "rep", "nan"):
        s = rng.permutation(s)
        while nzi >= 3 and (np.all(np.diff(s) > 0) or np.all(np.diff(s) < 0)):
            s = rng.permutation(s)
    if order == "rep":
        if nzi > 2:
            s[nzi // 2], s[-1] = s[0], s[1]
        elif nzi == 2:
            s[1] = s[0]
    if order == "nan":
        s[rng.integers(0, nzi)] = np.nan
    return s


def _levels(rng, kind, order, nzi):
    """A vertical_ref.Levels of NCOL columns (nt = ny = 1).  The formula kinds share their coefficients among the columns; the
    columns of the second half get a ps at which neighbouring float levels tie although the coefficients are ordered."""
    s = _sequence(rng, order, nzi)
    scale = 1 + 0.3 * rng.uniform(-1, 1, NCOL)
    if kind == vr.FIELD:
        field = (s[:, None] * scale[None, :]).astype(np.float32)
        if order == "nan":
            field[rng.uniform(size=field.shape) < 0.2] = np.nan
        return vr.Levels(kind, nzi, field=field.reshape(1, nzi, 1, NCOL))
    if kind == vr.AXIS:
        return vr.Levels(kind, nzi, axis=s)
    ps = np.float32(1e5) * scale.astype(np.float32)
    if kind == vr.SIGMA:
        ps[NCOL // 2:] = [0.0, 3e-45, 1e-44, 0.0][:NCOL - NCOL // 2]  # sigma * ps: zero or a few denormals
        return vr.Levels(kind, nzi, sigma=s / 1000., ptop=0.0, ps=ps.reshape(1, 1, NCOL))
    # a * p0 (or ap) = s * 1e-6 keeps the order on its own; b in steps of 0.1 repeats: at ps = 0 the levels are s * 1e-6, at
    # ps ~ 1e5 the levels of one b differ by less than an ulp
    b = np.floor(s / 100.) / 10.
    ps[:NCOL // 2] = [0.0, 1e-3, 0.0, 1e-2][:NCOL // 2]
    if kind == vr.HYBRID_SIGMA:
        return vr.Levels(kind, nzi, a=s * 1e-11, b=b, p0=1e5, ps=ps.reshape(1, 1, NCOL))
    return vr.Levels(kind, nzi, ap=s * 1e-6, b=b, ps=ps.reshape(1, 1, NCOL))


def _targets(rng, lev):
    """NX targets for one column of float levels: on a level, between levels, below and above the column, so far out that x - level
    rounds to one double for two levels, NaN and +-DBL_MAX."""
    ok = lev[~np.isnan(lev)].astype(np.float64)
    if ok.size == 0:
        ok = np.array([1.0])
    lo, hi = ok.min(), ok.max()
    pick = lambda: ok[rng.integers(0, ok.size)]
    x = [float(lev[0]), float(lev[-1]), pick(), pick(), lo, hi,
         0.5 * (pick() + pick()), 0.5 * (pick() + pick()), 0.5 * (lo + hi), float(np.nextafter(np.float32(pick()), np.float32(np.inf))),
         lo - 50., lo - abs(lo) * 1e-7 - 1e-30, hi + 50., hi + abs(hi) * 1e-7 + 1e-30,
         1e30, -1e30, (hi + 1.) * 2. ** 54, np.nan, DBL_MAX, -DBL_MAX, rng.uniform(-100., 1500.)]
    assert len(x) == NX
    return np.array(x, np.float64)


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(fb.build_vertical_search_host())
    V, Z, D, I, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_int, ctypes.c_uint
    lib.vertical_search_host.argtypes = [I, I, U, V, V, D, D, V, V, Z, V, Z, I, V, V, V, V]
    return lib


def _run(shim, group, lv, x, bisect):
    ptr = lambda a: None if a is None else a.ctypes.data
    c0 = {vr.AXIS: lv.axis, vr.SIGMA: lv.sigma, vr.HYBRID_SIGMA: lv.a, vr.HYBRID_SIGMA_AP: lv.ap}.get(lv.kind)
    first, second = np.full(x.shape, 99999, np.uint32), np.full(x.shape, 99999, np.uint32)
    walked = np.full(x.shape, 7, np.uint8)
    levels = np.empty((NCOL, lv.nz), np.float32)
    rc = shim.vertical_search_host(group, lv.kind, lv.nz, ptr(c0), ptr(lv.b), lv.p0, lv.ptop, ptr(lv.ps), ptr(lv.field), NCOL, x.ctypes.data, NX,
                                   bisect, first.ctypes.data, second.ctypes.data, walked.ctypes.data, levels.ctypes.data)
    assert rc == 0
    return first, second, walked, levels


def test_search_equals_the_sequential_reference(shim):
    bisected, walked_n, pairs = collections.Counter(), collections.Counter(), 0
    for oi, order in enumerate(ORDERS):
        for nzi in NZI:
            for kind in vr.KINDS:
                rng = np.random.default_rng(1000 * oi + 10 * nzi + kind)
                lv = _levels(rng, kind, order, nzi)
                ilev = vr.level_field(lv, 1, 1, NCOL)[0, :, 0, :].T.copy()  # [NCOL][nzi]
                x = np.stack([_targets(rng, ilev[c]) for c in range(NCOL)])
                want = np.array([[vr.find_closest_neighbor_distinct_elements(ilev[c], x[c, k]) for k in range(NX)] for c in range(NCOL)])
                for group, bisect in ((4, 1), (8, 1), (4, 0)):
                    label = "%s nzi %d kind %d group %d bisect %d" % (order, nzi, kind, group, bisect)
                    first, second, walked, levels = _run(shim, group, lv, x, bisect)
                    assert np.array_equal(levels.view(np.uint32), ilev.view(np.uint32)), label  # Column::level
                    bad = np.argwhere((first != want[..., 0]) | (second != want[..., 1]))
                    assert bad.size == 0, "%s: column %d levels %r x %r: got (%d, %d) want %r" % (
                        label, bad[0][0], ilev[bad[0][0]], x[tuple(bad[0])], first[tuple(bad[0])], second[tuple(bad[0])], want[tuple(bad[0])])
                    assert set(np.unique(walked)) <= {0, 1} and (bisect or walked.all()), label
                    if (group, bisect) == (4, 1):
                        key = order if order != "shuf" or nzi >= 3 else "shuf of two"
                        bisected[key] += int((walked == 0).sum())
                        walked_n[key] += int((walked == 1).sum())
                        pairs += x.size
    print("pairs %d; decided by the bisection %r; handed to the walk %r" % (pairs, dict(bisected), dict(walked_n)))
    assert pairs >= 20000
    for order in ("inc", "dec"):
        assert bisected[order] > 0 and walked_n[order] > 0
    # two distinct levels are always monotonic, so a shuffle of two is counted apart; from three on a shuffle never is
    for order in ("shuf", "rep", "nan"):
        assert bisected[order] == 0 and walked_n[order] > 0
