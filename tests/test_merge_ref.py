"""tests/merge_ref.py, the CPU restatement of the reference's grid merging, against the reference's own known answers
(test/testMerger.cc:58-60, :92-94, on its own fixtures and within its own bounds) and against a hand-made table of the branches of
CDMBorderSmoothing_Linear::operator() (src/CDMBorderSmoothing_Linear.cc:52-78), the wrap-around of its size_t arithmetic included."""
import functools
import math

import numpy as np
import pytest

import merge_ref as mr


@functools.lru_cache(maxsize=None)
def _merged(golden_dir, name):
    c = mr.load_case(golden_dir, name)
    pos = mr.merge_positions(c["inner"], c["outer"], c["target"])
    out, S = mr.merge(c["I"], c["O"], pos, mr.case_shapes(c))
    return c, out, S


@pytest.mark.parametrize("name", sorted(mr.KNOWN))
def test_known_answers_of_the_reference(golden_dir, name):
    shape, known, bound = mr.KNOWN[name]
    c, out, _ = _merged(golden_dir, name)
    assert c["target"].shape == shape and out.shape == (1,) + shape
    for ix, iy, expected in known:
        got = float(out[0, iy, ix])
        print("%s (%d, %d): %.6f, expected %s" % (name, ix, iy, got, expected))
        assert abs(got - expected) < bound


def test_known_cells_are_middle_transition_and_outer(golden_dir):
    """the three cells of test_merger lie where its comment says: inside the inner grid, in its transition band, outside it"""
    c, out, S = _merged(golden_dir, "test_merger")
    x0 = int(np.argmin(np.abs(c["target"].x - c["inner"].x[0]))), int(np.argmin(np.abs(c["target"].y - c["inner"].y[0])))
    ny, nx = c["inner"].shape
    branches = []
    for ix, iy, _ in mr.KNOWN["test_merger"][1]:
        x, y = ix - x0[0], iy - x0[1]
        branches.append(mr.linear_alpha(nx, ny, 5, 2, x, y)[0] if 0 <= x < nx and 0 <= y < ny else "beyond")
    assert branches == [mr.INNER, mr.BLEND, "beyond"]


def test_extend_inner_axis():
    np.testing.assert_array_equal(mr.extend_inner_axis([2., 2.5, 3.], [0., 1., 2., 3., 4.]), [0., .5, 1., 1.5, 2., 2.5, 3., 3.5, 4.])
    np.testing.assert_array_equal(mr.extend_inner_axis([3., 2.5, 2.], [0., 1., 2., 3., 4.]), [4., 3.5, 3., 2.5, 2., 1.5, 1., .5, 0.])
    np.testing.assert_array_equal(mr.extend_inner_axis([1.25, 1.75], [1., 2.]), [1.25, 1.75])
    with pytest.raises(ValueError, match="not inside"):
        mr.extend_inner_axis([3., 4., 5.], [0., 1., 2., 3., 4.])
    with pytest.raises(ValueError, match="constant step"):
        mr.extend_inner_axis([1., 2., 3.5], [0., 1., 2., 3., 4.])


def _r(n, tw):
    """sqrt(n) / tw in doubles, as :34 and :79 compute it"""
    return math.sqrt(float(n)) / tw


# (nx, ny, tw, bw, x, y) -> (branch, alpha), worked out by hand from :46-83
BRANCHES = [
    # 20 x 16, tw 5, bw 2: xmin1 2, xmax1 7, xmin2 13, xmax2 18; ymin1 2, ymax1 7, ymin2 9, ymax2 14
    ((20, 16, 5, 2, 1, 8), (mr.OUTER, None)),          # :52 x < xmin1
    ((20, 16, 5, 2, 18, 8), (mr.OUTER, None)),         # :52 x >= xmax2
    ((20, 16, 5, 2, 10, 1), (mr.OUTER, None)),         # :52 y < ymin1
    ((20, 16, 5, 2, 10, 14), (mr.OUTER, None)),        # :52 y >= ymax2
    ((20, 16, 5, 2, 7, 7), (mr.INNER, None)),          # :54 first interior cell
    ((20, 16, 5, 2, 12, 8), (mr.INNER, None)),         # :54 last interior cell
    ((20, 16, 5, 2, 4, 4), (mr.BLEND, _r(18, 5))),     # :62 dist(3, 3)
    ((20, 16, 5, 2, 2, 2), (mr.BLEND, 1.0)),           # :62 dist(5, 5) / 5 > 1, clamped (:80)
    ((20, 16, 5, 2, 5, 11), (mr.BLEND, _r(8, 5))),     # :64 dist(2, 2)
    ((20, 16, 5, 2, 4, 8), (mr.BLEND, 3 / 5)),         # :66 xmax1 - x
    ((20, 16, 5, 2, 15, 5), (mr.BLEND, _r(8, 5))),     # :69 dist(2, 2)
    ((20, 16, 5, 2, 16, 11), (mr.BLEND, _r(13, 5))),   # :71 dist(3, 2)
    ((20, 16, 5, 2, 13, 8), (mr.BLEND, 0.0)),          # :73 x - xmin2 = 0
    ((20, 16, 5, 2, 17, 8), (mr.BLEND, 4 / 5)),        # :73
    ((20, 16, 5, 2, 10, 3), (mr.BLEND, 4 / 5)),        # :75 ymax1 - y
    ((20, 16, 5, 2, 10, 9), (mr.BLEND, 0.0)),          # :77 y - ymin2 = 0
    ((20, 16, 5, 2, 10, 13), (mr.BLEND, 4 / 5)),       # :77
    # 14 x 14, tw 5, bw 2: xmax1 = xmin2 = 7 and ymax1 = ymin2 = 7, the bands touch and no cell is interior
    ((14, 14, 5, 2, 7, 7), (mr.BLEND, 0.0)),           # :71 dist(0, 0)
    ((14, 14, 5, 2, 6, 7), (mr.BLEND, 1 / 5)),         # :64 dist(1, 0)
    # 11 x 11, tw 5, bw 2: xmax1 7, xmin2 4, the bands overlap; a cell of both takes the first branch that matches (:60)
    ((11, 11, 5, 2, 5, 5), (mr.BLEND, _r(8, 5))),      # :62 dist(2, 2), not :71 dist(1, 1)
    ((11, 11, 5, 2, 8, 3), (mr.BLEND, 1.0)),           # :69 dist(4, 4) / 5 > 1
    # 4 x 4, tw 5, bw 2: xmax2 = 2 = xmin1, every cell fails the first test
    ((4, 4, 5, 2, 2, 2), (mr.OUTER, None)),
    ((4, 4, 5, 2, 1, 1), (mr.OUTER, None)),
    # 4 x 4, tw 3, bw 0: xmax1 3, xmin2 1, xmax2 4
    ((4, 4, 3, 0, 0, 0), (mr.BLEND, 1.0)),             # :62 dist(3, 3) / 3 > 1
    ((4, 4, 3, 0, 2, 1), (mr.BLEND, _r(5, 3))),        # :62 dist(1, 2)
    ((4, 4, 3, 0, 3, 3), (mr.BLEND, _r(8, 3))),        # :71 dist(2, 2)
    # xmin2 = xmax2 - tw wraps.  3 x 9, tw 5, bw 0: xmax1 5, xmax2 3, xmin2 = 2^64 - 2; ymax1 5, ymin2 4.  "x >= xmin2" never holds
    ((3, 9, 5, 0, 1, 6), (mr.BLEND, _r(20, 5))),       # :64 dist(4, 2)
    ((3, 9, 5, 0, 2, 4), (mr.BLEND, _r(10, 5))),       # :62 dist(3, 1); signed arithmetic would take :69 with xmin2 = -2
    # 10 x 10, tw 9, bw 2: xmax1 11, xmax2 8, xmin2 = 2^64 - 1
    ((10, 10, 9, 2, 7, 7), (mr.BLEND, _r(32, 9))),     # :62 dist(4, 4); signed arithmetic would take :71 dist(8, 8)
    # xmax2 = nx - bw wraps.  3 x 9, tw 1, bw 4: xmax2 = 2^64 - 1 stops nobody, xmin1 4 stops every x
    ((3, 9, 1, 4, 2, 4), (mr.OUTER, None)),
    # 9 x 30, tw 9, bw 20: bw > nx, x < xmin1 20 for the whole grid
    ((9, 30, 9, 20, 8, 25), (mr.OUTER, None)),
    # 2 x 40, tw 3, bw 1: xmax2 1 = xmin1
    ((2, 40, 3, 1, 1, 20), (mr.OUTER, None)),
    ((2, 40, 3, 1, 0, 20), (mr.OUTER, None)),
]


@pytest.mark.parametrize("case", BRANCHES, ids=lambda c: "-".join(str(v) for v in c[0]))
def test_branch_table(case):
    args, want = case
    branch, alpha = mr.linear_alpha(*args)
    assert branch == want[0]
    if want[1] is None:
        assert alpha is None
    else:
        assert alpha == want[1]
    # the value: valueO, valueI, or the blend in two operations
    vI, vO = 280.25, 290.5
    got, b = mr.linear_smoothing(*args, vI, vO)
    if branch == mr.OUTER:
        assert got == vO and b == mr.OUTER
    elif branch == mr.INNER:
        assert got == vI and b == mr.INNER
    else:
        assert got == np.float64(vI) + alpha * (np.float64(vO) - np.float64(vI)) and b == mr.BLEND


def test_wrapped_bounds_are_the_size_t_values():
    """the cells above decide on these: nx - bw and xmax2 - tw as unsigned 64-bit values"""
    assert (3 - 4) & mr.M64 == (1 << 64) - 1 and ((3 - 0) - 5) & mr.M64 == (1 << 64) - 2
    # 3 x 9, tw 5, bw 0: no x reaches xmin2 = 2^64 - 2, so the right-hand band never applies and x = 2 blends from the left only
    assert [mr.linear_alpha(3, 9, 5, 0, x, 4)[1] for x in range(3)] == [1.0, math.sqrt(17.) / 5, math.sqrt(10.) / 5]
    # 3 x 9, tw 1, bw 4: xmax2 = 2^64 - 1 lets every x through "x >= xmax2", xmin1 = 4 stops them
    assert all(mr.linear_alpha(3, 9, 1, 4, x, y)[0] == mr.OUTER for x in range(3) for y in range(9))
    # 9 x 30, tw 9, bw 20: xmax2 = 2^64 - 11; the frame test is x < 20, true for the whole grid
    assert all(mr.linear_alpha(9, 30, 9, 20, x, 25)[0] == mr.OUTER for x in range(9))


def test_zero_difference_returns_the_outer_value():
    """:57-58: diff == 0 returns valueO, so +0 inner and -0 outer give -0 (I + alpha * diff would give +0)"""
    got, b = mr.linear_smoothing(20, 16, 5, 2, 4, 8, 0.0, -0.0)
    assert b == mr.EQUAL and got == 0 and np.signbit(got)
    got, b = mr.linear_smoothing(20, 16, 5, 2, 4, 8, -0.0, 0.0)
    assert b == mr.EQUAL and not np.signbit(got)
    out = mr.border_smooth(np.zeros((16, 20), np.float32), np.full((16, 20), -0.0, np.float32))
    assert np.all(np.signbit(out[mr._alpha_planes(20, 16, 5, 2)[0] != 1])) and not np.any(np.signbit(out[7:9, 7:13]))


@pytest.mark.parametrize("shape", [(1, 1, 5, 2), (9, 3, 5, 2), (11, 11, 3, 4), (14, 14, 5, 2), (15, 17, 1, 0), (23, 19, 9, 20), (30, 26, 5, 2)],
                         ids=lambda s: "%dx%d-tw%d-bw%d" % s)
@pytest.mark.parametrize("use_outer", [True, False])
def test_vectorised_border_smooth_is_the_cell_by_cell_loop(shape, use_outer):
    """border_smooth against :129-139 written as the reference's loop over linear_smoothing"""
    nx, ny, tw, bw = shape
    rng = np.random.default_rng(nx * 100 + ny)
    I = rng.normal(280, 5, (2, ny, nx)).astype(np.float32)
    O = rng.normal(280, 5, (2, ny, nx)).astype(np.float32)
    I[rng.random(I.shape) < 0.1] = np.nan
    O[rng.random(O.shape) < 0.1] = np.nan
    O[0, 0, 0] = I[0, 0, 0]
    I.flat[1 % I.size] = np.inf
    O.flat[2 % O.size] = -np.inf
    got = mr.border_smooth(I, O, tw, bw, use_outer)
    want = np.empty_like(I)
    for z in range(2):
        for y in range(ny):
            for x in range(nx):
                vI, vO = np.float64(I[z, y, x]), np.float64(O[z, y, x])
                if np.isnan(vI):
                    m = vO if use_outer else np.float64(np.nan)
                elif np.isnan(vO):
                    m = vI
                else:
                    m = mr.linear_smoothing(nx, ny, tw, bw, x, y, vI, vO)[0]
                want[z, y, x] = np.float32(m)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))


def test_overlay():
    nan = np.float32(np.nan)
    top = np.array([1, nan, nan, -0.0, np.inf], np.float32)
    base = np.array([5, 6, nan, 7, nan], np.float32)
    got = mr.overlay(top, base)
    assert np.array_equal(got.view(np.uint32)[[0, 1, 3, 4]], np.array([1, 6, -0.0, np.inf], np.float32).view(np.uint32)) and np.isnan(got[2])
