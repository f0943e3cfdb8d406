"""tests/extract_ref.py against the reference's own expectations (test/testExtractor.cc) and against itself: where joinSlices'
concatenation is the row-major array and where it is not (divergence D9), reduceAxes on the sigma axis of coordTest.nc, and the
bounding box on that file's stored 2-D longitude / latitude.  CPU only."""
import numpy as np
import pytest

import extract_ref as ref

from extract_ref import BOXES, coordtest, random_reduction


def test_join_order_on_random_cases():
    rng = np.random.default_rng(20240611)
    same = differing = 0
    for _ in range(8000):
        dims = random_reduction(rng)
        a = np.arange(int(np.prod([d[0] for d in dims])))  # distinct values
        want, got = ref.pick(a, dims).ravel(), ref.reference_join(a, dims)
        assert got.size == want.size
        if ref.order_differs(dims):
            differing += 1
            assert not np.array_equal(got, want), dims
            assert np.array_equal(np.sort(got), np.sort(want)), dims  # the same elements in another order
        else:
            same += 1
            assert np.array_equal(got, want), dims
    assert same + differing >= 2000 and same >= 50 and differing >= 50, (same, differing)


def test_the_references_pick_expectations():
    """test/testExtractor.cc:67-123 on a synthetic [12][20][90] field: time reduced to neighbouring positions (reduceTime), y to
    {10, 11, 13, 16}, x to {80, 83} and then to a start and a length, shortened to 80..89 to fit the field."""
    field = np.arange(12 * 20 * 90, dtype=np.float32).reshape(12, 20, 90)
    data1 = field[:, 10:20, 80:90]  # precData1: x 80.., y 10..
    time, y = (12, np.arange(12), 0, 12), (20, [10, 11, 13, 16], 0, 4)
    pairs = [((0, 0), (0, 0)), ((3, 0), (1, 0)), ((0, 1), (0, 1)), ((3, 1), (1, 1)), ((0, 3), (0, 2)), ((3, 3), (1, 2)), ((0, 6), (0, 3)),
             ((3, 6), (1, 3))]  # :83-92, (x, y) in precData1 and in precData2
    dims = [(90, [80, 83], 0, 2), y, time]
    assert not ref.order_differs(dims)
    data2 = ref.reference_join(field, dims).reshape(12, 4, 2)
    assert np.array_equal(data2, ref.pick(field, dims))
    for t in range(12):
        for (x1, y1), (x2, y2) in pairs:
            assert data1[t, y1, x1] == data2[t, y2, x2]
    dims = [(90, np.arange(80, 90), 0, 10), y, time]  # reduceDimension("x", 80, 50), :101
    assert not ref.order_differs(dims)
    data2 = ref.reference_join(field, dims).reshape(12, 4, 10)
    assert np.array_equal(data2, ref.pick(field, dims))
    for t in range(12):
        for (x1, y1), (_, y2) in pairs:  # :114-123: the same x on both sides
            assert data1[t, y1, x1] == data2[t, y2, x1]


def test_axis_range():
    sigma = coordtest()["sigma"]
    np.testing.assert_allclose(sigma, [0.3, 0.5, 0.85, 1.0], rtol=1e-7)
    assert ref.axis_range(sigma, 0.5, 0.85) == (1, 2)       # test/testExtractor.cc:163-166
    assert ref.axis_range(sigma, -0.1, -0.05)[1] == 0       # :168-172
    assert ref.axis_range(sigma[::-1], 0.5, 0.85) == (1, 2)  # descending: 1.0, 0.85, 0.5, 0.3
    assert ref.axis_range(sigma[::-1], 0.85, 1.0) == (0, 2)
    assert ref.axis_range(sigma[::-1], 0.2, 0.3) == (3, 1)
    assert ref.axis_range([], 0.0, 1.0) == (0, 0)
    assert ref.axis_range([4.0], 4.0, 4.0) == (0, 1)
    assert ref.axis_range([4.0], 4.1, 5.0) == (1, 0)
    assert ref.axis_range([4.0], 5.0, 3.0) == (1, 0)  # end in front of start: size 0, not negative
    # two equal leading values: the delta is 1e-5, whatever follows
    assert ref.axis_range([1.0, 1.0, 2.0], 1.0 + 0.5e-5, 2.0 - 0.5e-5) == (0, 3)
    assert ref.axis_range([1.0, 1.0, 2.0], 1.0 + 2e-5, 2.0 - 2e-5) == (2, 0)
    # bounds exactly on value -+ delta (delta = 0.01 * 100, every sum exact): lower_bound and upper_bound both include the value
    axis = [0.0, 100.0, 200.0, 300.0]
    assert ref.axis_range(axis, 101.0, 199.0) == (1, 2)
    assert ref.axis_range(axis, 101.5, 198.5) == (2, 0)
    assert ref.axis_range(axis[::-1], 101.0, 199.0) == (1, 2)


@pytest.mark.parametrize("box,xs,ys", BOXES, ids=["inside", "across180", "empty"])
def test_bounding_box_on_the_stored_fields(box, xs, ys):
    c = coordtest()
    assert ref.bound_distance(c["lon"], c["lat"], *box) > 1e-3  # no stored point within rounding of a bound
    gx, gy = ref.bounding_box(c["lon"], c["lat"], *box)
    assert gx.tolist() == xs and gy.tolist() == ys
    if xs and box[2] < box[3]:
        keep = (c["lat"] >= box[0]) & (c["lat"] <= box[1]) & (c["lon"] >= box[2]) & (c["lon"] <= box[3])
        assert keep.sum() == 30


def test_bounding_box_leaves_failed_points_out():
    lon = np.array([[0.0, np.nan], [np.inf, 1.0]])
    lat = np.array([[50.0, 50.0], [50.0, np.nan]])
    gx, gy = ref.bounding_box(lon, lat, 40.0, 60.0, -10.0, 10.0)
    assert gx.tolist() == [0] and gy.tolist() == [0]
    gx, gy = ref.bounding_box(lon, lat, 40.0, 60.0, 10.0, -10.0)  # across 180: nothing but the failed points would be "inside"
    assert gx.tolist() == [] and gy.tolist() == []
