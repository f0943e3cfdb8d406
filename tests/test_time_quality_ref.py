"""tests/time_quality_ref.py, the yardstick of tests/test_gpu_time_quality.py, pinned: the blend to the reference's own object code
(oracle/_ref/libmifi_ref.so, where build() made it) and everything to the recorded answers of tests/golden/time_quality_answers.npz
(scripts/record_time_quality_answers.py).  The slice mapping and the quality mask are C++ behind boost: for them the restatement is
the only pin, and cases worked out by hand from the reference's text stand next to it.  fimex_amd_time_mapping runs on the CPU and
is checked here through libfimex_amd.so.  CPU only."""
import numpy as np
import pytest

import time_quality_ref as tq

NAN = np.nan


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return tq.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def live():
    lib = tq.reference_lib()
    if lib is None:
        pytest.skip("oracle/_ref/libmifi_ref.so is absent: no reference tree was at hand when build() ran")
    return lib


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(tq.as_bytes(a), tq.as_bytes(b))


def _is_undefined(a):
    return np.all(np.asarray(a, np.float32).view(np.uint32) == tq.UNDEFINED_F_BITS)


# ------------------------------------------------------------------ the time axis, worked by hand
def test_fine_axis_by_hand():
    """Old times 0, 6, 12, 18 and new times -9, -7.5, ..., 33: pair, f and branch from the reference's text."""
    old, new = tq.AXES["fine"]
    assert new.size == 29 and new[0] == -9.0 and new[1] == -7.5 and new[-1] == 33.0
    t1, t2 = tq.time_mapping(old, new)
    by_hand = {-9.0: ((0, 1), -1.5, tq.UNDEFINED), -6.0: ((0, 1), -1.0, tq.BLEND), 0.0: ((0, 1), 0.0, tq.COPY_A),
               6.0: ((0, 1), 1.0, tq.COPY_B), 7.5: ((1, 2), 0.25, tq.BLEND), 24.0: ((2, 3), 2.0, tq.BLEND),
               25.5: ((2, 3), 2.25, tq.UNDEFINED), 33.0: ((2, 3), 3.5, tq.UNDEFINED)}
    for x, (pair, f, branch) in by_hand.items():
        i = int(np.flatnonzero(new == x)[0])
        assert (int(t1[i]), int(t2[i])) == pair, x
        got_f, got_branch = tq.blend_factor(old[pair[0]], old[pair[1]], x)
        assert got_f == np.float32(f) and got_branch == branch, x
    # every step of the axis: lower_bound gives the first old time >= x, so x on an old time belongs to the pair below it
    want = [(0, 1)] * 11 + [(1, 2)] * 4 + [(2, 3)] * 14
    assert list(zip(t1.tolist(), t2.tolist())) == want
    A = np.array([[1.0, NAN], [3.0, 10.0], [NAN, 20.0], [7.0, 40.0]], np.float32)
    out = tq.time_interpolate(A, old, new)
    at = {float(x): out[i] for i, x in enumerate(new)}
    assert _is_undefined(at[-9.0]) and _is_undefined(at[-7.5]) and _is_undefined(at[25.5]) and _is_undefined(at[33.0])
    assert at[-6.0][0] == -1.0 and np.isnan(at[-6.0][1])           # 1 + -1 * (3 - 1)
    assert _same_bits(at[0.0], A[0]) and _same_bits(at[6.0], A[1])  # copies
    assert at[12.0][1] == 20.0 and np.isnan(at[12.0][0])            # f == 1 on (1, 2): a copy of slice 2, its NaN included
    assert at[7.5][1] == 12.5 and np.isnan(at[7.5][0])              # 10 + 0.25 * (20 - 10); NaN in B of a blend
    assert at[24.0][1] == 60.0                                      # 20 + 2 * (40 - 20)


def test_copies_do_not_leak_the_other_slice():
    A = np.array([[1.0, NAN], [NAN, 2.0]], np.float32)
    out = tq.time_interpolate(A, [0.0, 1.0], [0.0, 1.0])
    assert _same_bits(out[0], A[0]) and _same_bits(out[1], A[1])


def test_single_old_time():
    old, new = tq.AXES["single"]
    t1, t2 = tq.time_mapping(old, new)
    assert t1.tolist() == [0, 0, 0] and t2.tolist() == [0, 0, 0]
    x = np.array([[3, -4, 5]], np.int16)
    out = tq.time_interpolate(x, old, new)  # a == b: f = 0, a copy of asFloat()
    assert out.dtype == np.float32 and np.array_equal(out, np.tile(np.array([3, -4, 5], np.float32), (3, 1)))


def test_backwards_axis_keeps_the_search_start():
    """lastPos is the previous pos, so after 13 (pos 3) the search for 2 starts at 3: pair (2, 3), f = (2 - 12) / 6, undefined."""
    old, new = tq.AXES["backwards"]
    t1, t2 = tq.time_mapping(old, new)
    assert list(zip(t1.tolist(), t2.tolist())) == [(2, 3)] * 7
    und = tq.undefined_positions(old, new)
    assert und.tolist() == [False, True, False, False, True, False, False]  # f = 1/6, -5/3, -5/6, 1, -3/2, 0, -1
    assert tq.blend_factor(12.0, 18.0, 6.0) == (np.float32(-1.0), tq.BLEND)


def test_coarser_axis_skips_slices():
    old, new = tq.AXES["coarse"]
    t1, t2 = tq.time_mapping(old, new)
    assert list(zip(t1.tolist(), t2.tolist())) == [(0, 1), (0, 1), (3, 4), (3, 4), (5, 6), (5, 6)]
    assert any(int(a) != int(b) and int(a) != int(p) for a, b, p in zip(t1[1:], t2[1:], t2[:-1]))
    assert tq.undefined_positions(old, new).tolist() == [False] * 5 + [True]  # 30: f = 5 on (15, 18)


def test_mapping_refuses_what_the_library_refuses():
    for old in ([], [1.0, 1.0], [2.0, 1.0], [0.0, NAN], [NAN]):
        with pytest.raises(ValueError):
            tq.time_mapping(old, [0.0])


# ------------------------------------------------------------------ fimex_amd_time_mapping, on the CPU
@pytest.mark.parametrize("axis", sorted(tq.AXES))
def test_library_mapping_equals_the_restatement(axis):
    """Through libfimex_amd.so on a machine without a GPU."""
    from fimex_amd import capi
    old, new = tq.AXES[axis]
    t1, t2 = capi.time_mapping(old, new)
    want1, want2 = tq.time_mapping(old, new)
    assert np.array_equal(t1, want1) and np.array_equal(t2, want2)


def test_library_mapping_on_random_axes():
    from fimex_amd import capi
    rng = np.random.default_rng(11)
    for nOld in (1, 2, 3, 40):
        old = np.cumsum(rng.uniform(0.5, 3.0, nOld))
        new = rng.uniform(old[0] - 5.0, old[-1] + 5.0, 200)
        new[::9] = rng.choice(old, new[::9].size)  # on an old time
        for axis in (np.sort(new), new):
            t1, t2 = capi.time_mapping(old, axis)
            want1, want2 = tq.time_mapping(old, axis)
            assert np.array_equal(t1, want1) and np.array_equal(t2, want2), nOld
    t1, t2 = capi.time_mapping([1.0, 2.0], [])
    assert t1.size == 0 and t2.size == 0


# ------------------------------------------------------------------ the mask, worked by hand
DATA = np.array([[10, 11, 12, 13, 14, 15], [20, 21, 22, 23, 24, 25], [30, 31, 32, 33, 34, 35]], np.int16)  # nData = 3 * nStatus
STATUS = np.array([2.0, NAN, 9.0, 5.0, 0.0, 7.0])  # 9 is the statusFill below, 0 lies under validMin
FLAGS = {"validMin": 1.0, "validMax": 20.0, "statusFill": 9.0}
BY_HAND = {
    tq.VALUES: ({"values": (7.0, 2.0), "statusFill": 2.0, "validMin": 3.0}, [0, 1, 1, 1, 1, 0]),  # the three flag arguments are ignored
    tq.ALL: (FLAGS, [0, 1, 1, 0, 1, 0]),
    tq.MAX: (dict(FLAGS, limit=5.0), [0, 1, 1, 0, 1, 1]),  # 5 is not above 5
    tq.MIN: (dict(FLAGS, limit=5.0), [1, 1, 1, 0, 1, 0]),
    tq.HIGHEST: (FLAGS, [1, 1, 1, 1, 1, 0]),               # 9 is the fill: the highest defined status is 7
    tq.LOWEST: (FLAGS, [0, 1, 1, 1, 1, 1]),                # 0 is below validMin: the lowest defined status is 2
}


@pytest.mark.parametrize("mode", tq.MODES)
def test_mask_by_hand(mode):
    kw, masked = BY_HAND[mode]
    masked = np.array(masked, bool)
    assert np.array_equal(tq.masked_status(STATUS, mode, **kw), masked)
    got = tq.quality_mask(DATA, STATUS, mode, -32767.0, **kw)
    want = DATA.copy()
    want[:, masked] = -32767
    assert _same_bits(got, want)
    assert np.array_equal(DATA[0], [10, 11, 12, 13, 14, 15])  # the input is left alone


def test_mask_without_a_defined_status_takes_everything():
    s = np.array([NAN, 9.0, 0.5])
    for mode in (tq.HIGHEST, tq.LOWEST, tq.ALL):
        assert tq.masked_status(s, mode, **FLAGS).all()


def test_mask_own_status():
    x = np.array([1.0, NAN, 4.0, 2.0], np.float32)
    got = tq.quality_mask(x, None, tq.MAX, -1.0, limit=2.0)
    assert np.array_equal(got, np.array([1.0, -1.0, -1.0, 2.0], np.float32))


def test_fill_is_rounded_half_away_from_zero():
    assert tq.cast_fill(2.5, np.int16) == 3 and tq.cast_fill(-2.5, np.int16) == -3 and tq.cast_fill(0.49999999999999994, np.int8) == 0
    assert tq.cast_fill(-0.5, np.int32) == -1 and tq.cast_fill(127.4, np.int8) == 127 and tq.cast_fill(254.5, np.uint8) == 255
    assert tq.cast_fill(4294967295.0, np.uint32) == 4294967295  # through int and back
    assert tq.cast_fill(1e40, np.float64) == 1e40 and np.isnan(tq.cast_fill(NAN, np.float32)) and np.isinf(tq.cast_fill(np.inf, np.float32))
    got = tq.quality_mask(np.array([1, 2], np.int8), np.array([NAN, 1.0]), tq.ALL, -1.5)
    assert np.array_equal(got, np.array([-2, 2], np.int8))


@pytest.mark.parametrize("fill,dtype", [(127.5, np.int8), (-129.0, np.int8), (256.0, np.uint8), (-1.0, np.uint16), (NAN, np.int32),
                                         (3e9, np.int32), (1e10, np.int64), (-1.0, np.uint64), (1e39, np.float32), (np.inf, np.int16)])
def test_fill_the_type_cannot_hold_raises(fill, dtype):
    with pytest.raises(ValueError):
        tq.cast_fill(fill, dtype)
    with pytest.raises(ValueError):
        tq.quality_mask(np.zeros(4, dtype), np.zeros(4), tq.ALL, fill)


def test_mask_refuses_what_the_library_refuses():
    with pytest.raises(ValueError):
        tq.quality_mask(DATA, STATUS[:4], tq.ALL, 0.0)  # 18 cells against 4
    with pytest.raises(ValueError):
        tq.quality_mask(DATA, STATUS, tq.VALUES, 0.0)   # an empty list
    with pytest.raises(ValueError):
        tq.quality_mask(DATA, STATUS, tq.VALUES, 0.0, values=(1.0, NAN))
    with pytest.raises(ValueError):
        tq.quality_mask(DATA, STATUS, 6, 0.0)


# ------------------------------------------------------------------ the reference's object code
def test_blend_against_the_live_library(live):
    A, B = tq.recorded_blend_fields()
    rng = np.random.default_rng(12)
    cases = [(0.0, 6.0, x) for x in np.arange(-9.0, 34.0, 0.75)] + [(5.0, 5.0, 1.0), (6.0, 0.0, 3.0), (0.0, 3.0, NAN)]
    cases += [tuple(rng.uniform(-10.0, 10.0, 3)) for _ in range(200)]
    branches = set()
    for a, b, x in cases:
        assert _same_bits(tq.blend(A, B, a, b, x), live.blend(A, B, a, b, x)), (a, b, x)
        branches.add(tq.blend_factor(a, b, x)[1])
    assert branches == {tq.COPY_A, tq.COPY_B, tq.BLEND, tq.UNDEFINED}


def test_recording_is_reproducible(live, fixture):
    A, B = fixture["blend.A"], fixture["blend.B"]
    for k, (a, b, x) in enumerate(fixture["blend.abx"]):
        assert _same_bits(live.blend(A, B, a, b, x).view(np.uint32), fixture["blend.out"][k])


# ------------------------------------------------------------------ the recorded answers
def test_recorded_blend(fixture):
    A, B = fixture["blend.A"], fixture["blend.B"]
    assert len(fixture["blend.abx"]) >= 16
    for k, (a, b, x) in enumerate(fixture["blend.abx"]):
        assert _same_bits(tq.blend(A, B, a, b, x).view(np.uint32), fixture["blend.out"][k]), (a, b, x)


@pytest.mark.parametrize("axis", sorted(tq.AXES))
def test_recorded_series(fixture, axis):
    old, new = fixture["mapping.%s.old" % axis], fixture["mapping.%s.new" % axis]
    assert np.array_equal(old, tq.AXES[axis][0]) and np.array_equal(new, tq.AXES[axis][1])
    t1, t2 = tq.time_mapping(old, new)
    assert np.array_equal(t1, fixture["mapping.%s.t1" % axis]) and np.array_equal(t2, fixture["mapping.%s.t2" % axis])
    codes = [int(k.split(".")[2]) for k in fixture if k.startswith("series.%s." % axis) and k.endswith(".in")]
    assert len(codes) == 4
    for code in codes:
        x = fixture["series.%s.%d.in" % (axis, code)]
        assert x.dtype == np.dtype(tq.DTYPES[code])
        assert _same_bits(tq.time_interpolate(x, old, new).view(np.uint32), fixture["series.%s.%d.out" % (axis, code)]), code


@pytest.mark.parametrize("mode", tq.MODES)
def test_recorded_mask(fixture, mode):
    for c in tq.RECORDED_MASK_DATA:
        data = fixture["mask.data.%d" % c]
        for s in tq.RECORDED_MASK_STATUS:
            got = tq.quality_mask(data, fixture["mask.status.%d" % s], mode, 77.0, **tq.mode_arguments(mode))
            want = fixture["mask.out.%d.%d.m%d" % (c, s, mode)]
            assert np.array_equal(tq.as_bytes(got), want), (c, s, mode)
            changed = tq.as_bytes(got).reshape(-1, data.dtype.itemsize) != tq.as_bytes(data).reshape(-1, data.dtype.itemsize)
            assert 0 < changed.any(axis=1).sum() < data.size  # every rule takes some cells and leaves some
