"""tests/derived_ref.py, the yardstick of tests/test_gpu_derived.py, pinned: the humidity function to the reference's own object code
(oracle/_ref/libmifi_ref.so, where build() made it) and everything to the recorded answers of tests/golden/derived_answers.npz
(scripts/record_derived_answers.py).  ScaleValue, the theta2T loop, the packing to short and the accumulation are C++ behind boost:
for them the restatement is the only pin, and a handful of values worked out by hand from the reference's text stand next to it.
CPU only."""
import numpy as np
import pytest

import derived_ref as dr


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dr.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def live():
    lib = dr.reference_lib()
    if lib is None:
        pytest.skip("oracle/_ref/libmifi_ref.so is absent: no reference tree was at hand when build() ran")
    return lib


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(dr.as_bytes(a), dr.as_bytes(b))


# ------------------------------------------------------------------ worked by hand
def test_round_is_half_away_from_zero_with_the_wrap_of_int():
    d = np.array([0.5, -0.5, 1.5, -1.5, 2.5, 0.49999999999999994, -0.0, 2147483647.5, -2147483648.5, 4294967296.0 + 7, 1e19, -1e19, np.nan,
                  np.inf])
    want = np.array([1, -1, 2, -2, 3, 0, 0, -2147483648, 2147483647, 7, 0, 0, 0, 0], np.int32)
    assert np.array_equal(dr.mifi_round(d), want)


def test_scaled_conversion_by_hand():
    x = np.array([-32767, 0, 1, 3, -3, 100], np.int16)
    # unpacking: fill -> NaN, else 0.5 * x + 10 as float
    got = dr.convert_scaled(x, -32767.0, 0.5, 10.0, dr.CDM_FLOAT, np.nan)
    assert np.isnan(got[0]) and np.array_equal(got[1:], np.array([10, 10.5, 11.5, 8.5, 60], np.float32)) and got.dtype == np.float32
    # packing with newScale != 1: a = 0.25, b = (10 - 0.5) / 2 = 4.75; 5.5 -> 6 and 4.0 stays
    got = dr.convert_scaled(x, -32767.0, 0.5, 10.0, dr.CDM_CHAR, -128.0, 2.0, 0.5)
    assert np.array_equal(got, np.array([-128, 5, 5, 6, 4, 30], np.int8))  # 4.75 -> 5, 5.0, 5.5 -> 6, 4.0, 29.75 -> 30
    # past the range of the output: (signed char)(int)300 = 44, (unsigned char)(int)-3 = 253
    got = dr.convert_scaled(np.array([300.0, -3.0, np.nan], np.float64), np.nan, 1.0, 0.0, dr.CDM_CHAR, 7.0)
    assert np.array_equal(got, np.array([44, -3, 7], np.int8))
    got = dr.convert_scaled(np.array([300.0, -3.0], np.float32), np.nan, 1.0, 0.0, dr.CDM_UCHAR, 7.0)
    assert np.array_equal(got, np.array([44, 253], np.uint8))
    # a fill that IN cannot hold means no fill; one that OUT cannot hold is refused
    got = dr.convert_scaled(np.array([-128, 127], np.int8), 1000.0, 1.0, 0.0, dr.CDM_DOUBLE, np.nan)
    assert np.array_equal(got, np.array([-128.0, 127.0]))
    with pytest.raises(ValueError):
        dr.convert_scaled(x, 0.0, 1.0, 0.0, dr.CDM_SHORT, np.nan)
    with pytest.raises(ValueError):
        dr.convert_scaled(x, 0.0, 1.0, 0.0, dr.CDM_UCHAR, 256.0)
    with pytest.raises(ValueError):
        dr.convert_scaled(x, 0.0, 1.0, 0.0, dr.CDM_FLOAT, 1e39)
    assert np.isinf(dr.convert_scaled(x, -32767.0, 1.0, 0.0, dr.CDM_FLOAT, np.inf)[0])
    with pytest.raises(ValueError):
        dr.convert_scaled(x, 0.0, 1.0, 0.0, dr.CDM_STRING, 0.0)


def test_float_output_is_the_double_output_rounded_once():
    """->asFloat() of getScaledDataSliceInUnit's doubles: the same two roundings as outType FLOAT."""
    x = dr.scaled_values(np.int16, 500, 1, -32767)
    d = dr.convert_scaled(x, -32767.0, 0.01 * 1.0, 1.0 * 273.15 + 0.0, dr.CDM_DOUBLE, np.nan)
    f = dr.convert_scaled(x, -32767.0, 0.01 * 1.0, 1.0 * 273.15 + 0.0, dr.CDM_FLOAT, np.nan)
    assert _same_bits(d.astype(np.float32), f)


def test_packing_outside_short():
    got = dr.pack_relative_humidity(np.array([np.nan, 1.4, 3.0, 0.0, 1.0, 0.5], np.float32))
    assert np.array_equal(got, np.array([0, -30536, 9464, 0, 25000, 12500], np.int16))


def test_accumulate_by_hand():
    nan = np.nan
    x = np.array([[nan, 1.0], [2.0, nan], [3.0, 4.0]], np.float32)
    acc = dr.accumulate(x)
    assert np.isnan(acc[0, 0]) and acc[1, 0] == 2.0 and acc[2, 0] == 5.0  # the NaN of position 0 is kept there and counts as 0 after
    assert acc[0, 1] == 1.0 and np.isnan(acc[1, 1]) and np.isnan(acc[2, 1])  # a later NaN stays
    de = dr.deaccumulate(x)
    assert np.isnan(de[0, 0]) and de[1, 0] == 2.0 and de[2, 0] == 1.0
    assert de[0, 1] == 1.0 and np.isnan(de[1, 1]) and np.isnan(de[2, 1])
    # a batch split in two with the carry is the whole batch
    for split in (1, 2):
        assert _same_bits(np.concatenate([dr.accumulate(x[:split]), dr.accumulate(x[split:], split, acc[split - 1])]), acc)
        assert _same_bits(np.concatenate([dr.deaccumulate(x[:split]), dr.deaccumulate(x[split:], split, x[split - 1])]), de)
    with pytest.raises(ValueError):
        dr.accumulate(x, 1)


# ------------------------------------------------------------------ the reference's object code
def test_humidity_against_the_live_library(live):
    q, t, p = dr.recorded_humidity_inputs()
    assert _same_bits(dr.specific_to_relative(q, t, p), live.specific_to_relative(q, t, p))
    rng = np.random.default_rng(5)
    q, t = dr.humidity_inputs(6, (3000,))
    p = rng.uniform(10.0, 1050.0, 3000).astype(np.float32)
    got, want = dr.specific_to_relative(q, t, p), live.specific_to_relative(q, t, p)
    assert _same_bits(got, want)
    assert np.isnan(want).any() and (want == 100).any() and ((want > 0) & (want < 100)).mean() > 0.3


def test_recording_is_reproducible(live, fixture):
    q, t, p = fixture["humidity.q"], fixture["humidity.t"], fixture["humidity.p"]
    assert _same_bits(live.specific_to_relative(q, t, p).view(np.uint32), fixture["humidity.rh"])


# ------------------------------------------------------------------ the recorded answers
def test_recorded_humidity(fixture):
    q, t, p = fixture["humidity.q"], fixture["humidity.t"], fixture["humidity.p"]
    rh = dr.specific_to_relative(q, t, p)
    assert _same_bits(rh.view(np.uint32), fixture["humidity.rh"])
    assert _same_bits(dr.pack_relative_humidity(rh), fixture["humidity.packed"])
    assert _same_bits(dr.pack_relative_humidity(fixture["pack.rh"]), fixture["pack.packed"])


def test_recorded_theta(fixture):
    got = dr.theta_to_temperature(fixture["theta.theta"], fixture["theta.p"], float(fixture["theta.add_offset"]))
    assert _same_bits(got.view(np.uint32), fixture["theta.T"])


@pytest.mark.parametrize("variant", dr.RECORDED_SCALED_VARIANTS)
@pytest.mark.parametrize("inType", dr.TYPES)
def test_recorded_scaled_conversion(fixture, inType, variant):
    x = fixture["scaled.in.%d.v%d" % (inType, variant)]
    assert x.dtype == np.dtype(dr.DTYPES[inType])
    for o in dr.TYPES:
        par = [float(v) for v in fixture["scaled.par.%d.%d.v%d" % (inType, o, variant)]]
        got = dr.convert_scaled(x, par[0], par[1], par[2], o, par[3], par[4], par[5])
        assert got.dtype == np.dtype(dr.DTYPES[o])
        assert np.array_equal(dr.as_bytes(got), fixture["scaled.out.%d.%d.v%d" % (inType, o, variant)]), (inType, o, variant)


@pytest.mark.parametrize("code", dr.RECORDED_ACCUMULATE_TYPES)
def test_recorded_accumulation(fixture, code):
    x = fixture["accumulate.%d.in" % code]
    assert _same_bits(dr.accumulate(x).view(np.uint64), fixture["accumulate.%d.acc" % code])
    assert _same_bits(dr.deaccumulate(x).view(np.uint64), fixture["accumulate.%d.deacc" % code])
