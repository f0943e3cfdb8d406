"""The forward aggregation rules the HIP kernels compile (fimex_amd/csrc/forward_math.hpp: the ordered and the padded step with their
finishes, the median by rank, by key selection and of at most two values, the key mapping, RoundAndClamp) run here on the CPU:
tests/forward_math_host.hip uses the header the way the kernels do and fimex_amd/build.py compiles it for the host only.  Every bucket
must equal the oracle's CachedForwardInterpolation bit for bit, the sign of zero and the places of NaN included.  No GPU is involved."""
import ctypes

import numpy as np
import pytest

import cases
import oracle
from fimex_amd import build as fb

# both sides of the tiled kernel's group of 8, of the wave of 64 and of the median kernels' Q = 2 registers per lane, and beyond
LENGTHS = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 100, 129]
SEEDS = [1, 2, 3]
FORWARD = list(range(oracle.FWD_SUM, oracle.FWD_UNDEF_MIN + 1))
MEDIANS = (oracle.FWD_MEDIAN, oracle.FWD_UNDEF_MEDIAN)
ZERO_KEY, DROPPED_KEY = 0x80000000, 0xFFFFFFFF
_P = ctypes.c_void_p


def aggregate_of(method):
    """(Aggregate of plan.hpp, UNDEF) of an oracle method number"""
    return (method - oracle.FWD_SUM) % 5, method >= oracle.FWD_UNDEF_SUM


@pytest.fixture(scope="module")
def shim():
    lib = ctypes.CDLL(fb.build_forward_math_host())
    buckets = [_P, _P, ctypes.c_int64, _P]
    for name, args, res in [("forward_math_ordered", [ctypes.c_int, ctypes.c_int] + buckets, ctypes.c_int),
                            ("forward_math_padded", [ctypes.c_int, ctypes.c_int] + buckets, ctypes.c_int),
                            ("forward_math_median_by_rank", [ctypes.c_int] + buckets, None),
                            ("forward_math_median_of_two", [ctypes.c_int] + buckets, None),
                            ("forward_math_median_select", [ctypes.c_int] + buckets + [_P], None),
                            ("forward_math_keys", [_P, ctypes.c_int64, _P, _P], None),
                            ("forward_math_targets", [_P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _P, _P], None)]:
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    return lib


def _slices(lengths, seed):
    """One slice per kind of content, each [cells of all buckets]: what the rules must get right."""
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(int)
    mid = [s + l // 2 for s, l in zip(starts, lengths) if l]
    first = [s for s, l in zip(starts, lengths) if l]
    out = []
    plain = (280 + rng.normal(0, 5, n)).astype(np.float32)
    out.append(plain)
    for where in (first, mid):   # a NaN first, a NaN in the middle
        f = plain.copy(); f[where] = np.nan; out.append(f)
    out.append(np.full(n, np.nan, np.float32))
    for a, b in ((0.0, -0.0), (-0.0, 0.0)):   # zeros of both signs, in both orders
        f = np.where(np.arange(n) % 2 == 0, np.float32(a), np.float32(b)).astype(np.float32); f[first] = np.float32(a); out.append(f)
    out.append(rng.choice(np.array([-1.0, -0.0, 0.0, 1.0, 0.0, -0.0], np.float32), n))   # a zero of either sign as the median, the extremum
    out.append(rng.choice(np.array([1.5, 2.5, 2.5, 3.5], np.float32), n))                  # runs of equal values
    f = plain.copy(); f[rng.random(n) < 0.1] = np.inf; f[rng.random(n) < 0.1] = -np.inf; out.append(f)   # the sum is NaN on both sides
    out.append((rng.integers(-40, 41, n) * np.float32(1e-45)).astype(np.float32))         # denormals, a few zeros among them
    f = plain.copy(); f[rng.random(n) < 0.25] = np.nan; f[rng.random(n) < 0.1] = np.float32(-0.0); out.append(f)
    return out


@pytest.fixture(scope="module")
def buckets():
    """The buckets, their contents, and the oracle's result for every method: a one-row source whose cell i lies in target px[i]."""
    rng = np.random.default_rng(0)
    lengths = LENGTHS + [int(l) for l in rng.permutation(LENGTHS)]   # every length after a shorter and after a longer bucket
    tgt = np.concatenate([np.full(l, i) for i, l in enumerate(lengths)])
    nowhere = np.sort(rng.choice(tgt.size, 9, replace=False))
    px = np.insert(tgt.astype(np.float64), nowhere, -5.0)               # a few cells that map nowhere, among the others
    mapped = px >= 0
    f = np.full((len(SEEDS) * 11, px.size), 12345.0, np.float32)
    f[:, mapped] = np.stack([s for seed in SEEDS for s in _slices(lengths, seed)])
    want = {m: oracle.forward_interpolate_values(m, px, np.zeros_like(px), f, px.size, 1, len(lengths), 1)[:, 0, :] for m in FORWARD}
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    return {"lengths": np.array(lengths), "offsets": offsets, "values": np.ascontiguousarray(f[:, mapped]), "want": want}


def run(shim, entry, b, *head, keys=False):
    nb = b["lengths"].size
    out = np.full((b["values"].shape[0], nb), -777.0, np.float32)
    k = np.zeros(out.shape, np.uint32)
    for z, v in enumerate(b["values"]):
        tail = (k[z].ctypes.data,) if keys else ()
        rc = getattr(shim, entry)(*head, v.ctypes.data, b["offsets"].ctypes.data, nb, out[z].ctypes.data, *tail)
        assert not rc
    return (out, k) if keys else out


def assert_same_bits(got, want):
    assert cases.same(got, want), cases.describe_mismatch(got, want)
    assert np.array_equal(np.signbit(got[~np.isnan(got)]), np.signbit(want[~np.isnan(want)]))


@pytest.mark.parametrize("method", [m for m in FORWARD if m not in MEDIANS])
def test_ordered_and_padded_steps_match_the_oracle(shim, buckets, method):
    a, u = aggregate_of(method)
    ordered = run(shim, "forward_math_ordered", buckets, a, int(u))
    assert_same_bits(ordered, buckets["want"][method])
    padded = run(shim, "forward_math_padded", buckets, a, int(u))
    assert_same_bits(padded, ordered)
    assert_same_bits(padded, buckets["want"][method])
    assert np.isnan(ordered[:, buckets["lengths"] == 0]).all()


@pytest.mark.parametrize("method", MEDIANS)
def test_medians_match_the_oracle(shim, buckets, method):
    u = int(aggregate_of(method)[1])
    want = buckets["want"][method]
    ranked = run(shim, "forward_math_median_by_rank", buckets, u)
    assert_same_bits(ranked, want)
    short = buckets["lengths"] <= 2
    assert_same_bits(run(shim, "forward_math_median_of_two", buckets, u)[:, short], want[:, short])
    # by selection on keys: the value where the median is no zero, the zeros' common key where it is one (the kernel then picks by position)
    selected, keys = run(shim, "forward_math_median_select", buckets, u, keys=True)
    zero = want == 0
    assert zero.any() and (~zero & ~np.isnan(want)).any() and np.isnan(want).any()
    assert_same_bits(selected[~zero], want[~zero])
    assert (keys[zero] == ZERO_KEY).all() and (keys[np.isnan(want)] == DROPPED_KEY).all() and (keys[~zero & ~np.isnan(want)] != ZERO_KEY).all()


def test_the_dispatcher_leaves_the_median_to_its_own_kernels(shim, buckets):
    out = np.zeros(buckets["lengths"].size, np.float32)
    for entry in ("forward_math_ordered", "forward_math_padded"):
        assert getattr(shim, entry)(2, 0, buckets["values"][0].ctypes.data, buckets["offsets"].ctypes.data, out.size, out.ctypes.data) == -1


def test_keys_order_as_the_floats_do(shim):
    fmax, tiny = np.finfo(np.float32).max, np.float32(1e-45)
    v = np.array([-np.inf, -fmax, -281.5, -1.0, -1.0, -1e-38, -2 * tiny, -tiny, -0.0, 0.0, -0.0, tiny, 2 * tiny, 1e-38, 1.0, 1.0, 281.5, fmax, np.inf], np.float32)
    assert (np.diff(v) >= 0).all()
    keys, bits = np.zeros(v.size, np.uint32), np.zeros(v.size, np.uint32)
    shim.forward_math_keys(v.ctypes.data, v.size, keys.ctypes.data, bits.ctypes.data)
    assert np.array_equal(np.diff(keys.astype(np.int64)) > 0, np.diff(v) > 0) and (np.diff(keys.astype(np.int64)) >= 0).all()
    assert (keys[v == 0] == ZERO_KEY).all() and (keys[v != 0] != ZERO_KEY).all() and (keys < DROPPED_KEY).all()
    assert np.array_equal(bits[v != 0], v.view(np.uint32)[v != 0])
    assert (bits[v == 0] == 0).all()


@pytest.mark.parametrize("n", [7, 1])
def test_round_clamp_names_the_oracles_target_cells(shim, n):
    pos = np.concatenate([cases.SPECIAL, [0.0, -0.0, 0.5, -0.5, -0.4999999, -0.5000001, 1.5, 2.5, -1.0, n - 1.0, n - 0.5, n - 0.5000001, n - 1.5, n * 1.0,
                                          2.0 ** 30, -(2.0 ** 30), 2.0 ** 30 - 1, 3.49999999, 0.49999999999999994]])
    ones, zeros = np.ones(pos.size, np.float32), np.zeros(pos.size)
    rx, tgt = np.zeros(pos.size, np.int64), np.zeros(pos.size, np.uint32)
    for px, py, ox, oy in ((pos, zeros, n, 1), (zeros, pos, 1, n), (pos, pos[::-1].copy(), n, n)):
        want = oracle.forward_interpolate_values(oracle.FWD_SUM, px, py, ones, pos.size, 1, ox, oy).ravel()   # cells per target, NaN for none
        shim.forward_math_targets(px.ctypes.data, py.ctypes.data, pos.size, ox, oy, rx.ctypes.data, tgt.ctypes.data)
        assert ((rx >= -1) & (rx < ox)).all() and ((rx == -1) <= (tgt == 0xFFFFFFFF)).all()
        assert (tgt[tgt != 0xFFFFFFFF] < ox * oy).all()
        got = np.bincount(tgt[tgt != 0xFFFFFFFF], minlength=ox * oy).astype(np.float32)
        got[got == 0] = np.nan
        assert cases.same(got, want), cases.describe_mismatch(got, want)
