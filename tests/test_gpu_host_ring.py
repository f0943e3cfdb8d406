"""The host transfer ring (csrc/hostpipe.hip) in both directions at every chunk, piece and slot-reuse boundary.  Every *_host entry
moves its data through it: plain copies in chunks of one pinned slot (host_to_device, device_to_host), slices in chunks of as many
as fit a slot and the float scratch, each chunk in pieces (pipelined_slices), three slots in turn, a slot used again once the chunk
three places back has been drained.

The tuning build reads the ring's sizes from FIMEX_AMD_HOST_{SLOT,PIECE,FLOAT,STAGED_MIN}_BYTES, so most cases run a ring of
256 KiB slots and 32 KiB pieces on a few MB; three cases at the end run the product build's 64 MiB slots at the smallest sizes that
reach each branch.  The reference is never the ring: numpy on the caller's arrays for plain copies, the CPU oracle (or a numpy
gather of the oracle's own indices) for regrids, and besides the *_device twin of the entry on a resident copy.  Bit for bit, NaN
in the same cells, and the inputs unchanged after each call.  Which limit binds and how many chunks and pieces a case has is
asserted from the rule of csrc/hostpipe_layout.hpp itself (tests/hostpipe_layout_host.py), so that a change of constants cannot
move a case off its branch unnoticed."""
import ctypes
import threading
import time

import numpy as np
import pytest

import cases
import hostpipe_layout_host as layout
import oracle
from test_gpu_host_entries import _dev, _host, _identical, _stream, _unchanged

pytestmark = pytest.mark.gpu

SLOT, PIECE, SCRATCH, LEAST = 256 * 1024, 32 * 1024, 512 * 1024, 64 * 1024  # the shrunk ring, bytes
SMALL = (SLOT, PIECE, SCRATCH, LEAST)
SWITCHES = ("HOST_SLOT_BYTES", "HOST_PIECE_BYTES", "HOST_FLOAT_BYTES", "HOST_STAGED_MIN_BYTES")


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


@pytest.fixture(scope="module")
def rule():
    return layout.load()


@pytest.fixture
def ring(fa, tuning_build, monkeypatch):
    """set(sizes): the tuning build's ring works with these (slot, piece, float scratch, threshold) from the next call on"""
    def set_sizes(sizes=SMALL, **more):
        for name, value in zip(SWITCHES, sizes):
            monkeypatch.setenv("FIMEX_AMD_" + name, str(value))
        for name, value in more.items():
            monkeypatch.setenv("FIMEX_AMD_" + name, str(value))
        fa.release_caches()  # pipes keep the copy threads they were made with
    yield set_sizes
    fa.release_caches()


def test_the_switches_reach_the_ring(fa, ring):
    """sizes that need a ninth piece per slot are refused, by the call that would have used them"""
    ring((SLOT, SLOT // 8 - 4, SCRATCH, LEAST))
    a = np.ones(LEAST // 4, np.float32)
    with pytest.raises(fa.FimexAmdError, match="more pieces per slot"):
        fa.overlay_host(a, a)
    ring(SMALL)
    assert np.array_equal(fa.overlay_host(a, a), a)


# ------------------------------------------------------------------------------------------- 1. plain copies, both directions
def pattern(n, salt):
    """floats in [1, 2) whose mantissa is a hash of index + salt: a chunk from the wrong offset or a stale slot cannot pass"""
    k = (np.arange(n, dtype=np.uint32) + np.uint32(salt)) * np.uint32(2654435761)
    return ((k >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32)


def overlay_case(n, chunk):
    """top, base of n floats; NaN at the first and the last element of every chunk of `chunk` floats: in both arrays at the first,
    in top alone at the last"""
    top, base = pattern(n, 17), -pattern(n, 40503)
    first = np.arange(0, n, chunk)
    last = np.minimum(first + chunk - 1, n - 1)
    top[first] = np.nan
    base[first] = np.nan
    top[last] = np.nan
    return top, base


def check_overlay(fa, n, chunk, label):
    import torch
    top, base = overlay_case(n, chunk)
    copies = (top.copy(), base.copy())
    want = np.where(np.isnan(top), base, top)
    got = np.full(n, -7.0, np.float32)  # not np.empty: memory of an earlier, equal result must not stand in for a chunk never delivered
    fa._check(fa.load().fimex_amd_overlay_host(fa._fp(top), fa._fp(base), fa._fp(got), n))
    _unchanged((top, base), copies, label)
    _identical(got, want, label + ", numpy")
    d_top, d_base, d_out = _dev(top), _dev(base), torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    fa.overlay_device(d_top.data_ptr(), d_base.data_ptr(), d_out.data_ptr(), n, _stream())
    _identical(got, _host(d_out), label + ", device twin")


F = SLOT // 4  # floats per slot
PLAIN = {"threshold-1": LEAST // 4 - 1, "threshold": LEAST // 4, "slot-1": F - 1, "slot": F, "slot+1": F + 1, "3slots": 3 * F,
         "3slots+1": 3 * F + 1, "7slots+odd": 7 * F + 1235}


@pytest.mark.parametrize("name", list(PLAIN))
def test_plain_copies_on_the_shrunk_ring(fa, ring, rule, name):
    ring(SMALL)
    n = PLAIN[name]
    chunks = layout.byte_chunks(rule, SMALL, 4 * n)
    want_chunks = {"threshold-1": 1, "threshold": 1, "slot-1": 1, "slot": 1, "slot+1": 2, "3slots": 3, "3slots+1": 4, "7slots+odd": 8}[name]
    assert len(chunks) == want_chunks and (4 * n >= LEAST) == (name != "threshold-1"), (name, chunks)
    check_overlay(fa, n, F, "overlay_host, %s (%d floats, %d chunks)" % (name, n, len(chunks)))


# --------------------------------------------------------------------------------------------- 2. slices through apply_host
# (inX, inY, outX, outY) by which side is heavy and the slices per chunk; the output chunks come in every kind: exactly one piece,
# whole pieces, whole pieces and a tail shorter than 4096 bytes, less than a piece
SHAPES = {
    ("input", 1): (200, 180, 128, 64), ("input", 2): (160, 150, 40, 30), ("input", 5): (110, 110, 37, 29),
    ("output", 1): (40, 30, 256, 256), ("output", 2): (40, 30, 200, 123), ("output", 5): (37, 29, 140, 82),
    ("both", 1): (200, 180, 250, 200), ("both", 2): (160, 150, 200, 123), ("both", 5): (110, 110, 140, 82),
}


def piece_kind(rule, nbytes, piece=PIECE):
    p = layout.pieces(rule, nbytes, piece)
    tail = p[-1][1] if p[-1][1] < piece else 0
    if tail == 0:
        return "one piece" if len(p) == 1 else "whole pieces"
    return "less than a piece" if len(p) == 1 else ("pieces and a tail under 4096" if tail < 4096 else "pieces and a tail")


def nz_set(per):
    return sorted({1, per, per + 1, 3 * per, 3 * per + 1, 7 * per + 1})


def test_the_shapes_reach_every_kind_of_output_chunk(rule):
    kinds = set()
    for (heavy, per), (inX, inY, outX, outY) in SHAPES.items():
        fit, each, binding = layout.slices_per_chunk(rule, SMALL, 4 * inX * inY, 4 * outX * outY, 0, 0)
        assert fit == per, (heavy, per, fit, each)
        if heavy != "both":
            assert binding == {"input": layout.PIN_IN, "output": layout.PIN_OUT}[heavy] and each[1 - binding] > fit, (heavy, per, each)
        kinds.add(piece_kind(rule, per * 4 * outX * outY))
    assert kinds >= {"one piece", "whole pieces", "pieces and a tail under 4096", "less than a piece"}, kinds


_regrid_cache = {}


def regrid_case(method, shape, nz):
    """positions, nz source slices (NaN at the first and the last cell of each) and the oracle's answer: made once per shape and
    method for the longest batch, shorter batches are its first slices"""
    key = (method, shape)
    if key not in _regrid_cache or _regrid_cache[key][2].shape[0] < nz:
        inX, inY, outX, outY = shape
        px, py = cases.backward_positions(inX, inY, outX, outY, seed=inX + outX)
        f = cases.field(nz, inY, inX, seed=inY + outY)
        f[:, 0, 0] = np.nan
        f[:, -1, -1] = np.nan
        want = oracle.interpolate_values(method, px, py, f, inX, inY, outX, outY, nthreads=8)
        f.setflags(write=False)
        want.setflags(write=False)
        _regrid_cache[key] = (px, py, f, want)
    px, py, f, want = _regrid_cache[key]
    return px, py, f[:nz], want[:nz]


def check_apply_host(fa, plan, f, want, label, twin=True):
    import torch
    copy = f.copy()
    got, n = np.full(want.shape, -7.0, np.float32), ctypes.c_size_t(0)  # prefilled, as in check_overlay
    fa._check(fa.load().fimex_amd_regrid_apply_host(plan._h, fa._fp(np.ascontiguousarray(f)), f.size, fa._fp(got), got.size, ctypes.byref(n)))
    assert n.value == want.size
    _unchanged((f,), (copy,), label)
    _identical(got, want, label + ", oracle")  # every slice
    if twin:
        d_in, d_out = _dev(f), torch.full(want.shape, -7.0, dtype=torch.float32, device="cuda")
        plan.apply_device(d_in.data_ptr(), f.shape[0], d_out.data_ptr(), _stream())
        _identical(got, _host(d_out), label + ", device twin")


@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("heavy,per", list(SHAPES), ids=["%s-%d" % k for k in SHAPES])
def test_slices_on_the_shrunk_ring(fa, ring, rule, heavy, per, method):
    ring(SMALL)
    shape = SHAPES[(heavy, per)]
    inX, inY, outX, outY = shape
    assert layout.slices_per_chunk(rule, SMALL, 4 * inX * inY, 4 * outX * outY, 0, 0)[0] == per
    plan = fa.RegridPlan(method, *regrid_case(method, shape, 7 * per + 1)[:2], inX, inY, outX, outY)
    for nz in nz_set(per):
        px, py, f, want = regrid_case(method, shape, nz)
        n = len(layout.slice_chunks(rule, nz, per))
        assert n == -(-nz // per)
        check_apply_host(fa, plan, f, want, "apply_host %s-heavy, %d per chunk, nz %d (%d chunks, %s)" % (
            heavy, per, nz, n, piece_kind(rule, min(per, nz) * 4 * outX * outY)))
    plan.close()


@pytest.mark.parametrize("heavy,per", [("both", 2), ("output", 5)], ids=["both-2", "output-5"])
def test_nothing_is_read_or_written_past_the_arrays(fa, ring, rule, heavy, per):
    """the last piece of the last chunk is short: the caller's arrays lie inside larger buffers, a piece of slack behind each, and
    the slack behind the output keeps its bytes"""
    ring(SMALL)
    shape = SHAPES[(heavy, per)]
    inX, inY, outX, outY = shape
    nz = 3 * per + 1
    px, py, f, want = regrid_case(oracle.BILINEAR, shape, nz)
    last = layout.slice_chunks(rule, nz, per)[-1][1] * 4 * outX * outY
    assert 0 < layout.pieces(rule, last, PIECE)[-1][1] < PIECE
    slack = PIECE // 4
    buf_in = np.full(f.size + slack, 3.0, np.float32)
    buf_in[:f.size] = f.ravel()
    buf_out = np.full(want.size + slack, -7.0, np.float32)
    plan = fa.RegridPlan(oracle.BILINEAR, px, py, inX, inY, outX, outY)
    n = ctypes.c_size_t(0)
    fa._check(fa.load().fimex_amd_regrid_apply_host(plan._h, fa._fp(buf_in), f.size, fa._fp(buf_out), want.size, ctypes.byref(n)))
    assert n.value == want.size
    assert np.all(buf_out[want.size:] == -7.0), "%d cells behind the output were written" % np.count_nonzero(buf_out[want.size:] != -7.0)
    assert np.all(buf_in[f.size:] == 3.0)
    _identical(buf_out[:want.size].reshape(want.shape), want, "apply_host inside larger buffers, %s-%d" % (heavy, per))
    plan.close()


# ---------------------------------------------------------------------------------------- 3. stored types: regrid_slice_typed_host
# dtype, fill value, float scratch of the ring, shape, the limit that binds: one-byte cells are four times as large in the float
# scratch as in the pinned slot, so the scratch binds; for shorts a scratch of 1 MiB leaves the pinned slot binding
TYPED = {
    "int8-in": (np.int8, -128.0, SCRATCH, (250, 200, 60, 50), layout.FLOAT_IN),
    "int8-out": (np.int8, -128.0, SCRATCH, (60, 50, 250, 200), layout.FLOAT_OUT),
    "int16-in": (np.int16, -32768.0, 2 * SCRATCH, (250, 200, 60, 50), layout.PIN_IN),
    "int16-out": (np.int16, -32768.0, 2 * SCRATCH, (60, 50, 250, 200), layout.PIN_OUT),
}


def typed_case(dtype, fill, method, shape, nz):
    inX, inY, outX, outY = shape
    info = np.iinfo(dtype)
    rng = np.random.default_rng(inX + nz)
    px, py = cases.backward_positions(inX, inY, outX, outY, seed=3)
    a = rng.integers(info.min + 1, info.max, (nz, inY, inX), dtype=np.int64).astype(dtype)
    a[rng.random(a.shape) < 0.05] = dtype(fill)
    a[:, 0, 0] = dtype(fill)
    a[:, -1, -1] = dtype(fill)
    want = oracle.interpolation_array2data(
        oracle.interpolate_values(method, px, py, oracle.data2interpolation_array(a, fill), inX, inY, outX, outY, nthreads=8),
        oracle.cdm_type_of(dtype), fill)
    return px, py, a, want


@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("name", list(TYPED))
def test_stored_types_on_the_shrunk_ring(fa, ring, rule, name, method):
    import torch
    dtype, fill, scratch, shape, limit = TYPED[name]
    sizes = (SLOT, PIECE, scratch, LEAST)
    ring(sizes)
    inX, inY, outX, outY = shape
    elem = np.dtype(dtype).itemsize
    per, each, binding = layout.slices_per_chunk(rule, sizes, elem * inX * inY, elem * outX * outY, inX * inY, outX * outY)
    assert binding == limit and all(each[k] > each[limit] for k in range(4) if k != limit), (name, layout.LIMITS[binding], each)
    assert per == 2, (name, each)
    px, py, a_all, want_all = typed_case(dtype, fill, method, shape, 7 * per + 1)
    plan = fa.RegridPlan(method, px, py, inX, inY, outX, outY)
    for nz in nz_set(per):
        a, want = a_all[:nz], want_all[:nz]
        label = "regrid_slice_typed_host %s, nz %d" % (name, nz)
        copy = a.copy()
        got = fa.regrid_slice_typed_host(plan, a, fill)
        _unchanged((a,), (copy,), label)
        assert np.count_nonzero(want == dtype(fill)) > 0
        _identical(got, want.reshape(got.shape), label + ", oracle")
        d_in, d_out = _dev(a), torch.zeros(got.shape, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
        fa.regrid_apply_typed_device(plan, d_in.data_ptr(), fa.cdm_type_of(dtype), nz, fill, d_out.data_ptr(), _stream())
        _identical(got, _host(d_out), label + ", device twin")
    plan.close()


# ------------------------------------------------------------------------------------------------ 4. copy threads, the pipe off
# pieces of 1 MiB + 4100 bytes take the copier's threaded path (1 MiB and more) at a length no multiple of 4096 x parts
THREADED = (4 * 1024 * 1024 + 8, 1024 * 1024 + 4100, 8 * 1024 * 1024, 1024 * 1024)


@pytest.mark.parametrize("threads", [1, 2, 8])
def test_copy_threads(fa, ring, rule, threads):
    ring(THREADED, HOST_COPY_THREADS=threads)
    slot = THREADED[0]
    n = 3 * (slot // 4) + 1031
    assert len(layout.byte_chunks(rule, THREADED, 4 * n)) == 4
    check_overlay(fa, n, slot // 4, "overlay_host, %d copy threads" % threads)
    shape = (40, 30, 700, 500)  # 1 400 000 bytes a slice: two per chunk, pieces of 1 MiB + 4100 and a tail
    inX, inY, outX, outY = shape
    assert layout.slices_per_chunk(rule, THREADED, 4 * inX * inY, 4 * outX * outY, 0, 0)[0] == 2
    assert [length for _, length in layout.pieces(rule, 2 * 4 * outX * outY, THREADED[1])] == [THREADED[1]] * 2 + [2800000 - 2 * THREADED[1]]
    px, py, f, want = regrid_case(oracle.NEAREST, shape, 7)
    plan = fa.RegridPlan(oracle.NEAREST, px, py, inX, inY, outX, outY)
    check_apply_host(fa, plan, f, want, "apply_host, %d copy threads, 4 chunks" % threads, twin=False)
    plan.close()


def test_the_pipe_switched_off(fa, ring, rule):
    """HOST_PIPE=0: plain copies and the whole-array path give the same bits as the ring"""
    shape = SHAPES[("both", 2)]
    inX, inY, outX, outY = shape
    px, py, f, want = regrid_case(oracle.BILINEAR, shape, 7)
    for pipe in (1, 0):
        ring(SMALL, HOST_PIPE=pipe)
        plan = fa.RegridPlan(oracle.BILINEAR, px, py, inX, inY, outX, outY)
        check_apply_host(fa, plan, f, want, "apply_host, HOST_PIPE=%d" % pipe, twin=False)
        check_overlay(fa, PLAIN["7slots+odd"], F, "overlay_host, HOST_PIPE=%d" % pipe)
        plan.close()


@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR], ids=["nearest", "bilinear"])
def test_a_slice_one_element_larger_than_a_slot(fa, ring, rule, method):
    """pipelined_slices declines, the plain path (host_to_device of the whole array, in chunks of a slot) gives the same bits; with
    a slot of exactly one slice the ring takes it, one slice per chunk"""
    shape = SHAPES[("input", 1)]
    inX, inY, outX, outY = shape
    px, py, f, want = regrid_case(method, shape, 4)
    for slot, fit in ((4 * inX * inY - 4, 0), (4 * inX * inY, 1)):
        sizes = (slot, -(-slot // 8), SCRATCH, LEAST)
        ring(sizes)
        assert not layout.refused(rule, sizes)
        assert layout.slices_per_chunk(rule, sizes, 4 * inX * inY, 4 * outX * outY, 0, 0)[0] == fit
        plan = fa.RegridPlan(method, px, py, inX, inY, outX, outY)
        check_apply_host(fa, plan, f, want, "apply_host, slot of %d bytes, slice of %d" % (slot, 4 * inX * inY))
        plan.close()


# ------------------------------------------------------------------------------------------------- 5. two callers, cache release
def test_two_callers_mid_ring(fa, ring, rule):
    """two threads in apply_host at once, each eight chunks through its own ring of three slots"""
    ring(SMALL)
    shape = SHAPES[("both", 2)]
    inX, inY, outX, outY = shape
    nz = 15
    assert len(layout.slice_chunks(rule, nz, 2)) == 8
    px, py, f0, want0 = regrid_case(oracle.BILINEAR, shape, nz)
    f1 = np.ascontiguousarray(f0[::-1]) * np.float32(0.5)  # halving is exact: another field, its own oracle run
    want1 = oracle.interpolate_values(oracle.BILINEAR, px, py, f1, inX, inY, outX, outY, nthreads=8)
    plan = fa.RegridPlan(oracle.BILINEAR, px, py, inX, inY, outX, outY)
    fields, wants, results, failures = (f0, f1), (want0, want1), [[], []], []
    start = threading.Barrier(2)

    def work(i):
        try:
            start.wait()
            for _ in range(3):
                results[i].append(plan.apply_host(fields[i]))
        except BaseException as e:  # noqa: B902 - handed to the main thread
            failures.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    if failures:
        raise failures[0]
    for i in range(2):
        assert len(results[i]) == 3
        for k, got in enumerate(results[i]):
            _identical(got, wants[i], "caller %d, call %d" % (i, k))
    plan.close()


def test_release_caches_between_two_calls(fa, ring, rule):
    ring(SMALL)
    shape = SHAPES[("output", 2)]
    inX, inY, outX, outY = shape
    px, py, f, want = regrid_case(oracle.NEAREST, shape, 15)
    plan = fa.RegridPlan(oracle.NEAREST, px, py, inX, inY, outX, outY)
    check_apply_host(fa, plan, f, want, "apply_host before release_caches", twin=False)
    check_overlay(fa, PLAIN["3slots+1"], F, "overlay_host before release_caches")
    fa.release_caches()
    check_apply_host(fa, plan, f, want, "apply_host after release_caches", twin=False)
    check_overlay(fa, PLAIN["3slots+1"], F, "overlay_host after release_caches")
    plan.close()


# --------------------------------------------------------------------------------- 6. the product build's ring, 64 MiB slots
def timed(label, t0):
    print("%s: %.2f s" % (label, time.perf_counter() - t0))


def test_plain_copies_at_the_production_sizes(fa, rule):
    """3 x 64 MiB + 4 KiB + 4 bytes of float through overlay_host: the fourth chunk uses the first slot again, the last chunk is
    short in both directions and the length is no multiple of 4096.  Measured: see the pull request that added it (about 3 s)."""
    t0 = time.perf_counter()
    sizes = layout.production_sizes(rule)
    n = (3 * sizes[0] + 4096 + 4) // 4
    chunks = layout.byte_chunks(rule, sizes, 4 * n)
    assert len(chunks) == 4 and chunks[3] == (3 * sizes[0], 4100) and (4 * n) % 4096 != 0
    fa.use_tuning_build(False)
    check_overlay(fa, n, sizes[0] // 4, "overlay_host, 3 x 64 MiB + 4100 bytes")
    fa.release_caches()
    timed("overlay_host at the production sizes", t0)


def big_target():
    """a 64 x 48 source on a 4096 x 2050 target, positions by arithmetic: a shear, a rim of cells outside the source"""
    inX, inY, outX, outY = 64, 48, 4096, 2050
    j, i = np.divmod(np.arange(outX * outY, dtype=np.int64), outX)
    px = (i * 67 + j * 3) % 4500 / 4500.0 * (inX + 3) - 2.0
    py = (j * 53 + i) % 2300 / 2300.0 * (inY + 3) - 2.0
    return inX, inY, outX, outY, px, py


def oracle_indices(px, py, inX, inY, outX, outY):
    """the source cell of every target cell as the oracle's nearest neighbour picks it (-1: outside): the oracle regrids one slice
    that holds each cell's own index"""
    own = np.arange(inX * inY, dtype=np.float32).reshape(1, inY, inX)
    idx = oracle.interpolate_values(oracle.NEAREST, px, py, own, inX, inY, outX, outY, nthreads=16).ravel()
    return np.where(np.isnan(idx), -1, idx).astype(np.int64)


def test_slices_at_the_production_sizes(fa, rule):
    """apply_host, nearest, 5 slices of 33 587 200 bytes out: one slice per chunk, five chunks through three slots, four whole
    pieces and a tail of 32 768 bytes per chunk; every slice against a numpy gather of the oracle's own indices.  Measured: see
    the pull request that added it (about 3 s)."""
    t0 = time.perf_counter()
    inX, inY, outX, outY, px, py = big_target()
    sizes, nz = layout.production_sizes(rule), 5
    per, each, binding = layout.slices_per_chunk(rule, sizes, 4 * inX * inY, 4 * outX * outY, 0, 0)
    assert per == 1 and binding == layout.PIN_OUT and len(layout.slice_chunks(rule, nz, per)) == 5
    assert [length for _, length in layout.pieces(rule, 4 * outX * outY, sizes[1])] == [sizes[1]] * 4 + [32768]
    idx = oracle_indices(px, py, inX, inY, outX, outY)
    assert 0 < np.count_nonzero(idx < 0) < idx.size // 4
    f = pattern(nz * inY * inX, 5).reshape(nz, inY * inX).copy()
    f[:, 7] = np.nan
    want = np.where(idx < 0, np.float32(np.nan), f[:, np.maximum(idx, 0)]).reshape(nz, outY, outX)
    fa.use_tuning_build(False)
    plan = fa.RegridPlan(oracle.NEAREST, px, py, inX, inY, outX, outY)
    copy = f.copy()
    got = plan.apply_host(f)
    _unchanged((f,), (copy,), "apply_host at the production sizes")
    _identical(got, want, "apply_host at the production sizes, gather of the oracle's indices")
    plan.close()
    fa.release_caches()
    timed("apply_host at the production sizes", t0)


def test_stored_types_at_the_production_sizes(fa, rule):
    """The same target on int8 with fill values through regrid_slice_typed_host: the float scratch binds (three slices of
    8 396 800 cells per chunk, the pinned slot would take seven), so ten slices make the four chunks that use a slot again.  Against
    the oracle's data2interpolation_array, interpolate_values, interpolation_array2data.  Measured: see the pull request that added
    it (about 4 s)."""
    t0 = time.perf_counter()
    inX, inY, outX, outY, px, py = big_target()
    sizes, nz, fill = layout.production_sizes(rule), 10, -128.0
    per, each, binding = layout.slices_per_chunk(rule, sizes, inX * inY, outX * outY, inX * inY, outX * outY)
    assert per == 3 and binding == layout.FLOAT_OUT and each[layout.PIN_OUT] == 7
    assert layout.slice_chunks(rule, nz, per) == [(0, 3), (3, 3), (6, 3), (9, 1)]
    a = ((np.arange(nz * inY * inX, dtype=np.int64) * 37 + 11) % 255 - 127).astype(np.int8).reshape(nz, inY, inX)
    a[:, ::5, ::7] = np.int8(fill)
    want = oracle.interpolation_array2data(
        oracle.interpolate_values(oracle.NEAREST, px, py, oracle.data2interpolation_array(a, fill), inX, inY, outX, outY, nthreads=16),
        oracle.CDM_CHAR, fill)
    fa.use_tuning_build(False)
    plan = fa.RegridPlan(oracle.NEAREST, px, py, inX, inY, outX, outY)
    copy = a.copy()
    got = fa.regrid_slice_typed_host(plan, a, fill)
    _unchanged((a,), (copy,), "regrid_slice_typed_host at the production sizes")
    assert 0 < np.count_nonzero(want == np.int8(fill)) < want.size
    _identical(got, want.reshape(got.shape), "regrid_slice_typed_host at the production sizes, oracle")
    plan.close()
    fa.release_caches()
    timed("regrid_slice_typed_host at the production sizes", t0)
