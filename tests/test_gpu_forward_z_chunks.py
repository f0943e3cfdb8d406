"""The slice loops of the forward lane and wave kernels (csrc/forward.hip, wave_target of csrc/forward.hpp) against the CPU oracle.

launch_forward_apply cuts a batch into z chunks of 16 slices (64 where the target has 4096 workgroups of 256 cells), the lane kernels
walk a chunk ZC slices at a time with a short last pass whose slice offsets are clamped and whose stores are guarded, and the wave
kernel walks it slice by slice.  At the batch lengths of the other modules (at most 9 slices) all of that runs in one chunk with at
most one full pass.  Here every kernel runs in a second chunk and beyond, with several full passes and with short last passes of
every kind.  Each test asks csrc/forward_launch.hpp -- the function the library itself calls -- with the figures of plan.info() which
kernel, how many chunks and how many passes per chunk the call takes, and asserts the ones its case is named after: a retuned
launcher must fail here, not turn the cases back into one-chunk tests.

Chunks as (full passes + slices of the short last pass), by case (tests/forward_z_cases.py; the same table is checked on the CPU by
tests/test_forward_launch.py):
  lane<A, U, 8>                 nz 17: 1 + 1, 1; 35: 1 + 4, 1 + 4, 1 + 3; 48: 2, 2, 2; 83: 5 x (1 + 6), 1 + 5
  lane<A, U, 8, false, 8>       nz 17, 35 as above; FWD_ZPB 24, nz 50: 2 + 1, 2 + 1, 2; FWD_ZPB 3, nz 7: 0 + 3, 0 + 3, 0 + 1
  lane<Median, U, 8, true>      nz 17, 35: buckets of three cells and more slice by slice, the others batched, in one launch
  lane<Median, U, 8>            nz 17, 35 (no bucket of more than two cells)
  lane<Median, U, 4>            FWD_MEDIAN_ZC 4, nz 9: 2 + 1 in one chunk; 17: 2 + 1, 2
  lane<Max, U, 8> as the median nz 17 (single cells)
  wave<A, U>                    nz 17: 9, 8 slices; 35: 12, 12, 11; buckets of three rounds of 64 lanes, 856 of 1200 targets empty
  lane<Mean | Max, false, 8>    the 64-slice rule at 4100 workgroups: nz 64: 8 passes in one chunk; 65: 4 + 1, 4

Comparisons are bit for bit with identical NaN positions and equal sign bits.  The inputs are cases.field (slices that differ from each
other) with whole slices of NaN, +0.0, -0.0 and +inf at the first slice of a later chunk, the last slice of a full pass and inside a
short last pass.  The output lies inside a larger device allocation: the sentinels around it must survive and none may be left in it."""
import numpy as np
import pytest

import cases
import forward_launch_host as flh
import forward_z_cases as fz
import oracle

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.678)
PAD = 64  # floats of sentinel on either side of the output


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


def _apply_between_guards(plan, f, outY, outX):
    """apply_device into the middle of a sentinel-filled allocation -> the result on the host; checks the guards"""
    import torch
    nz, n = f.shape[0], f.shape[0] * outY * outX
    d_in = torch.from_numpy(np.array(f)).cuda()  # a copy: the shared inputs are read-only
    buf = torch.full((n + 2 * PAD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    plan.apply_device(d_in.data_ptr(), nz, buf.data_ptr() + 4 * PAD, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    del buf, d_in
    guards = np.concatenate([h[:PAD], h[PAD + n:]]).view(np.uint32)
    assert guards.size == 2 * PAD and np.all(guards == SENTINEL.view(np.uint32)), "the call wrote outside its output"
    return h[PAD:PAD + n].reshape(nz, outY, outX)


def _identical(got, want):
    assert not np.any(got.view(np.uint32) == SENTINEL.view(np.uint32)), "cells that no workgroup stored: %d, first (z, y, x) %s" % (
        np.count_nonzero(got.view(np.uint32) == SENTINEL.view(np.uint32)), np.argwhere(got.view(np.uint32) == SENTINEL.view(np.uint32))[:3].tolist())
    assert cases.same(got, want), cases.describe_mismatch(got, want)
    assert np.array_equal(np.signbit(got[~np.isnan(got)]), np.signbit(want[~np.isnan(want)]))


def _run_case(fa, monkeypatch, case, run, method):
    knobs = fz.knobs_of(case, run)
    for k, v in knobs.items():
        monkeypatch.setenv("FIMEX_AMD_" + k, str(v))
    inX, inY, outX, outY = case.geometry
    px, py = fz.positions(case.name)
    plan = fa.RegridPlan(method, px, py, inX, inY, outX, outY)
    info = plan.info()
    for k, v in fz.figures(case.name).items():  # the bucket figures the case relies on (the CPU test holds them to the oracle's rounding)
        assert info[k] == v, (k, info[k], v)
    assert case.max_bucket[0] <= info["maxBucket"] and (case.max_bucket[1] is None or info["maxBucket"] <= case.max_bucket[1]), info
    assert (info["undefinedCells"] > 0) == case.empty
    l = flh.launch_of_plan(info, run.nz, knobs)
    assert case.mean[0] < l.meanBucket < case.mean[1], l.meanBucket
    assert l.family == fz.family_of(case, method), flh.FAMILY_NAMES[l.family]
    assert (l.zc, l.ahead, l.rank, l.rankAll) == (case.zc, case.ahead, case.rank, False)
    assert l.chunks == len(run.chunks) and flh.chunk_lengths(l, run.nz) == run.chunks
    assert flh.chunk_passes(l, run.nz) == run.passes
    f, placed = fz.field(case.name, run.nz, l.zc, l.zPerBlock)
    assert fz.positions_needed(run, l.zc) <= {what for what, _ in placed.values()}
    return plan, f, l


def _params(names):
    return [pytest.param(c, r, m, id="%s-nz%d%s-%d" % (c.name, r.nz, "".join("-%s%d" % kv for kv in sorted(r.knobs.items())), m))
            for c in fz.CASES if c.name in names for r in c.runs for m in fz.methods_of(c, r.nz)]


@pytest.mark.parametrize("case,run,method", _params(["lane", "median_rank", "median_two", "median_single"]))
def test_forward_lane_kernels_beyond_one_chunk(fa, monkeypatch, case, run, method):
    """the product library under its own launch rule: forward_apply_lane<A, U, 8> on sparse buckets, the median by rank next to
    batched lanes, the median of at most two cells, and the median of single cells through the max kernel"""
    assert not case.knobs and not run.knobs
    plan, f, l = _run_case(fa, monkeypatch, case, run, method)
    _, _, outX, outY = case.geometry
    _identical(_apply_between_guards(plan, f, outY, outX), fz.want(case.name, method, run.nz, l.zc, l.zPerBlock))


@pytest.mark.parametrize("case,run,method", _params(["lane_ahead", "median_two_zc4", "wave"]))
def test_forward_kernels_behind_switches_beyond_one_chunk(fa, monkeypatch, case, run, method, tuning_build):
    """the tuning library: the lane kernels with eight cells of look-ahead (FWD_TILED=0, also with forced chunk lengths), the
    four-slice median kernel (FWD_MEDIAN_ZC=4) and forward_apply_wave (FWD_TILED=0, FWD_WAVE=1) with empty targets in every chunk"""
    plan, f, l = _run_case(fa, monkeypatch, case, run, method)
    _, _, outX, outY = case.geometry
    _identical(_apply_between_guards(plan, f, outY, outX), fz.want(case.name, method, run.nz, l.zc, l.zPerBlock))


@pytest.mark.parametrize("run", fz.BIG.runs, ids=lambda r: "nz%d" % r.nz)
@pytest.mark.parametrize("method", fz.BIG.methods, ids=["mean", "median"])
def test_forward_lane_kernels_under_the_64_slice_rule(fa, monkeypatch, run, method):
    """the product library at the smallest target at which its rule gives chunks of 64 slices (4100 workgroups): 64 slices in one
    chunk of eight passes, 65 in chunks of 33 and 32"""
    import torch
    case = fz.BIG
    plan, f, l = _run_case(fa, monkeypatch, case, run, method)
    assert l.zPerBlock == max(run.chunks) and l.laneGridX == 4104
    inX, inY, outX, outY = case.geometry
    want = oracle.forward_interpolate_values(method, *fz.positions(case.name), f, inX, inY, outX, outY)
    got = _apply_between_guards(plan, f, outY, outX)
    _identical(got, want)
    del got, want
    torch.cuda.empty_cache()
