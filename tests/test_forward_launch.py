"""Which kernel a forward apply launches and how it cuts the batch (fimex_amd/csrc/forward_launch.hpp) is plain arithmetic: compiled
here on its own with g++ (tests/forward_launch_host.py) and held to a Python restatement of the rule as forward.hip's comments give it,
and to what a launch needs whatever the rule: equal chunks that cover the batch once, a chunk count gridDim.y can hold, a lane grid
that is a multiple of the XCD count.  The inputs of tests/test_gpu_forward_z_chunks.py are checked here too, before any GPU run: every
mapping has the bucket figures its case relies on, gets the kernel, the z chunks and the passes per chunk the case is named after,
and its whole slices of NaN, +0.0, -0.0 and +inf lie at every position of a chunk."""
import itertools

import numpy as np
import pytest

import forward_launch_host as flh
import forward_z_cases as fz

SUM, MEAN, MEDIAN, MAX, MIN = range(5)


def _ceil_div(a, b):
    return -(-a // b)


def _restated(nOut, nz, mapped, empty, maxBucket, aggregate, tilesValid, knobs):
    """-> (family, zc, ahead, rank, zPerBlock, chunks, laneGridX)"""
    k = lambda name, default: knobs[name] if knobs.get(name, -1) >= 0 else default
    # z chunks of 16 slices, of 64 where the target grid alone has 4096 workgroups of 256 cells; then chunks of one size
    blocks = _ceil_div(nOut, 256)
    zpb = min(k("FWD_ZPB", 0) or (64 if blocks >= 4096 else 16), nz)
    chunks = _ceil_div(nz, zpb)
    zpb = _ceil_div(nz, chunks)
    chunks = _ceil_div(nz, zpb)
    grid = _ceil_div(blocks, 8) * 8
    mean = mapped / (nOut - empty) if nOut > empty else 0.0
    few = 1 if nz == 1 else 2 if nz <= 2 else 4 if nz <= 4 else 8  # slices per pass where the reference's one slice per call is likely
    if aggregate != MEDIAN:
        if tilesValid and k("FWD_TILED", 1) != 0:
            return flh.TILED, 1, 1, False, zpb, chunks, grid
        # long buckets are reduced by a whole wave, but only where the targets are too few to fill the chip with lanes
        wave = knobs["FWD_WAVE"] != 0 if knobs.get("FWD_WAVE", -1) >= 0 else (mean >= 32.0 and nOut * chunks < 65536)
        if wave:
            return flh.WAVE, 1, 1, False, zpb, chunks, grid
        if mean > 4.0:  # eight cells of look-ahead
            return flh.LANE, 8, 8, False, zpb, chunks, grid
        return flh.LANE, few, 1, False, zpb, chunks, grid
    rank_all = k("FWD_MEDIAN_SHORT", 1) == 0
    if maxBucket <= 1 and not rank_all:  # the median of one value is what the max kernel returns for it
        return flh.MEDIAN_AS_MAX, few, 1, False, zpb, chunks, grid
    if not rank_all and 2 < maxBucket <= 256 and mean >= k("FWD_MEDIAN_WAVE_MIN", 12) and k("FWD_MEDIAN_WAVE", 1) != 0:
        return flh.MEDIAN_WAVE, 1, 1, False, zpb, chunks, grid  # one wave per target from a mean length of twelve
    rank = maxBucket > 2 or rank_all
    return flh.LANE, 4 if not rank and k("FWD_MEDIAN_ZC", 8) == 4 else 8, 1, rank, zpb, chunks, grid


N_OUT = [1, 257, 3000, 65535, 4096 * 256 - 256, 4096 * 256 - 255, 4100 * 256]  # 4095 and 4096 workgroups among them
MEANS = [0.0, 1.0, 2.4, 2.5, 2.6, 3.9, 4.0, 4.1, 11.9, 12.0, 12.1, 31.9, 32.0, 32.1]
MAX_BUCKETS = [1, 2, 3, 255, 256, 257]
ZPB_KNOBS = [{}, {"FWD_ZPB": 1}, {"FWD_ZPB": 3}, {"FWD_ZPB": 24}, {"FWD_ZPB": 64}, {"FWD_ZPB": 300}, {"FWD_TILED": 0, "FWD_WAVE": 1, "FWD_ZPB": 5}]
KNOBS = ZPB_KNOBS + [{"FWD_WAVE": 0}, {"FWD_WAVE": 1}, {"FWD_MEDIAN_ZC": 4}, {"FWD_MEDIAN_ZC": 8}, {"FWD_MEDIAN_WAVE_MIN": 1}, {"FWD_MEDIAN_WAVE_MIN": 33},
                     {"FWD_MEDIAN_WAVE": 0}, {"FWD_MEDIAN_SHORT": 0}, {"FWD_TILED": 0}]


def _plans(means, max_buckets):
    """(nOut, mappedSourceCells, undefinedCells, maxBucket) with a third of the targets empty, at these mean and longest bucket lengths"""
    for nOut, mean, maxBucket in itertools.product(N_OUT, means, max_buckets):
        empty = nOut // 3
        mapped = int(round(mean * (nOut - empty)))
        if mean == 0.0:
            empty, mapped = nOut, 0
        elif mapped < maxBucket or mapped > maxBucket * (nOut - empty):
            continue  # no such plan
        yield nOut, mapped, empty, maxBucket


def _check(nOut, mapped, empty, maxBucket, nz, aggregate, tiles, knobs):
    got = flh.forward_launch(nOut, nz, mapped, empty, maxBucket, aggregate, tiles, knobs)
    want = _restated(nOut, nz, mapped, empty, maxBucket, aggregate, tiles, knobs)
    assert (got.family, got.zc, got.ahead, got.rank, got.zPerBlock, got.chunks, got.laneGridX) == want, (
        (nOut, nz, mapped, empty, maxBucket, aggregate, tiles, knobs), got)
    assert got.chunksFit and 1 <= got.chunks <= 65535
    assert got.chunks * got.zPerBlock >= nz > (got.chunks - 1) * got.zPerBlock  # every slice once, no empty chunk
    lengths = flh.chunk_lengths(got, nz)
    assert sum(lengths) == nz and set(lengths[:-1]) <= {got.zPerBlock} and 1 <= lengths[-1] <= got.zPerBlock  # chunks of one size
    assert got.laneGridX % 8 == 0 and 0 <= got.laneGridX * 256 - nOut < 8 * 256
    assert got.rankAll == (knobs.get("FWD_MEDIAN_SHORT") == 0)
    return got.family


def test_the_kernel_family_follows_the_restated_rule():
    """every threshold of the rule from both sides, at the batch lengths at which the slices per pass change and beyond one chunk"""
    flh.load()
    families = set()
    for plan, aggregate, knobs, nz, tiles in itertools.product(_plans(MEANS, MAX_BUCKETS), (MEAN, MEDIAN), KNOBS, (1, 2, 3, 4, 5, 17, 65, 200),
                                                              (False, True)):
        families.add(_check(*plan, nz, aggregate, tiles, knobs))
    assert families == {flh.TILED, flh.LANE, flh.WAVE, flh.MEDIAN_WAVE, flh.MEDIAN_AS_MAX}


def test_the_z_chunks_are_equal_and_cover_the_batch_once():
    """nz 1 .. 200 on either side of 4096 workgroups, with forced chunk lengths, short and long buckets (the wave rule counts
    targets times chunks) and every aggregate"""
    for plan, aggregate, knobs, nz in itertools.product(_plans([1.0, 40.0], [1, 64]), (SUM, MEAN, MEDIAN, MAX, MIN), ZPB_KNOBS, range(1, 201)):
        _check(*plan, nz, aggregate, False, knobs)


def test_the_chunk_sizes_of_the_launch_rule():
    """16 slices per chunk, 64 from 4096 workgroups of 256 targets, and the largest batch a launch holds"""
    small, large = 4096 * 256 - 256, 4096 * 256 - 255
    for nz in range(1, 201):
        assert flh.forward_launch(small, nz, small, 0, 1, MEAN, False).chunks == _ceil_div(nz, 16)
        assert flh.forward_launch(large, nz, large, 0, 1, MEAN, False).chunks == _ceil_div(nz, 64)
    assert flh.forward_launch(3000, 16 * 65535, 3000, 0, 1, MEAN, False).chunksFit
    assert not flh.forward_launch(3000, 16 * 65535 + 1, 3000, 0, 1, MEAN, False).chunksFit
    assert flh.forward_launch(3000, 0xFFFFFFFF, 3000, 0, 1, MEAN, False, {"FWD_ZPB": 70000}).chunks == 61357  # 64-bit arithmetic throughout


CASE_RUNS = [pytest.param(c, r, id="%s-nz%d%s" % (c.name, r.nz, "".join("-%s%d" % kv for kv in sorted(r.knobs.items()))))
             for c in fz.CASES + [fz.BIG] for r in c.runs]


@pytest.mark.parametrize("case", fz.CASES + [fz.BIG], ids=lambda c: c.name)
def test_forward_z_chunk_inputs_hold_what_their_cases_rely_on(case):
    """bucket counts by the oracle's own rounding (oracle.round_and_clamp on both coordinates of every source cell)"""
    _, _, outX, outY = case.geometry
    counts = fz.bucket_counts(*fz.positions(case.name), outX, outY)
    mean = counts.sum() / max(1, (counts > 0).sum())
    assert case.mean[0] < mean < case.mean[1], mean
    assert case.max_bucket[0] <= counts.max() and (case.max_bucket[1] is None or counts.max() <= case.max_bucket[1]), counts.max()
    assert (counts == 0).any() == case.empty
    fig = fz.figures(case.name)
    assert (fig["mappedSourceCells"], fig["undefinedCells"], fig["maxBucket"]) == (counts.sum(), (counts == 0).sum(), counts.max())
    if case.name == "lane":
        assert mean < 2.5  # not tiled on the product build
    if case.name == "lane_ahead":
        assert 8 < counts.max() < 16 and (counts >= 8).mean() > 0.25  # one round of eight cells ahead and a remainder, in many buckets
    if case.name == "median_rank":
        assert (counts > 2).sum() > 100 and ((counts > 0) & (counts <= 2)).sum() > 100  # both paths of the RANK kernel, side by side
    if case.name.startswith("median_two"):
        assert (counts == 2).sum() > 100 and (counts == 1).sum() > 100 and counts.size > 4 * 256
    if case.name == "wave":
        assert 128 < counts.max() <= 192 and (counts == 0).sum() == 856 and counts.size == 1200  # three rounds of 64 lanes
    if case.name == "zpb64":
        assert _ceil_div(counts.size, 256) == 4100  # at least 4096 workgroups


@pytest.mark.parametrize("case,run", CASE_RUNS)
def test_forward_z_chunk_cases_get_the_launch_they_are_named_after(case, run):
    for method in fz.methods_of(case, run.nz):
        l = fz.expected_launch(case.name, method, run)
        assert l.family == fz.family_of(case, method), flh.FAMILY_NAMES[l.family]
        assert (l.zc, l.ahead, l.rank, l.rankAll) == (case.zc, case.ahead, case.rank, False)
        assert flh.chunk_lengths(l, run.nz) == run.chunks and l.chunks == len(run.chunks)
        assert flh.chunk_passes(l, run.nz) == run.passes
    f, placed = fz.field(case.name, run.nz, l.zc, l.zPerBlock)
    assert fz.positions_needed(run, l.zc) <= {what for what, _ in placed.values()}
    values = [v for _, v in placed.values()]
    assert sum(np.isnan(v) for v in values) >= 1 and np.inf in values
    assert any(v == 0 and not np.signbit(v) for v in values) and any(v == 0 and np.signbit(v) for v in values)
    for z, (what, v) in placed.items():
        assert np.array_equal(f[z].view(np.uint32), np.full(f[z].shape, v, np.float32).view(np.uint32)), (z, what)
        c, k = divmod(z, l.zPerBlock)
        n = flh.chunk_lengths(l, run.nz)[c]
        if what == fz.FIRST:
            assert c > 0 and k == 0
        if what == fz.FULL:
            assert k % l.zc == l.zc - 1
        if what == fz.SHORT:
            assert k >= n - n % l.zc and n % l.zc
    others = [z for z in range(run.nz) if z not in placed]
    assert len({f[z].tobytes() for z in others}) == len(others) >= 2  # the slices differ from each other
