"""The cases of tests/test_gpu_forward_z_chunks.py: small forward mappings, the bucket figures each one relies on (computed on the CPU
with the oracle's own rounding), the launch each (case, nz) is meant to get from fimex_amd/csrc/forward_launch.hpp, and inputs with
whole slices of NaN, +0.0, -0.0 and +inf at the positions of a z chunk at which a slice index can go wrong.
tests/test_forward_launch.py checks all of it without a GPU."""
import collections
import functools

import numpy as np

import cases
import forward_launch_host as flh
import oracle

SEED = 11

Case = collections.namedtuple("Case", "name geometry density special knobs methods mean max_bucket empty family zc ahead rank runs")
# runs: (extra knobs, nz, slices per chunk, (full passes, slices of the short last pass) per chunk)
Run = collections.namedtuple("Run", "knobs nz chunks passes")

NON_MEDIAN = [oracle.FWD_SUM, oracle.FWD_MEAN, oracle.FWD_MAX, oracle.FWD_MIN, oracle.FWD_UNDEF_SUM, oracle.FWD_UNDEF_MEAN, oracle.FWD_UNDEF_MAX,
              oracle.FWD_UNDEF_MIN]
MEDIANS = [oracle.FWD_MEDIAN, oracle.FWD_UNDEF_MEDIAN]
FEW = [oracle.FWD_MEAN, oracle.FWD_UNDEF_SUM, oracle.FWD_UNDEF_MIN]

# what 16 slices per chunk make of nz (lane kernels, eight slices per pass)
NZ17 = Run({}, 17, [9, 8], [(1, 1), (1, 0)])
NZ35 = Run({}, 35, [12, 12, 11], [(1, 4), (1, 4), (1, 3)])
NZ48 = Run({}, 48, [16, 16, 16], [(2, 0)] * 3)
NZ83 = Run({}, 83, [14] * 5 + [13], [(1, 6)] * 5 + [(1, 5)])
# one slice per pass
WAVE17 = Run({}, 17, [9, 8], [(9, 0), (8, 0)])
WAVE35 = Run({}, 35, [12, 12, 11], [(12, 0), (12, 0), (11, 0)])

SMALL = (140, 110, 60, 50)
# found by searching the small geometries of cases.forward_positions (seed 11) for a longest bucket of exactly two cells: 554 targets
# stay empty, 342 hold one cell, 325 hold two; 1221 targets are five workgroups of the lane kernel
TWO = (64, 20, 37, 33)
# mean: (low, high) the mean bucket length lies between; max_bucket: (low, high) inclusive, None for no bound; empty: the mapping must leave targets empty
CASES = [
    # mean 1.1: below 2.5, so no tiled form
    Case("lane", SMALL, 0.3, True, {}, {17: NON_MEDIAN, 35: FEW, 48: FEW, 83: FEW}, (0.0, 2.5), (1, None), True, flh.LANE, 8, 1, False,
         [NZ17, NZ35, NZ48, NZ83]),
    # mean 8, longest 10: eight cells of look-ahead and a remainder behind them
    Case("lane_ahead", SMALL, 3.0, False, {"FWD_TILED": 0}, [oracle.FWD_SUM, oracle.FWD_MEAN, oracle.FWD_UNDEF_MEAN, oracle.FWD_MAX, oracle.FWD_UNDEF_MIN],
         (4.0, 12.0), (9, 15), True, flh.LANE, 8, 8, False,
         [NZ17, NZ35, Run({"FWD_ZPB": 24}, 50, [17, 17, 16], [(2, 1), (2, 1), (2, 0)]), Run({"FWD_ZPB": 3}, 7, [3, 3, 1], [(0, 3), (0, 3), (0, 1)])]),
    # mean 2.8, longest 25: below 12, so not the wave median; buckets of three and more by rank, the others batched, in one launch
    Case("median_rank", SMALL, 1.0, True, {}, MEDIANS, (0.0, 12.0), (3, None), True, flh.LANE, 8, 1, True, [NZ17, NZ35]),
    Case("median_two", TWO, 1.5, False, {}, MEDIANS, (0.0, 2.5), (2, 2), True, flh.LANE, 8, 1, False, [NZ17, NZ35]),
    Case("median_two_zc4", TWO, 1.5, False, {"FWD_MEDIAN_ZC": 4}, MEDIANS, (0.0, 2.5), (2, 2), True, flh.LANE, 4, 1, False,
         [Run({}, 9, [9], [(2, 1)]), Run({}, 17, [9, 8], [(2, 1), (2, 0)])]),
    Case("median_single", (20, 16, 61, 50), 0.3, False, {}, MEDIANS, (0.0, 2.5), (1, 1), True, flh.MEDIAN_AS_MAX, 8, 1, False, [NZ17]),
    # mean about 140, longest about 170: three rounds of 64 lanes; 856 of 1200 targets empty (the per-chunk NaN stores)
    Case("wave", (240, 200, 40, 30), 7.0, False, {"FWD_TILED": 0, "FWD_WAVE": 1},
         [oracle.FWD_SUM, oracle.FWD_MEAN, oracle.FWD_MAX, oracle.FWD_MIN, oracle.FWD_UNDEF_MEAN, oracle.FWD_UNDEF_MAX],
         (32.0, 192.0), (129, 192), True, flh.WAVE, 1, 1, False, [WAVE17, WAVE35]),
]
# 4100 workgroups of 256 targets: chunks of 64 slices
BIG = Case("zpb64", (48, 40, 1024, 1025), 1.0, False, {}, [oracle.FWD_MEAN, oracle.FWD_MEDIAN], (0.0, 2.5), (1, 1), True, None, 8, 1, False,
           [Run({}, 64, [64], [(8, 0)]), Run({}, 65, [33, 32], [(4, 1), (4, 0)])])
BY_NAME = {c.name: c for c in CASES + [BIG]}


def methods_of(case, nz):
    return case.methods[nz] if isinstance(case.methods, dict) else case.methods


def family_of(case, method):
    if case.family is not None:
        return case.family
    return flh.MEDIAN_AS_MAX if method in MEDIANS else flh.LANE  # BIG: buckets of one cell


def knobs_of(case, run):
    k = dict(case.knobs)
    k.update(run.knobs)
    return k


@functools.lru_cache(maxsize=None)
def positions(name):
    inX, inY, outX, outY = BY_NAME[name].geometry
    px, py = cases.forward_positions(inX, inY, outX, outY, seed=SEED, density=BY_NAME[name].density, special=BY_NAME[name].special)
    px.setflags(write=False)
    py.setflags(write=False)
    return px, py


def bucket_counts(px, py, outX, outY):
    """source cells per target cell, by the oracle's own rounding (CachedForwardInterpolation.cc: both coordinates rounded and clamped,
    a cell with either one outside is dropped)"""
    counts = np.zeros(outX * outY, np.int64)
    for x, y in zip(px, py):
        tx, ty = oracle.round_and_clamp(x, 0, outX - 1), oracle.round_and_clamp(y, 0, outY - 1)
        if tx >= 0 and ty >= 0:
            counts[ty * outX + tx] += 1
    return counts


@functools.lru_cache(maxsize=None)
def figures(name):
    """what plan.info() must report for the case: mappedSourceCells, undefinedCells, maxBucket, outX, outY, and no tiled form"""
    _, _, outX, outY = BY_NAME[name].geometry
    counts = bucket_counts(*positions(name), outX, outY)
    return {"outX": outX, "outY": outY, "mappedSourceCells": int(counts.sum()), "undefinedCells": int((counts == 0).sum()),
            "maxBucket": int(counts.max()), "stagedCells": 0}


def expected_launch(name, method, run):
    """the launch forward_launch.hpp gives the case, from the CPU's bucket figures"""
    info = dict(figures(name), funcType=method)
    return flh.launch_of_plan(info, run.nz, knobs_of(BY_NAME[name], run))


WHOLE_SLICES = [np.nan, 0.0, -0.0, np.inf]
FIRST, FULL, SHORT = "first of a chunk", "last of a full pass", "in the short last pass"


def chunk_positions(launch, nz):
    """{slice: what it is} for the positions of a z chunk at which a wrong slice index shows: the first slice of a chunk behind the
    first, the last slice of a full pass, a slice (the last one) of a short last pass, and the batch's last slice.  Chunks behind the
    first are preferred; a slice stands for one position only."""
    lengths = flh.chunk_lengths(launch, nz)
    starts = [c * launch.zPerBlock for c in range(len(lengths))]
    order = list(range(1, len(lengths))) + [0]
    want = [(FIRST, [starts[c] for c in order if c > 0])]
    if launch.zc > 1:
        want.append((FULL, [starts[c] + lengths[c] // launch.zc * launch.zc - 1 for c in order if lengths[c] >= launch.zc]))  # of the last one
        want.append((SHORT, [starts[c] + lengths[c] - 1 for c in order if lengths[c] % launch.zc]))
    want.append(("last of the batch", [nz - 1]))
    want.append(("first of the batch", [0]))
    want.append(("elsewhere", list(range(1, nz - 1))))
    taken = {}
    while len(taken) < len(WHOLE_SLICES) and any(zs for _, zs in want):  # one slice per position, then second ones
        for what, zs in want:
            while zs:
                z = zs.pop(0)
                if z not in taken:
                    taken[z] = what
                    break
    return taken


def positions_needed(run, zc):
    """the positions that the chunks of a run have"""
    need = set()
    if len(run.chunks) > 1:
        need.add(FIRST)
    if zc > 1 and any(full for full, _ in run.passes):
        need.add(FULL)
    if zc > 1 and any(short for _, short in run.passes):
        need.add(SHORT)
    return need


@functools.lru_cache(maxsize=None)
def field(name, nz, zc, z_per_block):
    """cases.field with whole slices of NaN, +0.0, -0.0 and +inf at chunk_positions; -> (field, {slice: (position, value)})"""
    inX, inY, _, _ = BY_NAME[name].geometry
    Cut = collections.namedtuple("Cut", "zc zPerBlock chunks")
    where = chunk_positions(Cut(zc, z_per_block, -(-nz // z_per_block)), nz)
    f = cases.field(nz, inY, inX, seed=400 + nz, nan_frac=0.04)
    assert len(where) >= len(WHOLE_SLICES) and nz - len(where) >= 2  # every whole-slice value, and ordinary slices next to them
    placed = {}
    for k, z in enumerate(sorted(where)):
        f[z] = np.float32(WHOLE_SLICES[k % 4])
        placed[z] = (where[z], WHOLE_SLICES[k % 4])
    f.setflags(write=False)
    return f, placed


@functools.lru_cache(maxsize=8)
def want(name, method, nz, zc, z_per_block):
    px, py = positions(name)
    inX, inY, outX, outY = BY_NAME[name].geometry
    w = oracle.forward_interpolate_values(method, px, py, field(name, nz, zc, z_per_block)[0], inX, inY, outX, outY)
    w.setflags(write=False)
    return w
