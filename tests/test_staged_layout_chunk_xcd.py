"""The chunk-per-XCD launch order of the second staged form (fimex_amd/csrc/staged_layout.hpp: chunk_xcd_order, chunk_xcd_workgroup,
chunk_xcd_chunk_count, launch_order_of), compiled on its own with g++ (tests/staged_layout_chunk_xcd_host.cc) and checked on the CPU
for what no parity test shows: every (tile, z chunk) pair is one workgroup and no workgroup is anything else, workgroup s runs a chunk
congruent to s % 8 (the XCD it runs on owns that chunk), vertical neighbours of a cohort are close in the sequence every XCD walks,
batches too short for 8 chunks run exactly what they ran before, and the chunks partition the batch.

"Within 32 entries" counts entries of the table every XCD walks.  With 8 chunks an entry is one workgroup of the XCD; with 16 it is
two consecutive ones (chunks x and x + 8 of the tile)."""
import numpy as np
import pytest

import staged_layout_chunk_xcd_host as cx
from staged_layout_chunk_xcd_host import decode, order_of, z_chunks

XCDS = 8
CHUNK_MAJOR, TILE_MAJOR, CHUNK_PER_XCD = 0, 1, 2
COHORTS = [(8, 4), (16, 2), (32, 1)]


@pytest.fixture(scope="module")
def lib():
    return cx.load()


def ceil_div(a, b):
    return -(-a // b)


def chunk_count(nz, zpb):
    """the rule of chunk_xcd_chunk_count, stated a second time"""
    if ceil_div(nz, zpb) > 16:
        zpb = ceil_div(nz, 16)
    shortest = (zpb + 1) // 2
    if ceil_div(nz, zpb) > 8 and nz // 16 >= shortest:
        return 16
    return 8 if nz // 8 >= shortest else 0


def ragged_bands(rng, nBands, tileW):
    """Tiles as the tile cutting leaves them (refine_bands): every band is cut into tiles of its own width, a multiple of the step
    and at most tileW (the last tile narrower), and here and there a tile is split in two on a step boundary.  The target is one to
    four widest tiles wide and no band holds more than nine tiles."""
    step = 64 if tileW >= 128 else 32
    outX = int(rng.integers(1, 4 * tileW + 1))
    narrowest = min(tileW, max(step, ceil_div(ceil_div(outX, 9), step) * step))  # nine tiles at the most
    x0s, ws, bands = [], [], []
    for b in range(nBands):
        w = int(rng.integers(narrowest // step, tileW // step + 1)) * step
        row = [(x, min(w, outX - x)) for x in range(0, outX, w)]
        if len(row) < 9 and rng.random() < 0.3:  # one split tile
            k = int(rng.integers(0, len(row)))
            x, tw = row[k]
            if tw > step:
                lw = (tw // 2 + step - 1) // step * step
                row[k:k + 1] = [(x, lw), (x + lw, tw - lw)]
        assert 1 <= len(row) <= 9
        for x, tw in row:
            x0s.append(x); ws.append(tw); bands.append(b)
    return np.array(x0s), np.array(ws), np.array(bands), outX


def band_counts():
    """1 .. 70 bands, every count"""
    return list(range(1, 71))


@pytest.mark.parametrize("by,bx", COHORTS)
def test_every_tile_and_chunk_is_one_workgroup_on_its_chunks_xcd(lib, by, bx):
    rng = np.random.default_rng(by)
    for nBands in band_counts():
        x0, w, band, _ = ragged_bands(rng, nBands, 256)
        order, _ = order_of(lib, x0, w, band, 256, by, bx)
        nTiles = len(x0)
        assert np.array_equal(np.sort(order), np.arange(nTiles)), "a tile twice, or not at all"
        for n in (8, 16):
            grid = nTiles * n
            slot, zc = decode(lib, grid, n, 1)
            assert (slot < nTiles).all() and (zc < n).all(), "a workgroup beyond the table or the chunks"
            assert (zc % XCDS == np.arange(grid) % XCDS).all(), "a chunk on another XCD than its own"
            pairs = order[slot] * n + zc
            assert np.array_equal(np.sort(pairs), np.arange(nTiles * n)), "a (tile, chunk) pair twice, or not at all"
            # every XCD walks the table front to back, n / 8 chunks per entry
            for x in range(XCDS):
                mine = slot[x::XCDS]
                assert np.array_equal(mine, np.repeat(np.arange(nTiles), n // XCDS))


def check_cohort_rule(x0, w, band, tileW, by, bx, order, cohort):
    """the rule as staged_layout.hpp states it"""
    column = (x0 + w // 2) // tileW
    key = np.stack([band[order] // by, column[order] // bx, column[order], band[order], x0[order]], axis=1)
    assert all(tuple(a) < tuple(b) for a, b in zip(key, key[1:])), "not in (band group, column group, column, band, x0) order"
    assert cohort[0] == 0 and set(np.diff(cohort)) <= {0, 1}, "cohorts are not consecutive runs"
    for c in range(cohort[-1] + 1):
        mine = key[cohort == c]
        assert 1 <= len(mine) <= by * bx
        assert (mine[:, 0] == mine[0, 0]).all() and (mine[:, 1] == mine[0, 1]).all(), "a cohort over two band or column groups"
    # a cut inside a (band group, column group) only where the cohort before it is full
    for k in np.flatnonzero(np.diff(cohort)) + 1:
        if tuple(key[k, :2]) == tuple(key[k - 1, :2]):
            assert (cohort == cohort[k - 1]).sum() == by * bx


@pytest.mark.parametrize("by,bx", COHORTS)
@pytest.mark.parametrize("tileW", [64, 256, 512])
def test_vertical_neighbours_of_a_cohort_are_within_32_entries(lib, by, bx, tileW):
    rng = np.random.default_rng(tileW + by)
    pairs_seen = cut_seen = 0
    for nBands in band_counts():
        x0, w, band, _ = ragged_bands(rng, nBands, tileW)
        order, cohort = order_of(lib, x0, w, band, tileW, by, bx)
        check_cohort_rule(x0, w, band, tileW, by, bx, order, cohort)
        cut_seen += int((np.bincount(cohort) == by * bx).any())
        where = np.empty(len(order), np.int64)
        where[order] = np.arange(len(order))
        cohort_of_tile = cohort[where]
        for b in range(nBands - 1):
            for i in np.flatnonzero(band == b):
                below = np.flatnonzero((band == b + 1) & (x0 < x0[i] + w[i]) & (x0 + w > x0[i]))
                for j in below:
                    if cohort_of_tile[i] == cohort_of_tile[j]:
                        pairs_seen += 1
                        assert abs(where[i] - where[j]) < 32, (nBands, int(i), int(j))
    assert pairs_seen > 100 and cut_seen > 0


@pytest.mark.parametrize("by,bx", COHORTS)
def test_uniform_bands_run_y_fastest(lib, by, bx):
    """bands of four equal tiles, as most bands of the benchmark plan are: inside a cohort the bands of one column follow each
    other, so vertical neighbours are adjacent entries; the last band group is not full"""
    tileW, nBands, perBand = 512, 2 * by + 3, 4
    band = np.repeat(np.arange(nBands), perBand)
    x0 = np.tile(np.arange(perBand) * tileW, nBands)
    w = np.full(len(x0), tileW)
    w[x0 == (perBand - 1) * tileW] = 464  # a target of 2000 columns
    order, cohort = order_of(lib, x0, w, band, tileW, by, bx)
    want, want_cohort, c = [], [], 0
    for g in range(0, nBands, by):
        for cg in range(0, perBand, bx):
            for col in range(cg, min(cg + bx, perBand)):
                for b in range(g, min(g + by, nBands)):
                    want.append(b * perBand + col)
                    want_cohort.append(c)
            c += 1
    assert order.tolist() == want and cohort.tolist() == want_cohort


def test_fewer_bands_than_a_cohort(lib):
    """three bands under cohorts of 8, 16 and 32 bands: one band group, columns left to right, the bands of a column together"""
    band = np.repeat(np.arange(3), 2)
    x0, w = np.tile([0, 256], 3), np.full(6, 256)
    for by, bx in COHORTS:
        order, cohort = order_of(lib, x0, w, band, 256, by, bx)
        assert order.tolist() == [0, 2, 4, 1, 3, 5]
        assert cohort.tolist() == ([0] * 6 if bx > 1 else [0, 0, 0, 1, 1, 1])


def test_batches_too_short_for_8_chunks_keep_the_tile_major_launch_bit_for_bit(lib):
    fell_back = took = 0
    for zpb in (1, 2, 3, 5, 8, 13, 25, 40):
        for nz in range(1, 301):
            count = lib.scx_chunk_count(nz, zpb)
            assert count in (0, 8, 16)
            assert lib.scx_launch_order(CHUNK_PER_XCD, 0, nz, zpb) == TILE_MAJOR, "a launch that does not allow the order got it"
            assert lib.scx_launch_order(TILE_MAJOR, 1, nz, zpb) == TILE_MAJOR and lib.scx_launch_order(CHUNK_MAJOR, 1, nz, zpb) == CHUNK_MAJOR
            got = lib.scx_launch_order(CHUNK_PER_XCD, 1, nz, zpb)
            assert got == (CHUNK_PER_XCD if count else TILE_MAJOR)
            ok, zs, n = z_chunks(lib, nz, CHUNK_PER_XCD, zpb)
            ok1, zs1, n1 = z_chunks(lib, nz, TILE_MAJOR, zpb)
            assert ok and ok1
            if count:
                took += 1
                assert n == count
                continue
            fell_back += 1
            assert n == n1 and np.array_equal(zs, zs1), "other z chunks than the tile-major launch"
            # and the launch decodes its workgroups as before: mode 0 is flat_workgroup itself
            slot, zc = decode(lib, 16 * n, n, 0)
            k = np.arange(16 * n) // XCDS
            assert np.array_equal(zc, k % n) and np.array_equal(slot, k // n * XCDS + np.arange(16 * n) % XCDS)
    assert fell_back > 100 and took > 100


def test_z_chunks_of_the_order_cover_the_batch_once(lib):
    for zpb in (1, 2, 3, 5, 8, 13, 25, 40):
        shortest = (zpb + 1) // 2
        for nz in range(1, 301):
            ok, zs, n = z_chunks(lib, nz, CHUNK_PER_XCD, zpb)
            assert ok and 1 <= n <= 16
            assert zs[0] == 0 and zs[n] == nz
            size = np.diff(zs[:n + 1])
            assert (size > 0).all() and size.max() - size.min() <= 1, "not a partition into chunks of one size"
            assert lib.scx_chunk_count(nz, zpb) == chunk_count(nz, zpb)
            if chunk_count(nz, zpb):
                assert n == chunk_count(nz, zpb) and size.min() >= shortest, (zpb, nz, n)
                # 16 only where the tile-major split makes more than 8 chunks of the same batch
                assert n == 8 or z_chunks(lib, nz, TILE_MAJOR, zpb)[2] > 8
    # the product's chunk length: 8 chunks from 104 slices on, 16 from 208 on where 8 chunks of 25 no longer hold the batch
    assert [lib.scx_chunk_count(nz, 25) for nz in (103, 104, 200, 201, 207, 208, 400, 4096)] == [0, 8, 8, 8, 8, 16, 16, 16]
