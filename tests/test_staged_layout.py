"""The launch layout of the staged regrid forms (fimex_amd/csrc/staged_layout.hpp) is plain arithmetic: compiled here on its own with
g++ (tests/staged_layout_host.py) and checked for what a parity test on the GPU cannot show -- a tile that two workgroups compute
gives the right bits and costs time, a tile that none computes shows only if the output held something else before.  Every workgroup
decode is a bijection onto the tiles and z chunks of its grid, the workgroup -> tile table holds every tile once on the XCD the
stripe rule names, the tile cutting ends with bands that partition the target, and the z chunks partition the batch."""
import numpy as np
import pytest

import staged_layout_host as slh

XCDS = 8


@pytest.fixture(scope="module")
def lib():
    return slh.load()


def test_flat_grid_decodes_to_every_slot_and_z_chunk_once(lib):
    import ctypes
    slot, zc = ctypes.c_uint32(0), ctypes.c_uint32(0)
    for gridX in range(8, 65, 8):
        for n in range(1, 17):
            first = {}
            for b in range(gridX * n):
                lib.sl_flat_workgroup(b, n, ctypes.byref(slot), ctypes.byref(zc))
                s, c = slot.value, zc.value
                assert s < gridX and c < n and s % XCDS == b % XCDS
                assert (s, c) not in first, "two workgroups for one tile and z chunk"
                first[(s, c)] = b
            assert len(first) == gridX * n
            # the chunks of a slot are consecutive workgroups of its XCD (every eighth workgroup of the launch)
            assert all(first[(s, c)] == first[(s, 0)] + XCDS * c for s in range(gridX) for c in range(n))


def test_first_form_grid_reaches_every_tile_once(lib):
    for remap in (0, 1, 2, 3):
        for tilesX in range(1, 6):
            for nTiles in range(1, 61):
                grid = lib.sl_first_form_grid(nTiles, tilesX, remap)
                assert grid % XCDS == 0 and grid >= nTiles
                tiles = np.zeros(grid, np.uint32)
                lib.sl_first_form_tiles(grid, nTiles, tilesX, remap, tiles.ctypes.data)
                real = np.sort(tiles[tiles < nTiles])
                assert np.array_equal(real, np.arange(nTiles)), (remap, tilesX, nTiles)  # the other blocks yield a tile >= nTiles


def n_stripes(nBands, stripe):
    """stripes of about `stripe` bands, their number a multiple of the XCD count (at least one per XCD, at most one per band)"""
    n = (nBands + stripe * XCDS // 2) // (stripe * XCDS) * XCDS
    n = max(n, XCDS)
    if n > nBands:
        n = max(nBands // XCDS * XCDS, 1)
    return n


def test_xcd_order_holds_every_tile_once_on_its_stripes_xcd(lib):
    rng = np.random.default_rng(5)
    for nBands in range(1, 41):
        for stripe in (1, 2, 4, 8):
            per_band = rng.integers(1, 6, nBands)  # ragged bands
            band_of = np.repeat(np.arange(nBands), per_band)
            order = slh.xcd_order(lib, band_of, nBands, stripe)
            assert len(order) % XCDS == 0
            real = order[order != slh.NONE]
            assert np.array_equal(np.sort(real), np.arange(len(band_of))), "a tile twice, or not at all"
            table = order.reshape(-1, XCDS)
            assert (table[-1] != slh.NONE).any(), "a row of workgroups without tiles"
            for x in range(XCDS):
                col = table[:, x]
                k = int((col != slh.NONE).sum())
                assert (col[k:] == slh.NONE).all() and (np.diff(col[:k].astype(np.int64)) > 0).all()
                if nBands >= XCDS:
                    ns = n_stripes(nBands, stripe)
                    assert all((int(band_of[t]) * ns // nBands) % XCDS == x for t in col[:k])
                else:
                    assert all(int(t) % XCDS == x for t in col[:k])


def synthetic_scan(weight, cap):
    """chunks of a tile: the weights of its columns in its band, summed (a weight per output column times the tile's width)"""
    def scan(tiles):
        out = []
        for t in tiles:
            c = int(weight[t.band, t.x0:t.x0 + t.w].sum())
            out.append(slh.TOO_LARGE if c > cap else c)
        return out
    return scan


@pytest.mark.parametrize("tileW", [64, 128, 256, 512])
def test_tile_cutting_partitions_every_band_and_narrows_only_heavy_ones(lib, tileW):
    rng = np.random.default_rng(tileW)
    tileH, cap = 8, 2000
    kept_seen = given_up_seen = narrowed_seen = gather_seen = 0
    for trial in range(60):
        outX = int(rng.choice([64, 100, 512, 1000, 1024, 1500]))
        nBands = int(rng.integers(1, 7))
        outY = nBands * tileH - int(rng.integers(0, tileH))
        # per band a weight level up to three times what the widest tile holds, some bands empty, and a few columns no tile can hold
        level = rng.choice([0.0, 0.3, 0.8, 1.5, 3.0], nBands) * cap / tileW
        weight = np.floor(level[:, None] * rng.uniform(0.5, 1.5, (nBands, outX))).astype(np.int64)
        spikes = int(rng.choice([0, 0, 1, 3, 40]))
        for _ in range(spikes):
            weight[int(rng.integers(0, nBands)), int(rng.integers(0, outX))] = cap + 1
        passes, kept, total = slh.cut_tiles(lib, outX, outY, tileW, tileH, synthetic_scan(weight, cap))
        assert len(passes) <= 64
        step = 64 if tileW >= 128 else 32
        for tiles in passes:
            for b in range(nBands):
                band = [t for t in tiles if t.band == b]
                assert band[0].x0 == 0 and band[-1].x0 + band[-1].w == outX and all(t.y0 == b * tileH for t in band)
                assert all(l.x0 + l.w == r.x0 for l, r in zip(band, band[1:])), "a gap or an overlap"
                assert all(t.w % step == 0 for t in band[:-1]) and all(0 < t.w <= tileW for t in band)
                assert all(t.w <= step for t in band if t.gather)
        failed = lambda t: not t.gather and t.chunks == slh.TOO_LARGE
        for before, after in zip(passes, passes[1:]):
            for b in range(nBands):
                old, new = [t for t in before if t.band == b], [t for t in after if t.band == b]
                nf = sum(failed(t) for t in old)
                if new[0].band_w != old[0].band_w:  # narrowed: only because most of its tiles failed, and by one step
                    assert 2 * nf > len(old) and new[0].band_w == old[0].band_w - step
                    assert all(t.w == new[0].band_w for t in new[:-1]) and not any(t.gather for t in new)
                    narrowed_seen += 1
                else:  # tiles that fit stay; a failing one is split on a step boundary, or becomes a gather tile
                    place = {t.x0: t for t in new}
                    for t in old:
                        if not failed(t):
                            assert place[t.x0].w == t.w and place[t.x0].gather == t.gather
                        elif t.w <= step:
                            assert place[t.x0].w == t.w and place[t.x0].gather
                        else:
                            l = place[t.x0]
                            r = place[t.x0 + l.w]
                            assert l.w == (t.w // 2 + step - 1) // step * step and l.w + r.w == t.w and not l.gather and not r.gather
        last = passes[-1]
        assert not any(failed(t) for t in last)
        gather = sum(t.w for t in last if t.gather)
        live = sum(t.w for t in last if t.gather or t.chunks != 0)
        assert kept == (not gather * 8 > live)
        gather_seen += gather > 0
        if kept:
            kept_seen += 1
            assert total == sum(t.chunks for t in last)
            assert [t.chunk_base for t in last] == [int(v) for v in np.cumsum([0] + [t.chunks for t in last[:-1]])]
        else:
            given_up_seen += 1
    assert kept_seen > 10 and narrowed_seen > 5 and gather_seen > 5
    assert given_up_seen > 0 or tileW == 512


def z_starts(call, nz0, count):
    kmax = 31
    zs, n = np.zeros((count, kmax + 1), np.uint32), np.zeros(count, np.uint32)
    call(zs, n)
    return zs.astype(np.int64), n.astype(np.int64)


def check_partition(zs, n, nz, most):
    """zStart starts at 0, ends at nz and strictly increases, with at most `most` chunks"""
    assert (n >= 1).all() and (n <= most).all()
    assert (zs[:, 0] == 0).all() and (zs[np.arange(len(n)), n] == nz).all()
    size = np.diff(zs, axis=1)
    inside = np.arange(size.shape[1])[None, :] < n[:, None]
    assert (size[inside] > 0).all()
    return size, inside


NZ = np.arange(1, 4097)


def test_z_chunks_of_the_tile_major_order_are_even_and_at_most_16(lib):
    for zpb in range(1, 65):
        ok = np.zeros(len(NZ), np.uint8)
        zs, n = z_starts(lambda zs, n: lib.sl_float_z_chunks(1, len(NZ), 1, zpb, 0, zs.ctypes.data, n.ctypes.data, ok.ctypes.data), 1, len(NZ))
        assert ok.all()
        size, inside = check_partition(zs, n, NZ, 16)
        assert (np.where(inside, size, 0).max(axis=1) - np.where(inside, size, 1 << 40).min(axis=1) <= 1).all()


def test_z_chunks_of_the_chunk_major_order_partition_the_batch(lib):
    """One corner is left out: STAGE2_ZTAIL 1 on 3200 slices and more.  The chunks before the tail are then 128 slices and longer, the
    tail halves them down to one slice, and 23 chunks plus nine halvings are more than the kernel argument holds (first input:
    zpb 1, ztail 1, nz 3200).  The rule says so (false: the launch is refused with "too many z chunks") and writes nothing past
    its table; every other tail length fits at every batch length."""
    for zpb in range(1, 65):
        for ztail in range(0, 17):
            ok = np.zeros(len(NZ), np.uint8)
            zs, n = z_starts(lambda zs, n: lib.sl_float_z_chunks(1, len(NZ), 0, zpb, ztail, zs.ctypes.data, n.ctypes.data, ok.ctypes.data), 1, len(NZ))
            inside = ok != 0
            assert inside[~((ztail == 1) & (NZ >= 3200))].all(), (zpb, ztail, int(NZ[~inside][0]))
            check_partition(zs[inside], n[inside], NZ[inside], lib.sl_max_z_chunks())


def test_z_chunks_of_stored_types_and_of_the_first_form(lib):
    for zpb in range(1, 65):
        zs, n = z_starts(lambda zs, n: lib.sl_typed_z_chunks(1, len(NZ), zpb, zs.ctypes.data, n.ctypes.data), 1, len(NZ))
        size, inside = check_partition(zs, n, NZ, 16)
        assert (n >= np.minimum(4, NZ // 6)).all()
        assert (np.where(inside, size, 0).max(axis=1) - np.where(inside, size, 1 << 40).min(axis=1) <= 1).all()
        per, chunks = np.zeros(len(NZ), np.uint32), np.zeros(len(NZ), np.uint64)
        lib.sl_first_form_z(1, len(NZ), zpb, per.ctypes.data, chunks.ctypes.data)
        per, chunks = per.astype(np.int64), chunks.astype(np.int64)
        assert (per == np.minimum(zpb, NZ)).all() and (chunks == -(-NZ // per)).all()  # chunk c = slices [c * per, min(nz, (c + 1) * per))


def test_chunk_cap_of_the_default_bilinear_shape(lib):
    """1024 threads, 159 KiB of LDS in two slots, five chunks per lane: the slot counts, 5056 chunks"""
    assert lib.sl_tile_chunk_cap(159 * 1024, 2, 5, 1024, 4) == 5056
    assert lib.sl_tile_chunk_cap(79 * 1024, 2, 6, 512, 16) == 2496 and lib.sl_tile_chunk_cap(159 * 1024, 2, 5, 1024, 16) == 4095
