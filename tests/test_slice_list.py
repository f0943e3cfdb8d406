"""fimex_amd/csrc/slice_list.hpp, the slice addressing of the list kernels (staged2_list.hip, staged2_list_typed.hip), on the CPU: a
launch counts the slices of its variables as logical slices 0 .. total - 1, a workgroup owns a z chunk [z0, z1) of them -- which
may begin and end inside a variable -- and finds the variable and the level of every slice with two cursors that it seeds at z0
and moves one slice at a time, the source cursor DEPTH - 1 slices ahead of the one for the slice in work.  A cursor that is off by
one makes the base pointer of a foreign allocation, so every list of up to five variables of zero to four slices is walked over
every chunk [z0, z1) here, for rings of two and of three slots, against a numpy restatement."""
import itertools

import numpy as np
import pytest

import slice_list_host as host


@pytest.fixture(scope="module")
def lib():
    return host.load()


def _slices(nz):
    """(variable, level) of every logical slice of the list, variables counted as the caller counts them."""
    nz = np.asarray(nz, dtype=np.int64)
    var = np.repeat(np.arange(len(nz)), nz)
    starts = np.concatenate([[0], np.cumsum(nz)[:-1]]) if len(nz) else np.zeros(0, np.int64)
    level = np.arange(int(nz.sum())) - np.repeat(starts, nz)
    return np.stack([var, level], axis=1).astype(np.int32)


def _lists():
    for nvar in range(1, 6):
        yield from itertools.product(range(5), repeat=nvar)


def test_the_table_leaves_out_variables_without_slices(lib):
    for nz in _lists():
        ok, ends, index, total = host.build(lib, nz)
        assert ok and total == sum(nz)
        kept = [i for i, n in enumerate(nz) if n]
        assert list(index) == kept
        assert list(ends) == list(np.cumsum([nz[i] for i in kept]))


def test_the_table_takes_as_many_variables_as_a_launch(lib):
    k = lib.sl_max_vars()
    assert k == 64  # FIMEX_AMD_REGRID_MULTI_MAX_VARS
    ok, ends, index, total = host.build(lib, [1, 0] * k)
    assert ok and total == k and len(ends) == k and list(index) == list(range(0, 2 * k, 2))
    assert not host.build(lib, [1] * (k + 1))[0]
    assert not host.build(lib, [2 ** 31, 2 ** 31])[0]
    assert host.build(lib, [2 ** 31, 2 ** 31 - 1])[0]


@pytest.mark.parametrize("depth", [2, 3])
def test_both_cursors_name_the_right_slices_over_every_chunk(lib, depth):
    walks = 0
    for nz in _lists():
        want = _slices(nz)
        total = len(want)
        for z0 in range(total):
            for z1 in range(z0 + 1, total + 1):
                got = host.walk(lib, nz, z0, z1, depth)
                assert got is not None, "a cursor left the list: nz %s, chunk [%d, %d)" % (nz, z0, z1)
                fetched, worked = got
                n = z1 - z0
                # every slice of the chunk is fetched once and in order, and worked on in order
                assert np.array_equal(fetched[:, :2], want[z0:z1]), (nz, z0, z1)
                assert np.array_equal(worked, want[z0:z1]), (nz, z0, z1)
                # the first depth - 1 fetches come ahead of the loop, fetch k is issued by trip k - (depth - 1): the source
                # cursor runs depth - 1 slices ahead of the slice in work
                assert np.array_equal(fetched[:, 2], np.maximum(np.arange(n) - (depth - 1), -1)), (nz, z0, z1)
                walks += 1
    assert walks > 100000


def test_single_slice_variables_put_the_source_cursor_two_variables_ahead(lib):
    fetched, worked = host.walk(lib, [1] * 7 + [3], 0, 10, 3)
    for k in range(2, 10):  # the fetch that trip k - 2 issues
        trip = int(fetched[k, 2])
        assert trip == k - 2
        if k < 7:
            assert fetched[k, 0] == worked[trip, 0] + 2
    assert [tuple(r) for r in worked[7:]] == [(7, 0), (7, 1), (7, 2)]


def _random_lists():
    """lists of up to 300 entries of which a tenth to nine tenths are without slices, and the edges: zeros at either end, exactly
    one, two and three launches of live variables, nothing but zeros"""
    rng = np.random.default_rng(64)
    for _ in range(400):
        n = int(rng.integers(1, 301))
        nz = rng.integers(1, 6, n)
        nz[rng.random(n) < rng.uniform(0.1, 0.9)] = 0
        yield nz
    k = 64
    for live in (1, k - 1, k, k + 1, 2 * k, 2 * k + 1, 3 * k, 3 * k + 2):
        yield np.ones(live, np.int64)
        yield np.concatenate([[0, 0], np.ones(live, np.int64), [0]])
        yield np.stack([np.ones(live, np.int64), np.zeros(live, np.int64)], axis=1).ravel()  # a zero after every live variable
    yield np.zeros(7, np.int64)


def test_a_list_is_cut_into_launches_of_at_most_64_live_variables(lib):
    """for_list_launches: every live variable lies in exactly one launch, the launches are in order and leave no gap between
    them, none holds more than 64 live variables or none at all, every launch but the last is full, and build_slice_ends takes
    each (first, count) as it stands."""
    k = lib.sl_max_vars()
    cut = 0
    for nz in _random_lists():
        got = host.launches(lib, nz)
        live = np.flatnonzero(nz)
        assert host.list_slices(lib, nz) == int(nz.sum())
        assert len(got) == -(-len(live) // k), (list(nz), got)
        owner = np.full(len(nz), -1)
        end = None
        for j, (first, count, accepted) in enumerate(got):
            assert accepted and count > 0 and first + count <= len(nz), (list(nz), got)
            assert end is None or first == end, "launches out of order or with a gap"
            end = first + count
            assert (owner[first:end] == -1).all()
            owner[first:end] = j
            held = int(np.count_nonzero(nz[first:end]))
            assert 0 < held <= k and (held == k or j == len(got) - 1), (list(nz), got)
            assert j == 0 or nz[first] != 0  # a launch after a cut begins with the variable that did not fit
        if len(live):
            assert (owner[live] >= 0).all() and (np.diff(owner[live]) >= 0).all() and end == len(nz)
            assert got[0][0] == 0
        cut += len(got) > 1
    assert cut > 100


def test_a_list_of_too_many_slices_counts_as_none(lib):
    assert host.list_slices(lib, [2 ** 31, 0, 2 ** 31 - 1]) == 2 ** 32 - 1
    assert host.list_slices(lib, [2 ** 31, 0, 2 ** 31]) == 0
    assert host.list_slices(lib, []) == 0


def test_chunks_outside_the_list_are_refused_by_the_walker(lib):
    assert host.walk(lib, [2, 3], 0, 6, 2) is None
    assert host.walk(lib, [0, 0], 0, 1, 2) is None
