"""fimex_amd/csrc/hostpipe_layout.hpp, the arithmetic of the host transfer ring (hostpipe.hip), on the CPU.  Every *_host entry
moves its data through that ring: chunks of as many slices as fit a pinned slot and the float scratch, each chunk moved in pieces,
three slots used in turn, a slot used again only once the chunk three places back has been drained.  A wrong offset there corrupts
a caller's data without an error, so the header's answers are compared here with a plain restatement, around every boundary, at
the production sizes and at the small sizes tests/test_gpu_host_ring.py runs the ring with.  The header's ParallelCopier runs as
a program of its own (tests/hostpipe_copier_main.cc) under the host sanitizers."""
import subprocess

import pytest

import hostpipe_layout_host as host


@pytest.fixture(scope="module")
def lib():
    return host.load()


SMALL = (256 * 1024, 32 * 1024, 512 * 1024, 64 * 1024)  # slot, piece, float scratch, threshold: test_gpu_host_ring.py's


# --------------------------------------------------------------------------------------------------------- the plain restatement
def ref_limits(sizes, in_bytes, out_bytes, in_floats, out_floats):
    slot, _, scratch, _ = sizes
    return [slot // max(in_bytes, 1), slot // max(out_bytes, 1), scratch // max(4 * in_floats, 1), scratch // max(4 * out_floats, 1)]


def ref_chunks(n, per):
    return [(first, min(per, n - first)) for first in range(0, n, per)]


def ref_pieces(nbytes, piece):
    return [(off, min(piece, nbytes - off)) for off in range(0, nbytes, piece)]


def walk(lib, sizes, in_bytes, out_bytes, in_floats, out_floats, nz):
    """The whole ring of one call: asserts that the pieces of all chunks tile both arrays exactly once and that no chunk exceeds a
    limit; returns (slices per chunk, chunks)."""
    slot, piece, scratch, _ = sizes
    label = (sizes, in_bytes, out_bytes, in_floats, out_floats, nz)
    fit, each, binding = host.slices_per_chunk(lib, sizes, in_bytes, out_bytes, in_floats, out_floats)
    want = ref_limits(sizes, in_bytes, out_bytes, in_floats, out_floats)
    assert each == want and fit == min(want) and binding == want.index(min(want)), (label, fit, each, binding, want)
    assert fit > 0, label
    per = min(fit, nz)
    chunks = host.slice_chunks(lib, nz, fit)
    assert chunks == ref_chunks(nz, per), (label, chunks[:4])
    for slice_bytes in (in_bytes, out_bytes):
        at = 0
        for first, units in chunks:
            nbytes = units * slice_bytes
            assert 0 < units <= per and nbytes <= slot and units * in_floats * 4 <= scratch and units * out_floats * 4 <= scratch, (label, first, units)
            got = host.pieces(lib, nbytes, piece)
            assert got == ref_pieces(nbytes, piece) and len(got) <= -(-slot // piece), (label, first, got[:3])
            for off, length in got:
                assert first * slice_bytes + off == at and 0 < length <= piece, (label, first, off, length, at)
                at += length
        assert at == nz * slice_bytes, (label, at)
    return per, len(chunks)


def nz_around(fit):
    return sorted({n for n in (1, fit - 1, fit, fit + 1, 3 * fit, 3 * fit + 1) if n > 0})


# ------------------------------------------------------------------------------------------------------------------ the sizes
def test_the_production_sizes(lib):
    c = host.constants(lib)
    assert c == {"slot": 64 << 20, "piece": 8 << 20, "float": 128 << 20, "staged_min": 16 << 20, "slots": 3, "pieces": 8}
    assert not host.refused(lib, host.production_sizes(lib)) and not host.refused(lib, SMALL)


def test_sizes_a_pipe_refuses(lib):
    """a slot has eight events, one per piece: sizes that need a ninth are refused, and so is a size of nothing"""
    slot, piece, scratch, least = SMALL
    assert not host.refused(lib, (slot, slot // 8, scratch, least))
    assert not host.refused(lib, (slot - 1, slot // 8, scratch, least))  # a short eighth piece
    assert host.refused(lib, (slot + 1, slot // 8, scratch, least))      # a ninth of one byte
    assert host.refused(lib, (slot, slot // 8 - 1, scratch, least))
    assert not host.refused(lib, (slot, slot, scratch, 0)) and not host.refused(lib, (slot, 2 * slot, scratch, least))
    for k in range(3):
        zero = list(SMALL)
        zero[k] = 0
        assert host.refused(lib, zero), zero


# ---------------------------------------------------------------------------------------------- slices per chunk and their pieces
@pytest.mark.parametrize("sizes", ["production", SMALL], ids=["production", "small"])
def test_pieces_tile_both_arrays_around_every_boundary(lib, sizes):
    sizes = host.production_sizes(lib) if sizes == "production" else sizes
    slot, piece = sizes[0], sizes[1]
    edges = [1, piece - 1, piece, piece + 1, slot - 1, slot]
    walked = 0
    for in_bytes in edges:
        for out_bytes in edges + [slot // 3 + 5]:  # chunks of two slices with a tail piece
            fit = min(ref_limits(sizes, in_bytes, out_bytes, 0, 0))
            for nz in nz_around(fit):
                per, n = walk(lib, sizes, in_bytes, out_bytes, 0, 0, nz)
                assert per == min(fit, nz) and n == -(-nz // per)
                walked += 1
    assert walked >= 100, walked


@pytest.mark.parametrize("sizes", ["production", SMALL], ids=["production", "small"])
def test_each_limit_as_the_binding_one(lib, sizes):
    """cells of one byte (their float form four times as large) make the float scratch bind; floats or a call without scratch
    make the pinned slot bind"""
    sizes = host.production_sizes(lib) if sizes == "production" else sizes
    slot, _, scratch, _ = sizes
    big, small = slot // 5 + 3, 1001  # cells per slice
    cases = {
        host.PIN_IN: (4 * big, 4 * small, 0, 0),           # float regrid, large source
        host.PIN_OUT: (4 * small, 4 * big, 0, 0),          # float regrid, large target
        host.FLOAT_IN: (big, small, big, small),           # one-byte cells, large source
        host.FLOAT_OUT: (small, big, small, big),          # one-byte cells, large target
    }
    for limit, (ib, ob, inf, outf) in cases.items():
        fit, each, binding = host.slices_per_chunk(lib, sizes, ib, ob, inf, outf)
        assert binding == limit and all(each[k] > each[limit] for k in range(4) if k != limit), (host.LIMITS[limit], each)
        assert fit == each[limit] and fit in (1, 2), (host.LIMITS[limit], fit)
        for nz in nz_around(fit) + [7 * fit + 1]:
            walk(lib, sizes, ib, ob, inf, outf, nz)
    # shorts: the pinned slot (2 bytes a cell of 64 MiB) and the float scratch (4 bytes a cell of 128 MiB) allow the same count at
    # the production sizes, and the first of them is named
    fit, each, binding = host.slices_per_chunk(lib, host.production_sizes(lib), 2 * big, 2 * small, big, small)
    assert each[host.PIN_IN] == each[host.FLOAT_IN] == fit and binding == host.PIN_IN


@pytest.mark.parametrize("sizes", ["production", SMALL], ids=["production", "small"])
def test_a_slice_larger_than_a_limit_does_not_fit(lib, sizes):
    sizes = host.production_sizes(lib) if sizes == "production" else sizes
    slot, _, scratch, _ = sizes
    cells = scratch // 4
    assert host.slices_per_chunk(lib, sizes, slot, slot, 0, 0)[0] == 1
    assert host.slices_per_chunk(lib, sizes, slot + 1, 4, 0, 0)[0] == 0
    assert host.slices_per_chunk(lib, sizes, 4, slot + 1, 0, 0)[0] == 0
    assert host.slices_per_chunk(lib, sizes, cells, 4, cells, 1)[0] == 1
    assert host.slices_per_chunk(lib, sizes, cells + 1, 4, cells + 1, 1)[0] == 0
    assert host.slices_per_chunk(lib, sizes, 4, cells + 1, 1, cells + 1)[0] == 0


def test_the_chunks_of_the_full_size_case(lib):
    """tests/test_gpu_fullsize.py::test_host_calls_with_slices_beyond_the_staging_buffers: 11 slices of 2400 x 2300 floats"""
    per, n = walk(lib, host.production_sizes(lib), 2400 * 2300 * 4, 300 * 200 * 4, 0, 0, 11)
    assert (per, n) == (3, 4)
    assert host.slice_chunks(lib, 11, 3) == [(0, 3), (3, 3), (6, 3), (9, 2)]


# --------------------------------------------------------------------------------------------------------------- plain copies
@pytest.mark.parametrize("sizes", ["production", SMALL], ids=["production", "small"])
def test_plain_copies_go_in_chunks_of_a_slot(lib, sizes):
    sizes = host.production_sizes(lib) if sizes == "production" else sizes
    slot = sizes[0]
    for nbytes in (1, slot - 1, slot, slot + 1, 3 * slot, 3 * slot + 4, 3 * slot + 4096 + 4, 7 * slot + 12345):
        chunks = host.byte_chunks(lib, sizes, nbytes)
        assert chunks == ref_chunks(nbytes, slot), (nbytes, chunks)
        assert sum(n for _, n in chunks) == nbytes and all(0 < n <= slot for _, n in chunks)
        assert [first for first, _ in chunks] == [c * slot for c in range(len(chunks))]


# ------------------------------------------------------------------------------------------------------------------ the ring
def test_the_chunk_to_drain_before_a_slot_is_used_again(lib):
    for slots in (1, 2, 3, 4):
        for c in range(4 * slots + 2):
            drain, slot = host.drain_before(lib, c, slots)
            assert slot == c % slots
            assert drain == (c - slots if c >= slots else None), (slots, c, drain)
            if drain is not None:
                assert host.drain_before(lib, drain, slots)[1] == slot  # the chunk that held this slot before


def test_a_ring_walked_in_order_never_holds_two_chunks_in_a_slot(lib):
    """the order of hostpipe.hip: before chunk c starts its drain is finished, at the end every chunk not yet finished; each chunk
    is finished exactly once, in order, and while it is in flight no other chunk writes its slot"""
    slots = host.constants(lib)["slots"]
    for n in range(1, 12):
        holds, finished = {}, []
        for c in range(n):
            drain, slot = host.drain_before(lib, c, slots)
            if drain is not None:
                assert holds.pop(host.drain_before(lib, drain, slots)[1]) == drain
                finished.append(drain)
            assert slot not in holds, (n, c, holds)
            holds[slot] = c
        finished += sorted(holds.values())
        assert finished == list(range(n)), (n, finished)


# ---------------------------------------------------------------------------------------------------------------- the copier
@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_the_copier_program_under_the_host_sanitizers(sanitizer):
    """0, 1, 3, 7 and 31 workers; 0 bytes to 64 MiB around the 1 MiB threshold of the threaded path, with guard bytes; 400 copies
    back to back on one copier; copiers made and destroyed unused.  Where the host compiler has no runtime of a sanitizer the
    program is built and run plain, and the output says so."""
    plain, err = host.build_copier()
    assert plain is not None, err
    exe, err = host.build_copier(["-fsanitize=" + sanitizer, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if exe is None:
        print("no -fsanitize=%s with this compiler, the program runs plain:\n%s" % (sanitizer, err[-400:]))
        exe = plain
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:], r.stderr[-3000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("copier ok"), (r.returncode, r.stdout[-300:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
