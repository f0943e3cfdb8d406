// fimex_amd/csrc/hostpipe_layout.hpp for the CPU tests (tests/test_hostpipe_layout.py, through tests/hostpipe_layout_host.py): the
// ring's sizes, the slices of a chunk, the chunks of a call, the pieces of a chunk and the chunk to drain before a slot is used
// again.  sizes[4] everywhere: slot, piece, float scratch, staged-copy threshold, in bytes.
#include <cstdint>

#include "hostpipe_layout.hpp"

using namespace fimex_amd::hostpipe;

namespace {
RingSizes sizes_of(const uint64_t* s)
{
    RingSizes r;
    r.slotBytes = (size_t)s[0];
    r.pieceBytes = (size_t)s[1];
    r.floatBytes = (size_t)s[2];
    r.stagedCopyMin = (size_t)s[3];
    return r;
}
}  // namespace

extern "C" {

// the production sizes, then the slots of the ring and the events (pieces) of a slot
void hp_constants(uint64_t* out)
{
    const RingSizes r;
    out[0] = r.slotBytes;
    out[1] = r.pieceBytes;
    out[2] = r.floatBytes;
    out[3] = r.stagedCopyMin;
    out[4] = (uint64_t)kSlots;
    out[5] = (uint64_t)kPieces;
}

// 1 where a pipe refuses these sizes
int hp_refused(const uint64_t* sizes) { return refuse(sizes_of(sizes)) != nullptr ? 1 : 0; }

// slices[4] each limit allows (pinned in, pinned out, float in, float out), *binding the one that decides; returns the slices per
// chunk, 0 where a slice does not fit
uint64_t hp_slices_per_chunk(const uint64_t* sizes, uint64_t inSliceBytes, uint64_t outSliceBytes, uint64_t inSliceFloats, uint64_t outSliceFloats,
                             uint64_t* slices, int* binding)
{
    const SliceLimits l = slice_limits(sizes_of(sizes), (size_t)inSliceBytes, (size_t)outSliceBytes, (size_t)inSliceFloats, (size_t)outSliceFloats);
    for (int k = 0; k < 4; ++k) slices[k] = l.slices[k];
    *binding = (int)binding_limit(l);
    return slices_per_chunk(l);
}

// the chunks of nz slices, `fit` fitting a slot: first[c] and units[c] for c < room; returns the chunk count
uint64_t hp_slice_chunks(uint64_t nz, uint64_t fit, uint64_t room, uint64_t* first, uint64_t* units)
{
    const Chunks ch = slice_chunks((size_t)nz, (size_t)fit);
    for (size_t c = 0; c < ch.count() && c < room; ++c) {
        first[c] = ch.first(c);
        units[c] = ch.units(c);
    }
    return ch.count();
}

// the chunks of a plain copy of `bytes`
uint64_t hp_byte_chunks(const uint64_t* sizes, uint64_t bytes, uint64_t room, uint64_t* first, uint64_t* units)
{
    const Chunks ch = byte_chunks((size_t)bytes, sizes_of(sizes));
    for (size_t c = 0; c < ch.count() && c < room; ++c) {
        first[c] = ch.first(c);
        units[c] = ch.units(c);
    }
    return ch.count();
}

// the pieces of a chunk of `bytes`: off[q], len[q] for q < room; returns the piece count
uint64_t hp_pieces(uint64_t bytes, uint64_t pieceBytes, uint64_t room, uint64_t* off, uint64_t* len)
{
    const size_t n = piece_count((size_t)bytes, (size_t)pieceBytes);
    for (size_t q = 0; q < n && q < room; ++q) {
        const Piece p = piece_at((size_t)bytes, (size_t)pieceBytes, q);
        off[q] = p.off;
        len[q] = p.len;
    }
    return n;
}

// the chunk to drain before chunk c starts, -1 where there is none; *slot: the slot chunk c goes into
int64_t hp_drain_before(uint64_t c, uint64_t slots, uint64_t* slot)
{
    size_t d = 0;
    *slot = slot_of((size_t)c, (size_t)slots);
    return drain_before((size_t)c, (size_t)slots, &d) ? (int64_t)d : -1;
}

}  // extern "C"
