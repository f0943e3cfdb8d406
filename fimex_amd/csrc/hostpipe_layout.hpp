// The arithmetic of the host transfer ring (hostpipe.hip): the one statement of it.  Which sizes the ring has, how many slices go
// into one chunk, where a chunk and each of its pieces lie, which chunk has to be drained before a slot is used again, and the
// memcpy on several threads that fills and empties the pinned staging.  Plain values in, plain values out: no HIP type, no
// tuning() call, so that tests/test_hostpipe_layout.py compiles it with g++ and walks every boundary on the CPU, and
// tests/hostpipe_copier_main.cc runs the copier under the host sanitizers.  hostpipe.hip keeps none of these rules itself.
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace fimex_amd {
namespace hostpipe {

constexpr size_t kPinBytes = (size_t)64 << 20;        // pinned staging per slot and direction
constexpr size_t kDevFloatBytes = (size_t)128 << 20;  // float scratch per slot and direction (typed slices)
constexpr int kSlots = 3;
constexpr size_t kPiece = (size_t)8 << 20;  // a slot's transfer goes in pieces: host memcpy of one overlaps the DMA of the other
constexpr int kPieces = (int)(kPinBytes / kPiece);  // events per slot: sized for the production sizes, whatever a tuning build asks for
constexpr size_t kStagedCopyMin = (size_t)16 << 20;  // below this a plain copy is as fast

// the sizes one pipe works with: the constants above in the product build, switches of the tuning build
struct RingSizes {
    size_t slotBytes = kPinBytes, pieceBytes = kPiece, floatBytes = kDevFloatBytes, stagedCopyMin = kStagedCopyMin;
    bool operator==(const RingSizes& o) const
    {
        return slotBytes == o.slotBytes && pieceBytes == o.pieceBytes && floatBytes == o.floatBytes && stagedCopyMin == o.stagedCopyMin;
    }
};

// nullptr, or why a pipe cannot work with these sizes: a slot never has more pieces than it has events
inline const char* refuse(const RingSizes& s)
{
    if (s.slotBytes == 0 || s.pieceBytes == 0 || s.floatBytes == 0) return "host ring: slot, piece and float scratch sizes must be positive";
    if ((s.slotBytes + s.pieceBytes - 1) / s.pieceBytes > (size_t)kPieces) return "host ring: more pieces per slot than the slot has events";
    return nullptr;
}

// The four byte limits of a chunk of slices, as slices each allows: the pinned slot against the incoming and the outgoing slice, the
// float scratch against their float forms (0 floats: the call does not use that scratch, and the limit is the scratch's byte count).
enum Limit { PinIn = 0, PinOut = 1, FloatIn = 2, FloatOut = 3 };
struct SliceLimits {
    size_t slices[4];
};

inline SliceLimits slice_limits(const RingSizes& s, size_t inSliceBytes, size_t outSliceBytes, size_t inSliceFloats, size_t outSliceFloats)
{
    return {{s.slotBytes / std::max<size_t>(inSliceBytes, 1), s.slotBytes / std::max<size_t>(outSliceBytes, 1),
             s.floatBytes / std::max<size_t>(inSliceFloats * 4, 1), s.floatBytes / std::max<size_t>(outSliceFloats * 4, 1)}};
}

// slices per chunk before the call's own nz caps it; 0: a single slice does not fit
inline size_t slices_per_chunk(const SliceLimits& l) { return std::min({l.slices[0], l.slices[1], l.slices[2], l.slices[3]}); }

// the limit that decides, the first of them where several allow the same count
inline Limit binding_limit(const SliceLimits& l)
{
    int b = 0;
    for (int k = 1; k < 4; ++k)
        if (l.slices[k] < l.slices[b]) b = k;
    return (Limit)b;
}

// nz units (slices, or bytes for a plain copy) in chunks of at most `per`
struct Chunks {
    size_t nz = 0, per = 1;
    size_t count() const { return (nz + per - 1) / per; }
    size_t first(size_t c) const { return c * per; }
    size_t units(size_t c) const { return std::min(per, nz - c * per); }
};

// nz slices, `fit` of them fitting a slot (slices_per_chunk, not 0)
inline Chunks slice_chunks(size_t nz, size_t fit) { return {nz, std::max<size_t>(std::min(fit, nz), 1)}; }
// a plain copy: chunks of one slot
inline Chunks byte_chunks(size_t bytes, const RingSizes& s) { return {bytes, s.slotBytes}; }

// a chunk's bytes go in pieces, all of pieceBytes but the last
struct Piece {
    size_t off, len;
};
inline size_t piece_count(size_t bytes, size_t pieceBytes) { return (bytes + pieceBytes - 1) / pieceBytes; }
inline Piece piece_at(size_t bytes, size_t pieceBytes, size_t q)
{
    const size_t off = q * pieceBytes;
    return {off, std::min(pieceBytes, bytes - off)};
}

// Chunk c goes into slot c % slots.  True, and the chunk in *drain, where that slot still holds an earlier chunk, which has to be
// drained (its result copied out, its upload waited for) before chunk c may start.
inline bool drain_before(size_t c, size_t slots, size_t* drain)
{
    if (c < slots) return false;
    *drain = c - slots;
    return true;
}
inline size_t slot_of(size_t c, size_t slots) { return c % slots; }

// memcpy on several threads: the workers live as long as the pipe
class ParallelCopier {
public:
    explicit ParallelCopier(int workers)
    {
        for (int i = 0; i < workers; ++i) threads_.emplace_back([this, i] { run(i); });
    }
    ~ParallelCopier()
    {
        { std::lock_guard<std::mutex> l(m_); stop_ = true; ++generation_; }
        cv_.notify_all();
        for (auto& t : threads_) t.join();
    }
    ParallelCopier(const ParallelCopier&) = delete;
    ParallelCopier& operator=(const ParallelCopier&) = delete;
    void copy(void* dst, const void* src, size_t bytes)
    {
        const size_t parts = threads_.size() + 1;
        if (bytes < ((size_t)1 << 20) || threads_.empty()) {
            if (bytes) std::memcpy(dst, src, bytes);
            return;
        }
        const size_t per = ((bytes + parts - 1) / parts + 4095) & ~(size_t)4095;
        {
            std::lock_guard<std::mutex> l(m_);
            dst_ = static_cast<char*>(dst);
            src_ = static_cast<const char*>(src);
            bytes_ = bytes;
            per_ = per;
            pending_ = (int)threads_.size();
            ++generation_;
        }
        cv_.notify_all();
        part(threads_.size());  // the caller takes the last part
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [this] { return pending_ == 0; });
    }

private:
    void part(size_t k)
    {
        const size_t off = k * per_;
        if (off < bytes_) std::memcpy(dst_ + off, src_ + off, std::min(per_, bytes_ - off));
    }
    void run(int k)
    {
        unsigned long long seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [&] { return generation_ != seen; });
                seen = generation_;
                if (stop_) return;
            }
            part((size_t)k);
            std::lock_guard<std::mutex> l(m_);
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    unsigned long long generation_ = 0;
    bool stop_ = false;
    char* dst_ = nullptr;
    const char* src_ = nullptr;
    size_t bytes_ = 0, per_ = 0;
    int pending_ = 0;
};

}  // namespace hostpipe
}  // namespace fimex_amd
