// The *_host entry points move caller-owned, pageable buffers over PCIe: that, not the kernels, is what a drop-in caller
// waits for (measured on this pool, scripts/calib/pcie.hip: pageable hipMemcpy 24 GB/s up / 32 GB/s down, pinned 57 GB/s
// each way and 75 GB/s duplex, hipHostRegister 50 ms per GB -- not worth it per call, host memcpy 30 GB/s on one thread,
// 127 GB/s on eight).  So slices are streamed: a few worker threads copy the next chunk into pinned staging while the DMA
// engines upload the previous one, the kernels run, and results flow back the same way in the other direction.
#include "plan.hpp"

#include "hostpipe_layout.hpp"

namespace fimex_amd {

using namespace hostpipe;  // the ring's sizes and arithmetic, and the copier: hostpipe_layout.hpp

namespace {

constexpr int kMaxCached = 4;  // idle pipes kept for the next call
constexpr int kMaxLive = 8;    // pipes in use at once: further callers wait for one (each pins up to 384 MB of host memory)

// the product build works with the constants of hostpipe_layout.hpp; the tuning build reads them per call, so that the tests reach
// every branch of the ring with a few MB (FIMEX_AMD_HOST_SLOT_BYTES, _PIECE_BYTES, _FLOAT_BYTES, _STAGED_MIN_BYTES)
RingSizes ring_sizes()
{
    RingSizes s;
#ifdef FIMEX_AMD_TUNING
    s.slotBytes = (size_t)tuning("HOST_SLOT_BYTES", (int)s.slotBytes);
    s.pieceBytes = (size_t)tuning("HOST_PIECE_BYTES", (int)s.pieceBytes);
    s.floatBytes = (size_t)tuning("HOST_FLOAT_BYTES", (int)s.floatBytes);
    s.stagedCopyMin = (size_t)tuning("HOST_STAGED_MIN_BYTES", (int)s.stagedCopyMin);
    if (const char* why = refuse(s)) throw Error(why);
#endif
    return s;
}

struct Slot {
    char *pinIn = nullptr, *pinOut = nullptr, *dRawIn = nullptr, *dRawOut = nullptr;
    float *dFIn = nullptr, *dFOut = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t piece[kPieces] = {};   // piece p of the result has arrived in pinOut
};

// Buffers are made on first use and only the kind a call needs: host_to_device touches pinIn alone, a float regrid the four
// raw buffers, only a conversion of stored types the float scratch (3 x 256 MB of HBM otherwise held for nothing).
class HostPipe {
public:
    HostPipe(int device, const RingSizes& sizes) : device(device), sizes(sizes), copier(worker_count())
    {
        for (Slot& s : slots) {
            FA_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
            FA_HIP(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
            for (hipEvent_t& e : s.piece) FA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
    }
    ~HostPipe()
    {
        for (Slot& s : slots) {
            if (s.stream) (void)hipStreamSynchronize(s.stream);
            if (s.pinIn) (void)hipHostFree(s.pinIn);
            if (s.pinOut) (void)hipHostFree(s.pinOut);
            if (s.dRawIn) (void)hipFree(s.dRawIn);
            if (s.dRawOut) (void)hipFree(s.dRawOut);
            if (s.dFIn) (void)hipFree(s.dFIn);
            if (s.dFOut) (void)hipFree(s.dFOut);
            if (s.done) (void)hipEventDestroy(s.done);
            for (hipEvent_t e : s.piece) if (e) (void)hipEventDestroy(e);
            if (s.stream) (void)hipStreamDestroy(s.stream);
        }
    }
    enum Need { PinIn = 1, PinOut = 2, RawIn = 4, RawOut = 8, FloatIn = 16, FloatOut = 32 };
    void ensure(Slot& s, int need)
    {
        if ((need & PinIn) && !s.pinIn) FA_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.pinIn), sizes.slotBytes));
        if ((need & PinOut) && !s.pinOut) FA_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.pinOut), sizes.slotBytes));
        if ((need & RawIn) && !s.dRawIn) FA_HIP(hipMalloc(reinterpret_cast<void**>(&s.dRawIn), sizes.slotBytes));
        if ((need & RawOut) && !s.dRawOut) FA_HIP(hipMalloc(reinterpret_cast<void**>(&s.dRawOut), sizes.slotBytes));
        if ((need & FloatIn) && !s.dFIn) FA_HIP(hipMalloc(reinterpret_cast<void**>(&s.dFIn), sizes.floatBytes));
        if ((need & FloatOut) && !s.dFOut) FA_HIP(hipMalloc(reinterpret_cast<void**>(&s.dFOut), sizes.floatBytes));
    }
    static int worker_count()
    {
        const int forced = tuning("HOST_COPY_THREADS", 0);
        if (forced > 0) return forced - 1;
        const unsigned hw = std::thread::hardware_concurrency();
        return (int)std::min(7u, std::max(1u, hw / 4));
    }
    int device;
    RingSizes sizes;  // what the buffers were made for: a pipe serves calls with these sizes only
    Slot slots[kSlots];
    ParallelCopier copier;
};

std::mutex g_poolMutex;
std::condition_variable g_poolFree;
std::vector<HostPipe*> g_pool;
int g_live = 0;  // pipes handed out

HostPipe* acquire_pipe(int device, const RingSizes& sizes)
{
    {
        std::unique_lock<std::mutex> l(g_poolMutex);
        // concurrent callers (interpolateValues is re-entrant) get a pipe each, up to kMaxLive; the next one waits
        g_poolFree.wait(l, [] { return g_live < kMaxLive; });
        ++g_live;
        for (size_t i = 0; i < g_pool.size(); ++i)
            if (g_pool[i]->device == device && g_pool[i]->sizes == sizes) {
                HostPipe* p = g_pool[i];
                g_pool.erase(g_pool.begin() + (long)i);
                return p;
            }
    }
    try {
        return new HostPipe(device, sizes);
    } catch (...) {
        { std::lock_guard<std::mutex> l(g_poolMutex); --g_live; }
        g_poolFree.notify_one();
        throw;
    }
}

void release_pipe(HostPipe* p)
{
    bool keep = false;
    {
        std::lock_guard<std::mutex> l(g_poolMutex);
        --g_live;
        if ((int)g_pool.size() < kMaxCached) { g_pool.push_back(p); keep = true; }
    }
    g_poolFree.notify_one();
    if (!keep) delete p;
}

struct PipeLease {
    PipeLease(int device, const RingSizes& sizes) : pipe(acquire_pipe(device, sizes)) {}
    ~PipeLease() { release_pipe(pipe); }
    HostPipe* pipe;
};

}  // namespace

// in / out: nz slices of inSliceBytes / outSliceBytes in caller memory.  fn(dRawIn, dRawOut, dFIn, dFOut, n, stream) turns
// n uploaded slices into n result slices in dRawOut (dFIn / dFOut: float scratch of inSliceFloats / outSliceFloats per
// slice).  Returns false when a single slice does not fit the staging buffers (the caller takes the plain path).
bool pipelined_slices(int device, const void* in, size_t inSliceBytes, void* out, size_t outSliceBytes, size_t inSliceFloats,
                      size_t outSliceFloats, size_t nz, const SliceChunkFn& fn)
{
    if (tuning("HOST_PIPE", 1) == 0 || nz == 0) return false;
    const RingSizes sizes = ring_sizes();
    const size_t fit = slices_per_chunk(slice_limits(sizes, inSliceBytes, outSliceBytes, inSliceFloats, outSliceFloats));
    if (fit == 0) return false;
    const Chunks chunks = slice_chunks(nz, fit);
    PipeLease lease(device, sizes);
    HostPipe& p = *lease.pipe;
    const int need = HostPipe::PinIn | HostPipe::PinOut | HostPipe::RawIn | HostPipe::RawOut | (inSliceFloats ? HostPipe::FloatIn : 0) |
                     (outSliceFloats ? HostPipe::FloatOut : 0);
    const size_t nChunks = chunks.count();
    for (size_t c = 0; c < std::min<size_t>(nChunks, kSlots); ++c) p.ensure(p.slots[c], need);
    const char* src = static_cast<const char*>(in);
    char* dst = static_cast<char*>(out);
    auto finish = [&](size_t c) {  // piece by piece: the host copy of one piece overlaps the DMA of the next
        Slot& s = p.slots[slot_of(c, kSlots)];
        const size_t bytes = chunks.units(c) * outSliceBytes;
        char* to = dst + chunks.first(c) * outSliceBytes;
        for (size_t q = 0, nq = piece_count(bytes, sizes.pieceBytes); q < nq; ++q) {
            const Piece pc = piece_at(bytes, sizes.pieceBytes, q);
            FA_HIP(hipEventSynchronize(s.piece[q]));
            p.copier.copy(to + pc.off, s.pinOut + pc.off, pc.len);
        }
        FA_HIP(hipEventSynchronize(s.done));
    };
    size_t finished = 0;
    try {
        for (size_t c = 0, drain = 0; c < nChunks; ++c) {
            Slot& s = p.slots[slot_of(c, kSlots)];
            if (drain_before(c, kSlots, &drain)) { finish(drain); finished = drain + 1; }
            const size_t k = chunks.units(c), inBytes = k * inSliceBytes, outBytes = k * outSliceBytes;
            const char* from = src + chunks.first(c) * inSliceBytes;
            for (size_t q = 0, nq = piece_count(inBytes, sizes.pieceBytes); q < nq; ++q) {
                const Piece pc = piece_at(inBytes, sizes.pieceBytes, q);
                p.copier.copy(s.pinIn + pc.off, from + pc.off, pc.len);
                FA_HIP(hipMemcpyAsync(s.dRawIn + pc.off, s.pinIn + pc.off, pc.len, hipMemcpyHostToDevice, s.stream));
            }
            fn(s.dRawIn, s.dRawOut, s.dFIn, s.dFOut, k, s.stream);
            for (size_t q = 0, nq = piece_count(outBytes, sizes.pieceBytes); q < nq; ++q) {
                const Piece pc = piece_at(outBytes, sizes.pieceBytes, q);
                FA_HIP(hipMemcpyAsync(s.pinOut + pc.off, s.dRawOut + pc.off, pc.len, hipMemcpyDeviceToHost, s.stream));
                FA_HIP(hipEventRecord(s.piece[q], s.stream));
            }
            FA_HIP(hipEventRecord(s.done, s.stream));
        }
        for (size_t c = finished; c < nChunks; ++c) finish(c);
    } catch (...) {
        for (Slot& s : p.slots) (void)hipStreamSynchronize(s.stream);  // nothing of this call may still be in flight
        throw;
    }
    return true;
}

// hipMemcpyAsync(HostToDevice) for caller-owned (pageable) memory: large copies go through the pinned ring with parallel
// memcpy (about 2x the pageable rate) and have landed when this returns; small ones are enqueued on `stream` as before
void host_to_device(void* d_dst, const void* h_src, size_t bytes, hipStream_t stream)
{
    if (bytes == 0) return;
    const RingSizes sizes = ring_sizes();
    if (bytes < sizes.stagedCopyMin || tuning("HOST_PIPE", 1) == 0) {
        FA_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, stream));
        return;
    }
    int device = 0;
    FA_HIP(hipGetDevice(&device));
    PipeLease lease(device, sizes);
    HostPipe& p = *lease.pipe;
    const Chunks chunks = byte_chunks(bytes, sizes);
    const size_t nChunks = chunks.count();
    for (size_t c = 0; c < std::min<size_t>(nChunks, kSlots); ++c) p.ensure(p.slots[c], HostPipe::PinIn);
    try {
        for (size_t c = 0, drain = 0; c < nChunks; ++c) {
            Slot& s = p.slots[slot_of(c, kSlots)];
            if (drain_before(c, kSlots, &drain)) FA_HIP(hipEventSynchronize(p.slots[slot_of(drain, kSlots)].done));
            const size_t off = chunks.first(c), len = chunks.units(c);
            p.copier.copy(s.pinIn, static_cast<const char*>(h_src) + off, len);
            FA_HIP(hipMemcpyAsync(static_cast<char*>(d_dst) + off, s.pinIn, len, hipMemcpyHostToDevice, s.stream));
            FA_HIP(hipEventRecord(s.done, s.stream));
        }
        for (Slot& s : p.slots) FA_HIP(hipStreamSynchronize(s.stream));
    } catch (...) {
        for (Slot& s : p.slots) (void)hipStreamSynchronize(s.stream);
        throw;
    }
}

// the reverse; waits for the work queued on `stream` first (it produced d_src) when it takes the staged path
void device_to_host(void* h_dst, const void* d_src, size_t bytes, hipStream_t stream)
{
    if (bytes == 0) return;
    const RingSizes sizes = ring_sizes();
    if (bytes < sizes.stagedCopyMin || tuning("HOST_PIPE", 1) == 0) {
        FA_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, stream));
        return;
    }
    FA_HIP(hipStreamSynchronize(stream));
    int device = 0;
    FA_HIP(hipGetDevice(&device));
    PipeLease lease(device, sizes);
    HostPipe& p = *lease.pipe;
    const Chunks chunks = byte_chunks(bytes, sizes);
    const size_t nChunks = chunks.count();
    for (size_t c = 0; c < std::min<size_t>(nChunks, kSlots); ++c) p.ensure(p.slots[c], HostPipe::PinOut);
    auto finish = [&](size_t c) {
        Slot& s = p.slots[slot_of(c, kSlots)];
        FA_HIP(hipEventSynchronize(s.done));
        p.copier.copy(static_cast<char*>(h_dst) + chunks.first(c), s.pinOut, chunks.units(c));
    };
    size_t finished = 0;
    try {
        for (size_t c = 0, drain = 0; c < nChunks; ++c) {
            Slot& s = p.slots[slot_of(c, kSlots)];
            if (drain_before(c, kSlots, &drain)) { finish(drain); finished = drain + 1; }
            FA_HIP(hipMemcpyAsync(s.pinOut, static_cast<const char*>(d_src) + chunks.first(c), chunks.units(c), hipMemcpyDeviceToHost, s.stream));
            FA_HIP(hipEventRecord(s.done, s.stream));
        }
        for (size_t c = finished; c < nChunks; ++c) finish(c);
    } catch (...) {
        for (Slot& s : p.slots) (void)hipStreamSynchronize(s.stream);
        throw;
    }
}

// frees the idle pipes (pinned host memory, device staging, copy threads); pipes in use are freed when their call returns and
// the cache is full, or by the next call of this
void release_host_pipes()
{
    std::vector<HostPipe*> idle;
    {
        std::lock_guard<std::mutex> l(g_poolMutex);
        idle.swap(g_pool);
    }
    for (HostPipe* p : idle) {
        int prev = 0;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(p->device);
        delete p;
        (void)hipSetDevice(prev);
    }
}

}  // namespace fimex_amd
