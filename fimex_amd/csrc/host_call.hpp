// One *_host call of the C boundary: the stream, every device copy made for it and the copies back.
//
// A *_host entry reads: check the caller's arguments, select the device as that entry always did (INTEGRATION.md lists the
// policies), launch on hc.in(...) / hc.out(...) pointers and hc.stream(), hc.finish().  Where the *_device twin states the same
// check and the same launch, both are one function template over the call type: HostCall copies, DeviceCall hands the caller's
// device pointers and stream through, so the checks that compare addresses always see the caller's own pointers.
//
// Failure path: the destructor waits for the stream, ignoring the result, before any buffer is released.  An exception anywhere
// between the first upload and finish() therefore leaves nothing in flight that reads or writes the caller's memory, and since
// only finish() queues the copies back, nothing is copied back to the caller after an error.
//
// Copies go through host_to_device / device_to_host (hostpipe.hip): arrays of 16 MiB and more take the pinned ring.
#pragma once

#include "plan.hpp"

#include <optional>
#include <vector>

#pragma GCC visibility push(hidden)  // inline code of the capi_*.hip files, no part of the library's exported symbols
namespace fimex_amd {

// device pointers of an array that is read and then written: one buffer in a host call (the kernels work in place, as the
// reference does), the caller's two pointers in a device call
template <typename T>
struct Through {
    const T* in;
    T* out;
};

class HostCall {
public:
    HostCall() = default;
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;
    ~HostCall()
    {
        if (stream_) (void)hipStreamSynchronize(stream_->get());  // nothing in flight when the buffers go
        buffers_.clear();
    }

    // created at first use: a temporary HostCall handed to a call that its checks refuse costs nothing
    hipStream_t stream()
    {
        if (!stream_) stream_.emplace();
        return stream_->get();
    }
    // device copy of h[n]; nullptr, with no allocation and no copy, for NULL or n == 0
    template <typename T>
    T* in(const T* h, size_t n) { return through<T>(h, nullptr, n).out; }
    // device buffer that finish() copies to h[n]
    template <typename T>
    T* out(T* h, size_t n) { return static_cast<T*>(buffer(n * sizeof(T), h)); }
    template <typename T>
    T* inout(T* h, size_t n) { return through<T>(h, h, n).out; }
    // device copy of hIn[n] that finish() copies to hOut[n]: in-place work on the device that leaves hIn as it was
    template <typename T>
    Through<T> through(const T* hIn, T* hOut, size_t n)
    {
        if (!hIn || !n) return {nullptr, nullptr};
        T* d = static_cast<T*>(buffer(n * sizeof(T), hOut));
        host_to_device(d, hIn, n * sizeof(T), stream());
        return {d, d};
    }
    // arrays in a stored type: void* and a size in bytes
    void* in_bytes(const void* h, size_t bytes) { return in(static_cast<const unsigned char*>(h), bytes); }
    void* out_bytes(void* h, size_t bytes) { return buffer(bytes, h); }

    void finish()
    {
        for (const Buffer& b : buffers_)
            if (b.host && b.mem.bytes()) device_to_host(b.host, b.mem.get(), b.mem.bytes(), stream());
        if (stream_) stream_->sync();
    }

private:
    struct Buffer {
        DeviceArray<unsigned char> mem;
        void* host;  // where finish() copies it, or nullptr
    };
    void* buffer(size_t bytes, void* host)
    {
        buffers_.push_back(Buffer{DeviceArray<unsigned char>(bytes), host});
        return buffers_.back().mem.get();
    }
    std::optional<ScopedStream> stream_;
    std::vector<Buffer> buffers_;
};

// the *_device form of the same call: the caller's device pointers and stream, nothing copied, nothing to wait for
struct DeviceCall {
    hipStream_t st;
    hipStream_t stream() const { return st; }
    template <typename T> const T* in(const T* d, size_t) const { return d; }
    template <typename T> T* out(T* d, size_t) const { return d; }
    template <typename T> T* inout(T* d, size_t) const { return d; }
    template <typename T> Through<T> through(const T* dIn, T* dOut, size_t) const { return {dIn, dOut}; }
    const void* in_bytes(const void* d, size_t) const { return d; }
    void* out_bytes(void* d, size_t) const { return d; }
    void finish() const {}
};

// the device of a plan object in an apply: the device form demands it, the host form switches to it for the call
struct PlanDevice {
    bool switchTo;
    std::optional<ScopedDevice> scoped;
    void enter(int device)
    {
        if (switchTo) scoped.emplace(device);
        else require_current_device(device);
    }
};

// a level description for the launch: the caller's own for a device call, with device copies of its 2-D / 3-D members for a
// host call
inline fimex_amd_vertical_levels levels_on(const DeviceCall&, const fimex_amd_vertical_levels& l, size_t, size_t) { return l; }

inline fimex_amd_vertical_levels levels_on(HostCall& hc, const fimex_amd_vertical_levels& h, size_t plane, size_t nt)
{
    fimex_amd_vertical_levels d = h;
    d.ps = nullptr;
    d.field = nullptr;
    if (h.kind == FIMEX_AMD_VLEVEL_FIELD) d.field = hc.in(h.field, nt * h.nz * plane);
    else if (h.kind != FIMEX_AMD_VLEVEL_AXIS) d.ps = hc.in(h.ps, nt * plane);
    return d;
}

}  // namespace fimex_amd
#pragma GCC visibility pop
