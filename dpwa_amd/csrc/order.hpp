// order.hpp -- which stream waits for which: the two event types behind every cross-stream
// dependency of a learner (learner.cpp).  Host only.
//
// Cross-stream ordering is recorded lazily: the stream of every publish / consumption is
// remembered (StreamMark::note) and an event is recorded (on that stream, at the moment a
// dependent operation is enqueued) only when the dependent operation runs on a different stream.
// In the common single-stream loop no event is recorded at all.  Where the dependent can never
// share the producer's stream (a staging buffer read on the caller's stream and refilled on the
// side stream) the event is recorded at once and waited for later (DoneEvent).
//
// Neither type knows about devices: a caller that orders against another device's learner
// switches devices around the call.
#pragma once

#include <hip/hip_runtime_api.h>

namespace dpwa {

// One HIP handle `h` and the call that gives it back, once; a moved-from owner holds nothing.
template <class T, hipError_t (*Free)(T)> struct Owned {
    T h = nullptr;
    Owned() = default;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = nullptr; }
    Owned &operator=(Owned &&o) noexcept   // `o` leaves with what this held, and frees it
    {
        T mine = h;
        h = o.h;
        o.h = mine;
        return *this;
    }
    ~Owned()
    {
        if (h) (void)Free(h);
    }
};

// A plain device allocation.
struct DevBuf : Owned<void *, hipFree> {
    hipError_t alloc(size_t bytes) { return hipMalloc(&h, bytes); }
    char *ptr() const { return (char *)h; }
};

// A non-blocking stream.
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t create() { return hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
    hipError_t create(int priority) { return hipStreamCreateWithPriority(&h, hipStreamNonBlocking, priority); }
};

// An event made by init() or at first need; hipEventDefault for one whose timestamp is read.
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t init(unsigned flags = hipEventDisableTiming) { return h ? hipSuccess : hipEventCreateWithFlags(&h, flags); }
};

// A lazily recorded mark: note() remembers where the producer ran and records nothing; order()
// records and waits only for a dependent on another stream.
class StreamMark {
public:
    StreamMark() = default;
    StreamMark(StreamMark &&o) noexcept { *this = static_cast<StreamMark &&>(o); }
    StreamMark &operator=(StreamMark &&o) noexcept
    {
        ev_ = static_cast<Event &&>(o.ev_);
        stream_ = o.stream_;
        noted_ = o.noted_;
        o.noted_ = false;
        return *this;
    }

    hipError_t init() { return ev_.init(); }
    void note(hipStream_t s) { stream_ = s; noted_ = true; }
    void clear() { noted_ = false; }   // the producer's work no longer matters to anyone
    bool noted() const { return noted_; }
    hipStream_t stream() const { return stream_; }   // of the last note (nullptr before the first)

    // Would order() enqueue anything for a dependent whose stream order `covered_by` provides?
    bool crosses(hipStream_t covered_by) const { return noted_ && stream_ != covered_by; }

    // Makes `waiter` wait for the noted work, unless the mark was never noted or the work ran on
    // `covered_by` -- the stream whose own order already puts the dependent behind it.  That is
    // `waiter` itself, except for a side stream that is itself ordered after the caller's.
    hipError_t order(hipStream_t waiter) { return order(waiter, waiter); }
    hipError_t order(hipStream_t waiter, hipStream_t covered_by)
    {
        if (!crosses(covered_by)) return hipSuccess;
        hipError_t e = ev_.init();
        if (e == hipSuccess) e = hipEventRecord(ev_.h, stream_);
        if (e == hipSuccess) e = hipStreamWaitEvent(waiter, ev_.h, 0);
        return e;
    }

private:
    Event ev_;
    hipStream_t stream_ = nullptr;
    bool noted_ = false;
};

// An eagerly recorded event: record() records now; wait() and query() concern only an event that
// was ever recorded (a moved-from one has none, so it was not).
class DoneEvent {
public:
    hipError_t init() { return ev_.init(); }
    hipError_t record(hipStream_t s)
    {
        hipError_t e = ev_.init();
        if (e == hipSuccess) e = hipEventRecord(ev_.h, s);
        if (e == hipSuccess) recorded_ = true;
        return e;
    }
    hipError_t wait(hipStream_t s) const { return recorded() ? hipStreamWaitEvent(s, ev_.h, 0) : hipSuccess; }
    // hipSuccess: done (or never recorded); hipErrorNotReady: still pending
    hipError_t query() const { return recorded() ? hipEventQuery(ev_.h) : hipSuccess; }
    bool recorded() const { return recorded_ && ev_.h; }
    hipEvent_t event() const { return ev_.h; }   // for a host-side wait

private:
    Event ev_;
    bool recorded_ = false;
};

}  // namespace dpwa
