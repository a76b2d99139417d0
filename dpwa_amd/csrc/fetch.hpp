// fetch.hpp -- the fetch in flight of one learner (learner.cpp): where the snapshot it is about to
// average with comes from, which buffer it lands in, who waits for it, and when that buffer may be
// refilled; and the rescue lanes a re-selected pull goes to.  Which peer and slot, the order after
// the peer's publish and the device belong to the learner; everything here is handed its streams.
// Host only; tests/native/fetch_check.cpp pins the exact calls.
#pragma once

#include <utility>

#include "kernels.hpp"
#include "order.hpp"

namespace dpwa {

// The host's monotonic clock (learner.cpp; a check defines its own).
int64_t now_ns();

// A rescue lane: where a fetch re-selected after a timed-out pull goes (conn.py:304-309) -- a
// buffer and a stream of the greatest priority (a hardware queue no stalled normal-priority stream
// shares), so no stalled pull ahead of it can hold it up.  Lanes are made at first use, up to
// kMaxRescueLanes, only while the device keeps kRescueReserve free beyond the new buffer and all
// lanes together stay within 1/kRescueShare of the device's memory (7B bf16: two 14 GB lanes on a
// 288 GB GPU); an allocation that fails caps the count where it is instead of failing the round.
// Lanes beyond the first kKeepRescueLanes are given back once they have been idle for
// kLaneIdleRounds fetch rounds (trim), so a burst of stalled pulls does not hold HBM outside
// PyTorch's allocator for the rest of the process.
constexpr int kMaxRescueLanes = 8;
constexpr int kKeepRescueLanes = 2;
constexpr uint64_t kLaneIdleRounds = 8;
constexpr size_t kRescueShare = 8;
constexpr size_t kRescueReserve = (size_t)1 << 30;
// Fetch::state: a backlog on the caller's stream longer than this no longer defers the timeout (a
// stream that never reaches update_send is stuck, not slow); a probe waits at most kProbeWaitUs
constexpr int64_t kMaxBacklogMs = 60000;
constexpr int64_t kProbeWaitUs = 2000;

struct RescueLane {
    DevBuf buf;
    Stream stream;
    DoneEvent landed;                   // its last pull landed (recorded: a pull was issued into it)
    DoneEvent done;                     // the last reader of its buffer is done
    uint64_t last_round = 0;            // fetch round of its last pull
};

// The lanes, allocated at first use: a lane whose pull has not landed stays taken and the next
// re-selected pull takes another, as TxThread keeps re-selecting.
class RescueLanes {
public:
    // A free lane: one whose last pull landed (or none issued), else a new one when fewer than cap()
    // exist; *lane = -1 when none is free and none can be made.  A new lane is built in a local and
    // counted only once every resource exists.  Running short of memory (or an allocation failing)
    // is not an error of the round: the count is capped where it is and the caller waits for a lane
    // to land.
    int acquire(size_t slot_stride, int *lane)
    {
        *lane = -1;
        for (int j = 0; j < count_; ++j) {
            const hipError_t e = lane_[j].landed.query();
            if (e == hipSuccess) {
                *lane = j;
                return DPWA_OK;
            }
            if (e != hipErrorNotReady) return set_error(DPWA_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(e));
        }
        if (count_ >= cap_) return DPWA_OK;
        size_t free_b = 0, total_b = 0;
        RescueLane r;
        int least = 0, greatest = 0;
        hipError_t e = hipMemGetInfo(&free_b, &total_b);
        if (e == hipSuccess && (free_b < slot_stride + kRescueReserve ||
                                (size_t)(count_ + 1) * slot_stride > total_b / kRescueShare))
            e = hipErrorOutOfMemory;   // the budget: nothing is asked for
        if (e == hipSuccess) e = r.buf.alloc(slot_stride);
        if (e == hipSuccess) e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (e == hipSuccess) e = r.stream.create(greatest);
        if (e == hipSuccess) e = r.landed.init();
        if (e == hipSuccess) e = r.done.init();
        if (e != hipSuccess) {                // `r` gives back what it made
            (void)hipGetLastError();          // clear the sticky error: the round goes on without a new lane
            cap_ = count_;
            return DPWA_OK;
        }
        lane_[count_] = std::move(r);
        *lane = count_++;
        return DPWA_OK;
    }

    // Gives back the lanes beyond the first kKeepRescueLanes, last first, once idle for
    // kLaneIdleRounds fetch rounds: their pull landed and the last reader of their buffer is done
    // (event queries, no wait); never the lane the fetch source lies in.  Called at a round's first
    // pull, the normal path, where it costs one comparison.
    void trim(uint64_t fetch_rounds, int source_lane)
    {
        if (count_ <= kKeepRescueLanes) return;
        while (count_ > kKeepRescueLanes) {
            RescueLane &r = lane_[count_ - 1];
            if (fetch_rounds - r.last_round < kLaneIdleRounds || source_lane == count_ - 1) return;
            if (r.landed.query() != hipSuccess || r.done.query() != hipSuccess) break;
            r = RescueLane();
            count_--;
        }
        (void)hipGetLastError();   // a not-ready query leaves no error behind
    }

    void set_cap(int cap) { cap_ = cap < count_ ? count_ : cap > kMaxRescueLanes ? kMaxRescueLanes : cap; }
    int count() const { return count_; }
    int cap() const { return cap_; }   // lowered when a lane's allocation fails
    RescueLane &operator[](int j) { return lane_[j]; }

private:
    RescueLane lane_[kMaxRescueLanes];
    int count_ = 0;
    int cap_ = kMaxRescueLanes;
};

// How one snapshot moves: `bytes` from the peer's slot `from` into a slot-sized buffer, by the copy
// engine or the pull kernel (dpwa_learner_set_pull).
struct Pull {
    const char *from;
    size_t bytes;
    int mode, blocks;
    bool cross_device;
    // on `stream`, between the events of the fetch-timing pair `ft` when there is one
    int into(char *dst, hipStream_t stream, const LaunchTiming *ft = nullptr) const
    {
        if (ft) HIP_TRY(hipEventRecord(ft->start, stream));
        if (mode == DPWA_PULL_KERNEL)
            HIP_TRY(launch_pull(dst, from, (int64_t)bytes, blocks, cross_device, stream));
        else
            HIP_TRY(hipMemcpyAsync(dst, from, bytes, hipMemcpyDefault, stream));
        if (ft) HIP_TRY(hipEventRecord(ft->stop, stream));
        return DPWA_OK;
    }
};

// The snapshot a fetch reads.
struct Source {
    enum Kind { InPlace, Staging, Lane };   // the buffer `ptr` lies in: a peer's slot, staging 0 | 1, rescue lane j
    const char *ptr = nullptr;              // header of the snapshot to average with
    Kind kind = InPlace;
    int index = 0;                          // of the staging buffer or the lane
    bool copied = false;                    // a copy, which `landed` covers
    const void *owner = nullptr;            // local peer whose slot is being read (reader tracking); null: none
    int slot = -1;
    int lane() const { return kind == Lane ? index : -1; }
};

class Fetch {
public:
    // What a learner holds from its creation on: staging buffer 0 and the events (ev_issue is
    // timed: its timestamp is the fetch deadline's start).  `side`: the learner's side stream.
    hipError_t init(size_t slot_stride, hipStream_t side)
    {
        slot_stride_ = slot_stride;
        side_ = side;
        hipError_t e = staging_[0].alloc(slot_stride);
        if (e == hipSuccess) e = ev_issue_.init(hipEventDefault);
        if (e == hipSuccess) e = landed_.init();
        if (e == hipSuccess) e = consumed_.init();
        if (e == hipSuccess) e = stage_done_[0].init();
        if (e == hipSuccess) e = stage_done_[1].init();
        return e;
    }

    // The round's phase: no fetch -> fetched -> factored.
    bool fetched() const { return phase_ != Phase::None; }
    bool factored() const { return phase_ == Phase::Factored; }
    hipError_t factored_on(hipStream_t s)   // the factor, launched on `s`, has read the header
    {
        const hipError_t e = note_consumed(s);
        if (e == hipSuccess) phase_ = Phase::Factored;
        return e;
    }
    void finish()   // averaged or cancelled (the source's buffer stays known: trim spares its lane)
    {
        phase_ = Phase::None;
        src_.ptr = nullptr;
    }

    const Source &source() const { return src_; }
    // Is an unfinished fetch reading local peer `owner`'s slot `slot`?
    bool reads(const void *owner, int slot) const { return fetched() && src_.owner == owner && src_.slot == slot; }
    // Is there a copy to wait for?  (An in-place source has none: stream order covers it.)
    bool awaits_copy() const { return fetched() && src_.copied; }
    char *staging() const { return staging_[0].ptr(); }
    RescueLanes &lanes() { return lanes_; }
    hipStream_t stream() const { return stream_ ? stream_ : side_; }   // the fetch in flight moves its bytes on it
    // Where this learner finished reading its last source: whoever rewrites that orders after it.
    StreamMark &consumed_mark() { return consumed_; }

    // ------------------------------------------------------------ the four pulls (dpwa_learner_fetch)
    // `s`: the caller's stream at update_send; `owner`, `slot`: the local peer's slot read (else null, -1).
    // A second pull before the lerp keeps the factor computed, as it always has.

    // Re-selected after a timed-out pull: a free lane (its own stream and buffer), ordered after
    // `s` (unless the snapshot is a published one: `ordered` false) and after the last reader of
    // the lane's buffer.  Not timed.
    int pull_rescue(const Pull &p, hipStream_t s, bool ordered, const void *owner, int slot)
    {
        begin();
        int j = -1;
        if (int rc = lanes_.acquire(slot_stride_, &j)) return rc;
        if (j < 0) return set_error(DPWA_ERR_STATE, "dpwa_learner_fetch: all %d rescue lanes are still pulling", lanes_.count());
        RescueLane &r = lanes_[j];
        if (ordered) {
            HIP_TRY(issue_after(s, r.stream.h));
            issue_evented_ = true;
        }
        HIP_TRY(r.done.wait(r.stream.h));
        if (int rc = p.into(r.buf.ptr(), r.stream.h)) return rc;
        HIP_TRY(r.landed.record(r.stream.h));
        HIP_TRY(landed_.record(r.stream.h));
        r.last_round = rounds_;
        stream_ = r.stream.h;
        pulled(Source{r.buf.ptr(), Source::Lane, j, true, owner, slot});
        return DPWA_OK;
    }

    // A local peer's slot on the same device, read where it is: no call; stream order covers the rest.
    void read_in_place(const char *peer_slot, const void *owner, int slot)
    {
        begin_round();
        pulled(Source{peer_slot, Source::InPlace, 0, false, owner, slot});
    }

    // A published snapshot (DPWA_FETCH_PUBLISHED: the gossip board) is not ordered after the caller's
    // stream: pulls alternate between two staging buffers and each waits only for the average that
    // last read its buffer (stage_done), so a pull starts at update_send instead of after the
    // caller's queued work, and a peer's read mark is released sooner.
    int pull_published(const Pull &p, const LaunchTiming *ft, const void *owner, int slot)
    {
        begin_round();
        if (!staging_[1].ptr()) {   // allocated at the first such fetch
            HIP_TRY(staging_[1].alloc(slot_stride_));
            HIP_TRY(hipMemsetAsync(staging_[1].ptr(), 0, DPWA_SLOT_PAYLOAD_OFFSET, side_));
        }
        const int b = stage_next_;
        stage_next_ ^= 1;
        // WAR: the average that last read this buffer; nothing else on the caller's stream
        HIP_TRY(stage_done_[b].wait(side_));
        if (int rc = p.into(staging_[b].ptr(), side_, ft)) return rc;
        HIP_TRY(landed_.record(side_));
        pulled(Source{staging_[b].ptr(), Source::Staging, b, true, owner, slot});
        return DPWA_OK;
    }

    // Into staging 0 on the side stream, which runs on from where `s` is now.
    int pull_ordered(const Pull &p, const LaunchTiming *ft, hipStream_t s, const void *owner, int slot)
    {
        begin_round();
        HIP_TRY(stage_done_[0].wait(side_));
        HIP_TRY(issue_after(s, side_));
        issue_evented_ = true;
        // WAR on our own staging buffer: the previous average must have consumed it (the side
        // stream waits, and now follows `s`, which covers a consumption on itself)
        HIP_TRY(consumed_.order(side_, s));
        if (int rc = p.into(staging_[0].ptr(), side_, ft)) return rc;
        HIP_TRY(landed_.record(side_));
        pulled(Source{staging_[0].ptr(), Source::Staging, 0, true, owner, slot});
        return DPWA_OK;
    }

    // ------------------------------------------------------------ arrivals someone else writes
    // A snapshot put into staging 0 on the side stream (a host copy, the relay's second phase):
    // staging_writable*, the write, landed_on_side, arrived_in_staging.  (A relay's deferred second
    // phase arrives before its gather; the gather then goes the same way without arriving again.)

    // The side stream waits for the last reader of staging 0 (every consumer records stage_done) ...
    hipError_t staging_writable() const { return stage_done_[0].wait(side_); }
    // ... and, first, for a consumption anywhere (covered_by = nullptr: a consumption on the
    // default stream is indistinguishable from "never")
    hipError_t staging_writable_after_consumption()
    {
        const hipError_t e = consumed_.order(side_, nullptr);
        return e == hipSuccess ? staging_writable() : e;
    }
    // The side stream runs on from the point `s` has reached (the relay's first phase).
    hipError_t side_after(hipStream_t s) { return issue_after(s, side_); }
    hipError_t landed_on_side() { return landed_.record(side_); }
    hipError_t host_wait_landed() const { return hipEventSynchronize(landed_.event()); }   // the host's bytes have been taken
    void arrived_in_staging()   // a new fetch, whatever the phase was
    {
        src_ = Source{staging_[0].ptr(), Source::Staging, 0, true, nullptr, -1};
        phase_ = Phase::Fetched;
    }

    // ------------------------------------------------------------ the consumer's side
    // `s` reads the source after it landed: no call for an in-place source (TxThread.fetch_wait).
    hipError_t wait_landed(hipStream_t s) const { return awaits_copy() ? landed_.wait(s) : hipSuccess; }

    // Everything enqueued on `s` so far has read the fetch source: a staging buffer or lane may be
    // refilled once `s` gets here (recorded now: refills run elsewhere); so may the source itself.
    hipError_t note_consumed(hipStream_t s)
    {
        hipError_t e = hipSuccess;
        if (src_.copied && src_.kind == Source::Lane) e = lanes_[src_.index].done.record(s);
        if (src_.copied && src_.kind == Source::Staging) e = stage_done_[src_.index].record(s);
        if (e == hipSuccess) consumed_.note(s);
        return e;
    }
    // The relay's stripes were read where its first phase left them: no staging buffer was.
    void note_consumed_in_place(hipStream_t s) { consumed_.note(s); }

    // dpwa_learner_fetch_state: DPWA_FETCH_LANDED / _IN_FLIGHT / _TIMED_OUT, without blocking.
    int state(int64_t timeout_ms, bool relay_deferred, int *out)
    {
        *out = DPWA_FETCH_LANDED;
        if (!awaits_copy() || relay_deferred) return DPWA_OK;
        const hipError_t e = landed_.query();
        if (e == hipSuccess) return DPWA_OK;
        if (e != hipErrorNotReady) return set_error(DPWA_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(e));
        *out = DPWA_FETCH_IN_FLIGHT;
        if (timeout_ms < 0) return DPWA_OK;
        // The host's enqueue is an upper bound on how long the request has been out: within the
        // timeout by it, the pull is in time.  Past it, a pull ordered after the caller's stream
        // (ev_issue: a local peer's snapshot) is timed from when that stream reached update_send --
        // the reference's socket timeout bounds only the wait for the reply (conn.py:249), and work the
        // caller queued before update_send is not the peer's delay.
        const int64_t waited_ns = now_ns() - issue_ns_;
        if (waited_ns < timeout_ms * 1000000LL) return DPWA_OK;
        if (issue_evented_ && waited_ns < (timeout_ms + kMaxBacklogMs) * 1000000LL) {
            const hipError_t q = hipEventQuery(ev_issue_.h);
            if (q == hipErrorNotReady) return DPWA_OK;        // the request has not gone out yet
            if (q != hipSuccess) return set_error(DPWA_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(q));
            float ms = 0.f;
            if (probe_since(ev_issue_.h, &ms) == DPWA_OK && ms >= 0.f) {
                *out = ms >= (float)timeout_ms ? DPWA_FETCH_TIMED_OUT : DPWA_FETCH_IN_FLIGHT;
                return DPWA_OK;
            }
        }
        *out = DPWA_FETCH_TIMED_OUT;
        return DPWA_OK;
    }

private:
    enum class Phase { None, Fetched, Factored };
    struct Probe {   // state's clock (probe_since): a stream that only ever holds `ev`, a timing event
        Stream stream;
        Event ev;
    };

    void begin()   // any pull: its timeout clock starts, on the side stream until a lane takes it
    {
        issue_ns_ = now_ns();
        stream_ = side_;
        issue_evented_ = false;
    }
    void begin_round()   // a round's first pull: the lanes' idle clock moves on
    {
        begin();
        rounds_++;
        lanes_.trim(rounds_, src_.lane());
    }
    void pulled(const Source &src)
    {
        src_ = src;
        if (phase_ == Phase::None) phase_ = Phase::Fetched;
    }
    // `to` runs on from the point `s` has reached; state() reads ev_issue's time of reaching it
    hipError_t issue_after(hipStream_t s, hipStream_t to)
    {
        const hipError_t e = hipEventRecord(ev_issue_.h, s);
        return e == hipSuccess ? hipStreamWaitEvent(to, ev_issue_.h, 0) : e;
    }

    // Milliseconds since the (completed, timing) event `since`, on the device's clock: an event
    // recorded now on the probe stream -- a stream that holds nothing else -- and the two timestamps'
    // difference.  DPWA_ERR_STATE when the probe does not complete within kProbeWaitUs (its hardware
    // queue is held up by another stream mapped to it: no measurement).  The probe stream has the
    // normal priority: the greatest-priority hardware queues are left to the rescue lanes (streams are
    // dealt round-robin onto a few queues per priority, so a probe there would push a lane onto a
    // queue another lane already uses).
    int probe_since(hipEvent_t since, float *ms)
    {
        if (!probe_.stream.h) {   // made at the first probe
            Probe p;
            hipError_t e = p.stream.create();
            if (e == hipSuccess) e = p.ev.init(hipEventDefault);
            if (e != hipSuccess) return set_error(DPWA_ERR_HIP, "probe stream: %s", hipGetErrorString(e));
            probe_ = std::move(p);
        }
        const hipEvent_t ev_probe = probe_.ev.h;
        HIP_TRY(hipEventRecord(ev_probe, probe_.stream.h));
        const int64_t t0 = now_ns();
        for (;;) {
            const hipError_t q = hipEventQuery(ev_probe);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return set_error(DPWA_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(q));
            if (now_ns() - t0 > kProbeWaitUs * 1000) return set_error(DPWA_ERR_STATE, "probe held up");
        }
        HIP_TRY(hipEventElapsedTime(ms, since, ev_probe));
        return DPWA_OK;
    }

    size_t slot_stride_ = 0;
    hipStream_t side_ = nullptr;        // the learner's (not owned)
    DevBuf staging_[2];                 // 1 slot each; the second for published pulls
    DoneEvent stage_done_[2];           // the last reader of staging b is done
    int stage_next_ = 0;
    RescueLanes lanes_;
    Event ev_issue_;                    // fetch may start (recorded on the caller's stream); timed
    DoneEvent landed_;                  // fetch landed (recorded on the stream that moved it)
    StreamMark consumed_;               // this learner finished reading its fetch source
    Source src_;
    Phase phase_ = Phase::None;
    uint64_t rounds_ = 0;               // first (non-rescue) pulls issued: the lanes' idle clock
    int64_t issue_ns_ = 0;              // host time the fetch in flight was issued (its timeout clock)
    // the fetch in flight waits for ev_issue (the caller's stream at update_send): its deadline runs
    // from when that point is reached, not from the host's enqueue (state)
    bool issue_evented_ = false;
    Probe probe_;
    hipStream_t stream_ = nullptr;      // stream the fetch in flight moves its bytes on (not owned)
};

}  // namespace dpwa
