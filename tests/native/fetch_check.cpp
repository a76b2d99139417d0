// fetch_check.cpp -- dpwa_amd/csrc/fetch.hpp (Fetch, RescueLanes) against recording stand-ins of every
// HIP entry point it and order.hpp call, of launch_pull and of set_error.  No HIP runtime is linked: the
// calls land in the log below, the host clock is g_now, and every case asserts the exact log.  Every
// stream, event and allocation is made here, and destroying one twice (or one never made) ends the
// program; at the end none may be left.  Built with AddressSanitizer + UBSan by
// tests/test_native_sanitizers.py.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../dpwa_amd/csrc/fetch.hpp"

using namespace dpwa;

namespace {

// op: EC / ED event create (n: flags) / destroy; R record (a event, b stream); W stream wait (a event, b
// stream); Q query; Y host wait; T elapsed (a since, b until); SC stream create (a stream, n: priority, -1
// none) / SD destroy; PR priority range; MI memory query; MA malloc (a allocation, n bytes) / MF free; MS
// memset (a allocation, b stream, n bytes); CP copy engine / LP pull kernel (a destination's allocation, b
// stream, n bytes); GE hipGetLastError.
struct Call {
    std::string op;
    uintptr_t a, b;
    int64_t n;
    bool operator==(const Call &o) const { return op == o.op && a == o.a && b == o.b && n == o.n; }
};

std::vector<Call> g_log;
std::string g_error;
int g_failures = 0;

// handles: events 1, 2, ...; streams kMade + 1, ...; allocations 1, 2, ... (host memory, so that ASan sees them)
constexpr uintptr_t kMade = 0x1000;
uintptr_t g_next_event = 1, g_next_stream = kMade + 1;
std::vector<int> g_event_alive{0}, g_stream_alive{0};
std::vector<void *> g_alloc{nullptr};       // by allocation number; null once freed
std::set<uintptr_t> g_pending;              // events whose query says hipErrorNotReady
int64_t g_now = 0;                          // the host clock, ns
int64_t g_pending_query_ns = 0;             // ... which every not-ready query moves on by this much
float g_elapsed_ms = 0.f;
size_t g_free_b = 0, g_total_b = 0;
bool g_fail_malloc = false, g_fail_stream = false;
const void *const kFrom = (const void *)0xF000;   // the peer's slot: never dereferenced

uintptr_t id(hipEvent_t e) { return (uintptr_t)e; }
uintptr_t id(hipStream_t s) { return (uintptr_t)s; }
hipStream_t stream(uintptr_t k) { return (hipStream_t)k; }

void must_be_alive(const std::vector<int> &alive, uintptr_t k, const char *what)
{
    if (k == 0 || k >= alive.size() || alive[k] != 1) {
        fprintf(stderr, "%s on handle %zu, which is not alive\n", what, (size_t)k);
        abort();
    }
}
void must_be_event(hipEvent_t e, const char *what) { must_be_alive(g_event_alive, id(e), what); }
void must_be_stream(hipStream_t s, const char *what)   // a stream made here; the caller's are plain numbers
{
    if (id(s) > kMade) must_be_alive(g_stream_alive, id(s) - kMade, what);
}
uintptr_t alloc_of(const void *p)
{
    for (size_t k = 1; k < g_alloc.size(); ++k)
        if (g_alloc[k] == p) return k;
    fprintf(stderr, "%p is no live allocation\n", p);
    abort();
}

std::string show(const std::vector<Call> &v)
{
    std::string s;
    for (const Call &c : v) {
        char buf[96];
        snprintf(buf, sizeof(buf), "%s(%zx,%zx,%lld) ", c.op.c_str(), (size_t)c.a, (size_t)c.b, (long long)c.n);
        s += buf;
    }
    return s.empty() ? "(no calls)" : s;
}

void expect(const char *name, const std::vector<Call> &want)
{
    if (!(g_log == want)) {
        fprintf(stderr, "FAIL %s\n  want %s\n  got  %s\n", name, show(want).c_str(), show(g_log).c_str());
        ++g_failures;
    }
    g_log.clear();
}

void check(const char *name, bool ok)
{
    if (!ok) {
        fprintf(stderr, "FAIL %s (last error: %s)\n", name, g_error.c_str());
        ++g_failures;
    }
}

}  // namespace

// ---------------------------------------------------------------- stand-ins
namespace dpwa {

int set_error(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}

int64_t now_ns() { return g_now; }

hipError_t launch_pull(void *dst, const void *src, int64_t nbytes, int max_blocks, bool remote, hipStream_t s)
{
    if (src != kFrom || max_blocks != 7 || !remote) abort();
    must_be_stream(s, "launch_pull");
    g_log.push_back({"LP", alloc_of(dst), id(s), nbytes});
    return hipSuccess;
}

}  // namespace dpwa

extern "C" {

hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned flags)
{
    const uintptr_t k = g_next_event++;
    g_event_alive.resize(k + 1, 0);
    g_event_alive[k] = 1;
    *event = (hipEvent_t)k;
    g_log.push_back({"EC", k, 0, (int64_t)flags});
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event)
{
    must_be_event(event, "hipEventDestroy");   // a second destroy of one event ends the program
    g_event_alive[id(event)] = 0;
    g_log.push_back({"ED", id(event), 0, 0});
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t s)
{
    must_be_event(event, "hipEventRecord");
    must_be_stream(s, "hipEventRecord");
    g_log.push_back({"R", id(event), id(s), 0});
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t event, unsigned)
{
    must_be_event(event, "hipStreamWaitEvent");
    must_be_stream(s, "hipStreamWaitEvent");
    g_log.push_back({"W", id(event), id(s), 0});
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t event)
{
    must_be_event(event, "hipEventQuery");
    g_log.push_back({"Q", id(event), 0, 0});
    if (!g_pending.count(id(event))) return hipSuccess;
    g_now += g_pending_query_ns;
    return hipErrorNotReady;
}
hipError_t hipEventSynchronize(hipEvent_t event)
{
    must_be_event(event, "hipEventSynchronize");
    g_log.push_back({"Y", id(event), 0, 0});
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t start, hipEvent_t stop)
{
    must_be_event(start, "hipEventElapsedTime");
    must_be_event(stop, "hipEventElapsedTime");
    g_log.push_back({"T", id(start), id(stop), 0});
    *ms = g_elapsed_ms;
    return hipSuccess;
}

static hipError_t make_stream(hipStream_t *s, unsigned flags, int priority)
{
    if (flags != hipStreamNonBlocking) abort();
    if (g_fail_stream) {
        g_log.push_back({"SC", 0, 0, priority});
        return hipErrorOutOfMemory;
    }
    const uintptr_t k = g_next_stream++;
    g_stream_alive.resize(k - kMade + 1, 0);
    g_stream_alive[k - kMade] = 1;
    *s = stream(k);
    g_log.push_back({"SC", k, 0, priority});
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags) { return make_stream(s, flags, -1); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int priority) { return make_stream(s, flags, priority); }
hipError_t hipStreamDestroy(hipStream_t s)
{
    if (id(s) <= kMade) abort();
    must_be_stream(s, "hipStreamDestroy");
    g_stream_alive[id(s) - kMade] = 0;
    g_log.push_back({"SD", id(s), 0, 0});
    return hipSuccess;
}
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest)
{
    *least = 0;
    *greatest = 3;   // (not HIP's own numbers: only that the greatest is the one used)
    g_log.push_back({"PR", 0, 0, 0});
    return hipSuccess;
}

hipError_t hipMemGetInfo(size_t *free_b, size_t *total_b)
{
    *free_b = g_free_b;
    *total_b = g_total_b;
    g_log.push_back({"MI", 0, 0, 0});
    return hipSuccess;
}
hipError_t hipMalloc(void **ptr, size_t bytes)
{
    if (g_fail_malloc) {
        g_log.push_back({"MA", 0, 0, (int64_t)bytes});
        return hipErrorOutOfMemory;
    }
    if (posix_memalign(ptr, 256, 64)) abort();   // nothing is ever written: 64 bytes stand for `bytes`
    g_alloc.push_back(*ptr);
    g_log.push_back({"MA", g_alloc.size() - 1, 0, (int64_t)bytes});
    return hipSuccess;
}
hipError_t hipFree(void *ptr)
{
    const uintptr_t k = alloc_of(ptr);   // a second free of one allocation ends the program
    g_alloc[k] = nullptr;
    free(ptr);
    g_log.push_back({"MF", k, 0, 0});
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t s)
{
    if (value != 0) abort();
    g_log.push_back({"MS", alloc_of(dst), id(s), (int64_t)bytes});
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s)
{
    if (src != kFrom || kind != hipMemcpyDefault) abort();
    must_be_stream(s, "hipMemcpyAsync");
    g_log.push_back({"CP", alloc_of(dst), id(s), (int64_t)bytes});
    return hipSuccess;
}
hipError_t hipGetLastError(void)
{
    g_log.push_back({"GE", 0, 0, 0});
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t) { return "stand-in error"; }

}  // extern "C"

namespace {

const hipStream_t A = stream(0xA0), B = stream(0xB0), SIDE = stream(0x51);   // the caller's, a third, the side stream
constexpr size_t kStride = 4096 + 8192;              // [header | pad | payload of 4,001 bytes, to 4 KiB]
constexpr int64_t kBytes = 4096 + 4016;              // 4096 + round_up(4001, 16), as learner.cpp hands it over
constexpr unsigned kNoTiming = hipEventDisableTiming;
const Pull kCopy{(const char *)kFrom, (size_t)kBytes, DPWA_PULL_COPY_ENGINE, 7, true};
const Pull kKernel{(const char *)kFrom, (size_t)kBytes, DPWA_PULL_KERNEL, 7, true};
constexpr int64_t kMs = 1000000;

// A fetch as dpwa_learner_create makes it: staging 0 is allocation m, its events issue, landed, consumed,
// done0, done1 (ev_issue alone is timed).
struct Rig {
    Fetch f;
    uintptr_t m, issue, landed, consumed, done0, done1;
    Rig()
    {
        m = g_alloc.size();
        issue = g_next_event;
        landed = issue + 1, consumed = issue + 2, done0 = issue + 3, done1 = issue + 4;
        check("init", f.init(kStride, SIDE) == hipSuccess);
        expect("init: staging 0, then the five events, ev_issue timed",
               {{"MA", m, 0, (int64_t)kStride}, {"EC", issue, 0, hipEventDefault}, {"EC", landed, 0, kNoTiming},
                {"EC", consumed, 0, kNoTiming}, {"EC", done0, 0, kNoTiming}, {"EC", done1, 0, kNoTiming}});
        check("init: no fetch", !f.fetched() && !f.factored() && !f.awaits_copy() && f.stream() == SIDE &&
                                    f.staging() == g_alloc[m] && f.source().ptr == nullptr);
    }
};

void memory_plenty()
{
    g_free_b = (size_t)64 << 30;
    g_total_b = (size_t)256 << 30;
}

void ordered_pull()
{
    Rig r;
    Fetch &f = r.f;
    int owner = 0;
    check("ordered 1", f.pull_ordered(kCopy, nullptr, A, &owner, 1) == DPWA_OK);
    expect("ordered, first round: nothing was ever recorded, so no wait",
           {{"R", r.issue, id(A), 0}, {"W", r.issue, id(SIDE), 0}, {"CP", r.m, id(SIDE), kBytes}, {"R", r.landed, id(SIDE), 0}});
    check("ordered 1: source", f.fetched() && !f.factored() && f.awaits_copy() && f.source().kind == Source::Staging &&
                                   f.source().index == 0 && f.source().ptr == f.staging() && f.stream() == SIDE);
    check("reads", f.reads(&owner, 1) && !f.reads(&owner, 0) && !f.reads(&r, 1));
    check("landed", f.wait_landed(A) == hipSuccess && f.note_consumed(A) == hipSuccess);
    expect("the consumer waits for landed and records staging 0's done, no other", {{"W", r.landed, id(A), 0}, {"R", r.done0, id(A), 0}});
    f.finish();
    check("finish", !f.fetched() && f.source().ptr == nullptr && !f.reads(&owner, 1) && f.wait_landed(A) == hipSuccess);
    expect("finish, and a wait with no fetch, make no call", {});

    check("ordered 2", f.pull_ordered(kCopy, nullptr, A, nullptr, -1) == DPWA_OK);
    expect("after a consumption on the caller's stream: a wait on done0 and no consumed event",
           {{"W", r.done0, id(SIDE), 0}, {"R", r.issue, id(A), 0}, {"W", r.issue, id(SIDE), 0}, {"CP", r.m, id(SIDE), kBytes},
            {"R", r.landed, id(SIDE), 0}});
    check("consumed on B", f.note_consumed(B) == hipSuccess);
    f.finish();
    g_log.clear();
    hipEvent_t t0, t1;   // a fetch-timing pair
    (void)hipEventCreateWithFlags(&t0, hipEventDefault);
    (void)hipEventCreateWithFlags(&t1, hipEventDefault);
    const LaunchTiming ft{t0, t1};
    g_log.clear();
    check("ordered 3", f.pull_ordered(kKernel, &ft, A, nullptr, -1) == DPWA_OK);
    expect("after a consumption on a third stream: one record there, one wait on the side stream; the pair around the pull kernel",
           {{"W", r.done0, id(SIDE), 0}, {"R", r.issue, id(A), 0}, {"W", r.issue, id(SIDE), 0}, {"R", r.consumed, id(B), 0},
            {"W", r.consumed, id(SIDE), 0}, {"R", id(t0), id(SIDE), 0}, {"LP", r.m, id(SIDE), kBytes}, {"R", id(t1), id(SIDE), 0},
            {"R", r.landed, id(SIDE), 0}});
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    g_log.clear();
}

void published_pull()
{
    Rig r;
    Fetch &f = r.f;
    const uintptr_t m1 = g_alloc.size();
    check("published 1", f.pull_published(kCopy, nullptr, nullptr, -1) == DPWA_OK);
    expect("published, first use: the second buffer, its header cleared on the side stream; buffer 0",
           {{"MA", m1, 0, (int64_t)kStride}, {"MS", m1, id(SIDE), 4096}, {"CP", r.m, id(SIDE), kBytes}, {"R", r.landed, id(SIDE), 0}});
    check("published 1: source", f.source().kind == Source::Staging && f.source().index == 0 && f.stream() == SIDE);
    g_pending = {r.landed};
    g_now = 1000 * kMs;   // far past any timeout
    int st = -1;
    check("state", f.state(10, false, &st) == DPWA_OK && st == DPWA_FETCH_TIMED_OUT);
    expect("ev_issue was never recorded: past the timeout state() never probes", {{"Q", r.landed, 0, 0}});
    g_pending.clear();
    g_now = 0;
    check("consume 0", f.note_consumed(A) == hipSuccess);
    expect("Staging{0} records done0, no other", {{"R", r.done0, id(A), 0}});
    f.finish();
    check("published 2", f.pull_published(kCopy, nullptr, nullptr, -1) == DPWA_OK && f.source().index == 1 &&
                             f.source().ptr == g_alloc[m1]);
    expect("buffer 1, whose done was never recorded", {{"CP", m1, id(SIDE), kBytes}, {"R", r.landed, id(SIDE), 0}});
    check("consume 1", f.note_consumed(A) == hipSuccess);
    expect("Staging{1} records done1, no other", {{"R", r.done1, id(A), 0}});
    f.finish();
    check("published 3", f.pull_published(kCopy, nullptr, nullptr, -1) == DPWA_OK && f.source().index == 0);
    expect("buffer 0 again: it waits for its own done only", {{"W", r.done0, id(SIDE), 0}, {"CP", r.m, id(SIDE), kBytes}, {"R", r.landed, id(SIDE), 0}});
    f.finish();
    check("published 4", f.pull_published(kCopy, nullptr, nullptr, -1) == DPWA_OK && f.source().index == 1);
    expect("buffer 1 again", {{"W", r.done1, id(SIDE), 0}, {"CP", m1, id(SIDE), kBytes}, {"R", r.landed, id(SIDE), 0}});
}

void in_place()
{
    Rig r;
    Fetch &f = r.f;
    int owner = 0, st = -1;
    f.read_in_place((const char *)kFrom, &owner, 0);
    check("in place", f.fetched() && !f.awaits_copy() && f.source().kind == Source::InPlace && f.source().ptr == kFrom &&
                          f.reads(&owner, 0));
    check("in place: landed", f.wait_landed(A) == hipSuccess && f.state(0, false, &st) == DPWA_OK && st == DPWA_FETCH_LANDED);
    check("in place: consumed", f.note_consumed(A) == hipSuccess && f.consumed_mark().noted() && f.consumed_mark().stream() == A);
    expect("an in-place read makes no HIP call at all", {});
}

void rescue_pull()
{
    Rig r;
    Fetch &f = r.f;
    memory_plenty();
    const uintptr_t m0 = g_alloc.size(), s0 = g_next_stream, l0 = g_next_event, d0 = l0 + 1;
    check("rescue 1", f.pull_rescue(kCopy, A, true, nullptr, -1) == DPWA_OK);
    expect("a new lane: memory query, buffer, priority range, a stream of the greatest priority, two events; an untimed pull",
           {{"MI", 0, 0, 0}, {"MA", m0, 0, (int64_t)kStride}, {"PR", 0, 0, 0}, {"SC", s0, 0, 3}, {"EC", l0, 0, kNoTiming},
            {"EC", d0, 0, kNoTiming}, {"R", r.issue, id(A), 0}, {"W", r.issue, s0, 0}, {"CP", m0, s0, kBytes}, {"R", l0, s0, 0},
            {"R", r.landed, s0, 0}});
    check("rescue 1: source", f.source().kind == Source::Lane && f.source().lane() == 0 && f.stream() == stream(s0) &&
                                  f.lanes().count() == 1);
    check("consume lane 0", f.note_consumed(A) == hipSuccess);
    expect("Lane{0} records its own done, no other", {{"R", d0, id(A), 0}});

    g_pending = {l0};
    const uintptr_t m1 = g_alloc.size(), s1 = g_next_stream, l1 = g_next_event, d1 = l1 + 1;
    check("rescue 2", f.pull_rescue(kCopy, A, false, nullptr, -1) == DPWA_OK && f.source().lane() == 1);
    expect("lane 0 still pulling: lane 1 is made; a published snapshot's pull records no ev_issue",
           {{"Q", l0, 0, 0}, {"MI", 0, 0, 0}, {"MA", m1, 0, (int64_t)kStride}, {"PR", 0, 0, 0}, {"SC", s1, 0, 3},
            {"EC", l1, 0, kNoTiming}, {"EC", d1, 0, kNoTiming}, {"CP", m1, s1, kBytes}, {"R", l1, s1, 0}, {"R", r.landed, s1, 0}});
    g_pending = {l1, r.landed};
    g_now = 1000 * kMs;
    int st = -1;
    check("rescue 2: state", f.state(10, false, &st) == DPWA_OK && st == DPWA_FETCH_TIMED_OUT);
    expect("... and so is not probed", {{"Q", r.landed, 0, 0}});
    g_now = 0;

    check("rescue 3", f.pull_rescue(kCopy, A, true, nullptr, -1) == DPWA_OK && f.source().lane() == 0 && f.stream() == stream(s0));
    expect("lane 0 landed: it is taken again, and its stream waits for its done",
           {{"Q", l0, 0, 0}, {"R", r.issue, id(A), 0}, {"W", r.issue, s0, 0}, {"W", d0, s0, 0}, {"CP", m0, s0, kBytes},
            {"R", l0, s0, 0}, {"R", r.landed, s0, 0}});

    g_pending = {l0, l1};
    f.lanes().set_cap(2);
    check("rescue 4", f.pull_rescue(kCopy, A, true, nullptr, -1) == DPWA_ERR_STATE &&
                          g_error == "dpwa_learner_fetch: all 2 rescue lanes are still pulling");
    expect("every lane pulling at the cap: two queries, nothing allocated", {{"Q", l0, 0, 0}, {"Q", l1, 0, 0}});
    int lane = 0;
    check("acquire at the cap", f.lanes().acquire(kStride, &lane) == DPWA_OK && lane == -1);
    g_pending.clear();
    g_log.clear();
}

// The pool STAYS capped once an allocation was refused or failed: set_cap alone raises it again.  This
// pins what the code does today, which ADVICE.md questions (a first lane refused by the share rule is
// never retried); changing it is a change of behaviour with a case of its own here.
void budget()
{
    int lane = 0;
    {
        RescueLanes p;
        memory_plenty();
        g_free_b = kStride + kRescueReserve - 1;
        check("reserve", p.acquire(kStride, &lane) == DPWA_OK && lane == -1 && p.cap() == 0 && p.count() == 0);
        expect("free memory one byte short of a slot and the reserve: no allocation", {{"MI", 0, 0, 0}, {"GE", 0, 0, 0}});
        memory_plenty();
        check("capped", p.acquire(kStride, &lane) == DPWA_OK && lane == -1);
        expect("capped for good: with memory back, not even a query", {});
    }
    {
        RescueLanes p;
        memory_plenty();
        g_total_b = kRescueShare * (kStride - 1);
        check("share", p.acquire(kStride, &lane) == DPWA_OK && lane == -1 && p.cap() == 0);
        expect("one lane one byte over the share of the device's memory: no allocation", {{"MI", 0, 0, 0}, {"GE", 0, 0, 0}});
        p.set_cap(kMaxRescueLanes);
        g_total_b = kRescueShare * kStride;   // exactly one lane's worth
        check("share, exactly", p.acquire(kStride, &lane) == DPWA_OK && lane == 0 && p.count() == 1);
        const uintptr_t l0 = g_next_event - 2;
        check("lane 0 pulling", p[0].landed.record(A) == hipSuccess);
        g_pending = {l0};
        g_log.clear();
        check("share, the second", p.acquire(kStride, &lane) == DPWA_OK && lane == -1 && p.cap() == 1 && p.count() == 1);
        expect("two lanes are over it: capped at the one", {{"Q", l0, 0, 0}, {"MI", 0, 0, 0}, {"GE", 0, 0, 0}});
        g_pending.clear();
    }
    g_log.clear();
    {
        RescueLanes p;
        memory_plenty();
        g_fail_malloc = true;
        check("malloc fails", p.acquire(kStride, &lane) == DPWA_OK && lane == -1 && p.cap() == 0);
        expect("a failing hipMalloc: the error is cleared, the count capped", {{"MI", 0, 0, 0}, {"MA", 0, 0, (int64_t)kStride}, {"GE", 0, 0, 0}});
        g_fail_malloc = false;
    }
    {
        RescueLanes p;
        g_fail_stream = true;
        const uintptr_t m = g_alloc.size();
        check("stream fails", p.acquire(kStride, &lane) == DPWA_OK && lane == -1 && p.cap() == 0 && p.count() == 0);
        expect("a stream that cannot be made after the buffer exists: the buffer is freed once",
               {{"MI", 0, 0, 0}, {"MA", m, 0, (int64_t)kStride}, {"PR", 0, 0, 0}, {"SC", 0, 0, 3}, {"GE", 0, 0, 0}, {"MF", m, 0, 0}});
        g_fail_stream = false;
    }
    expect("... and by nobody else", {});
    {
        RescueLanes p;
        check("two lanes", p.acquire(kStride, &lane) == DPWA_OK && lane == 0 && p[0].landed.record(A) == hipSuccess);
        g_pending = {g_next_event - 2};
        check("two lanes", p.acquire(kStride, &lane) == DPWA_OK && lane == 1);
        g_pending.clear();
        p.set_cap(0);
        check("set_cap(0) with two lanes", p.cap() == 2 && p.count() == 2);
        p.set_cap(99);
        check("set_cap(99)", p.cap() == kMaxRescueLanes);
    }
    g_log.clear();
}

void trim()
{
    RescueLanes p;
    memory_plenty();
    uintptr_t m[4], s[4], landed[4], done[4];
    for (int j = 0; j < 4; ++j) {   // four lanes, each pulled into at fetch round 1 and read since
        int lane = -1;
        m[j] = g_alloc.size(), s[j] = g_next_stream, landed[j] = g_next_event, done[j] = landed[j] + 1;
        check("lane", p.acquire(kStride, &lane) == DPWA_OK && lane == j);
        check("lane used", p[j].landed.record(stream(s[j])) == hipSuccess && p[j].done.record(A) == hipSuccess);
        p[j].last_round = 1;
        g_pending.insert(landed[j]);
    }
    g_pending.clear();
    g_log.clear();
    p.trim(8, -1);
    expect("7 rounds idle: nothing is asked", {});
    p.trim(9, 3);
    expect("8 rounds idle, but the fetch source lies in it: nothing is asked", {});
    g_pending = {landed[3]};
    p.trim(9, -1);
    expect("its pull has not landed", {{"Q", landed[3], 0, 0}, {"GE", 0, 0, 0}});
    g_pending = {done[3]};
    p.trim(9, -1);
    expect("its last reader is not done", {{"Q", landed[3], 0, 0}, {"Q", done[3], 0, 0}, {"GE", 0, 0, 0}});
    check("none released yet", p.count() == 4);
    g_pending.clear();
    p.trim(9, -1);
    expect("lanes 3 and then 2 are released, each resource once; no lane below two",
           {{"Q", landed[3], 0, 0}, {"Q", done[3], 0, 0}, {"ED", done[3], 0, 0}, {"ED", landed[3], 0, 0}, {"SD", s[3], 0, 0},
            {"MF", m[3], 0, 0}, {"Q", landed[2], 0, 0}, {"Q", done[2], 0, 0}, {"ED", done[2], 0, 0}, {"ED", landed[2], 0, 0},
            {"SD", s[2], 0, 0}, {"MF", m[2], 0, 0}, {"GE", 0, 0, 0}});
    p.trim(1000, -1);
    expect("two lanes are kept", {});
    check("two lanes are kept", p.count() == 2 && p.cap() == kMaxRescueLanes);
}

void phase_and_arrivals()
{
    Rig r;
    Fetch &f = r.f;
    int owner = 0;
    check("ordered", f.pull_ordered(kCopy, nullptr, A, &owner, 0) == DPWA_OK && f.fetched() && !f.factored());
    g_log.clear();
    check("factored_on", f.factored_on(A) == hipSuccess && f.fetched() && f.factored() && f.reads(&owner, 0));
    expect("the factor has read the header: staging 0's done", {{"R", r.done0, id(A), 0}});
    f.read_in_place((const char *)kFrom, &owner, 1);
    check("a second pull before the lerp keeps the factor", f.factored() && f.reads(&owner, 1));
    check("host arrival", f.staging_writable() == hipSuccess && f.landed_on_side() == hipSuccess && f.host_wait_landed() == hipSuccess);
    f.arrived_in_staging();
    expect("a host copy into staging: the side stream waits for done0; landed is recorded there and waited for",
           {{"W", r.done0, id(SIDE), 0}, {"R", r.landed, id(SIDE), 0}, {"Y", r.landed, 0, 0}});
    check("an arrival while factored is a new fetch", f.fetched() && !f.factored() && !f.reads(&owner, 1) && f.awaits_copy() &&
                                                          f.source().ptr == f.staging() && f.source().owner == nullptr);
    check("consumed on B", f.note_consumed(B) == hipSuccess);
    f.finish();
    check("finish", !f.fetched() && !f.factored() && f.source().ptr == nullptr);
    g_log.clear();
    check("relay phase 1", f.side_after(A) == hipSuccess);
    expect("the relay's first phase: the side stream runs on from the caller's", {{"R", r.issue, id(A), 0}, {"W", r.issue, id(SIDE), 0}});
    check("relay gather", f.staging_writable_after_consumption() == hipSuccess && f.landed_on_side() == hipSuccess);
    f.arrived_in_staging();
    expect("the relay's gather: after the consumption on whatever stream, then staging 0's reader",
           {{"R", r.consumed, id(B), 0}, {"W", r.consumed, id(SIDE), 0}, {"W", r.done0, id(SIDE), 0}, {"R", r.landed, id(SIDE), 0}});
    f.note_consumed_in_place(A);
    check("stripes read in place", f.consumed_mark().stream() == A && f.fetched());
    expect("the relay's fused average records nothing", {});
}

void state()
{
    Rig r;
    Fetch &f = r.f;
    int st = -1;
    check("no fetch", f.state(10, false, &st) == DPWA_OK && st == DPWA_FETCH_LANDED);
    g_now = 5 * kMs;
    check("ordered", f.pull_ordered(kCopy, nullptr, A, nullptr, -1) == DPWA_OK);   // issued at 5 ms
    g_log.clear();
    g_pending = {r.landed};
    check("deferred relay phase", f.state(10, true, &st) == DPWA_OK && st == DPWA_FETCH_LANDED);
    expect("no fetch, or a deferred relay phase: no call", {});
    g_pending.clear();
    check("landed", f.state(10, false, &st) == DPWA_OK && st == DPWA_FETCH_LANDED);
    expect("landed", {{"Q", r.landed, 0, 0}});
    g_pending = {r.landed, r.issue};
    g_now = 1000 * kMs;
    check("no timeout", f.state(-1, false, &st) == DPWA_OK && st == DPWA_FETCH_IN_FLIGHT);
    expect("timeout_ms < 0", {{"Q", r.landed, 0, 0}});
    g_now = 15 * kMs - 1;
    check("inside", f.state(10, false, &st) == DPWA_OK && st == DPWA_FETCH_IN_FLIGHT);
    expect("inside the timeout by the host's clock: ev_issue is not asked", {{"Q", r.landed, 0, 0}});
    g_now = 15 * kMs;
    check("not out yet", f.state(10, false, &st) == DPWA_OK && st == DPWA_FETCH_IN_FLIGHT);
    expect("past it, the caller's stream has not reached ev_issue", {{"Q", r.landed, 0, 0}, {"Q", r.issue, 0, 0}});
    g_pending = {r.landed};
    const uintptr_t ps = g_next_stream, pe = g_next_event;
    g_elapsed_ms = 9.5f;
    check("probe, below", f.state(10, false, &st) == DPWA_OK && st == DPWA_FETCH_IN_FLIGHT);
    expect("the first probe makes its stream (normal priority) and timed event, and reads the time since ev_issue",
           {{"Q", r.landed, 0, 0}, {"Q", r.issue, 0, 0}, {"SC", ps, 0, -1}, {"EC", pe, 0, hipEventDefault}, {"R", pe, ps, 0},
            {"Q", pe, 0, 0}, {"T", r.issue, pe, 0}});
    g_elapsed_ms = 10.f;
    check("probe, at", f.state(10, false, &st) == DPWA_OK && st == DPWA_FETCH_TIMED_OUT);
    expect("the second probe makes nothing; elapsed at the timeout is out",
           {{"Q", r.landed, 0, 0}, {"Q", r.issue, 0, 0}, {"R", pe, ps, 0}, {"Q", pe, 0, 0}, {"T", r.issue, pe, 0}});
    g_elapsed_ms = -1.f;
    check("probe, negative", f.state(10, false, &st) == DPWA_OK && st == DPWA_FETCH_TIMED_OUT);
    g_log.clear();
    g_elapsed_ms = 0.f;
    g_pending = {r.landed, pe};
    g_pending_query_ns = 600 * 1000;   // four not-ready queries pass kProbeWaitUs
    check("probe held up", f.state(10, false, &st) == DPWA_OK && st == DPWA_FETCH_TIMED_OUT && g_error == "probe held up");
    expect("a probe not ready for more than kProbeWaitUs: no measurement, timed out",
           {{"Q", r.landed, 0, 0}, {"Q", r.issue, 0, 0}, {"R", pe, ps, 0}, {"Q", pe, 0, 0}, {"Q", pe, 0, 0}, {"Q", pe, 0, 0}, {"Q", pe, 0, 0}});
    g_pending_query_ns = 0;
    g_pending = {r.landed};
    g_now = (5 + 10 + kMaxBacklogMs) * kMs;
    check("backlog", f.state(10, false, &st) == DPWA_OK && st == DPWA_FETCH_TIMED_OUT);
    expect("beyond timeout + kMaxBacklogMs: timed out without a probe", {{"Q", r.landed, 0, 0}});
    g_now -= 1;
    g_elapsed_ms = 1.f;
    check("backlog, just inside", f.state(10, false, &st) == DPWA_OK && st == DPWA_FETCH_IN_FLIGHT);
    g_pending.clear();
    g_now = 0;
    g_log.clear();
}

}  // namespace

int main()
{
    ordered_pull();
    g_log.clear();   // (each case's fetch gives back what it holds: counted at the end)
    published_pull();
    g_log.clear();
    in_place();
    g_log.clear();
    rescue_pull();
    g_log.clear();
    budget();
    trim();
    g_log.clear();
    phase_and_arrivals();
    g_log.clear();
    state();
    g_log.clear();

    size_t left = 0;
    for (size_t k = 1; k < g_event_alive.size(); ++k) left += g_event_alive[k];
    for (size_t k = 1; k < g_stream_alive.size(); ++k) left += g_stream_alive[k];
    for (size_t k = 1; k < g_alloc.size(); ++k) left += g_alloc[k] != nullptr;
    if (left) {
        fprintf(stderr, "FAIL %zu events, streams or allocations never given back\n", left);
        ++g_failures;
    }
    if (g_failures) return 1;
    printf("fetch check ok (%zu events, %zu streams, %zu allocations)\n", g_event_alive.size() - 1, g_stream_alive.size() - 1,
           g_alloc.size() - 1);
    return 0;
}
