// order_check.cpp -- dpwa_amd/csrc/order.hpp (StreamMark, DoneEvent) against a recording stand-in
// of the five HIP entry points it calls.  No HIP runtime is linked: the calls land in the log
// below, and every case asserts the exact log.  Built with AddressSanitizer + UBSan by
// tests/test_native_sanitizers.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../dpwa_amd/csrc/order.hpp"

namespace {

struct Call {
    char op;          // 'C'reate, 'D'estroy, 'R'ecord, 'W'ait, 'Q'uery
    uintptr_t event;  // 1, 2, ... in order of creation
    uintptr_t stream; // the fake stream handle (0: the default stream)
    bool operator==(const Call &o) const { return op == o.op && event == o.event && stream == o.stream; }
};

std::vector<Call> g_log;
uintptr_t g_next_event = 1;
std::vector<int> g_alive;               // per event id: 1 while created and not destroyed
hipError_t g_record_result = hipSuccess;
hipError_t g_query_result = hipSuccess;

hipStream_t stream(uintptr_t k) { return (hipStream_t)k; }
uintptr_t id(hipEvent_t e) { return (uintptr_t)e; }
uintptr_t id(hipStream_t s) { return (uintptr_t)s; }

void must_be_alive(hipEvent_t e, const char *what)
{
    if (id(e) == 0 || id(e) >= g_alive.size() || g_alive[id(e)] != 1) {
        fprintf(stderr, "%s on event %zu, which is not alive\n", what, (size_t)id(e));
        abort();
    }
}

std::string show(const std::vector<Call> &v)
{
    std::string s;
    for (const Call &c : v) {
        char buf[64];
        snprintf(buf, sizeof(buf), "%c(e%zu,s%zu) ", c.op, (size_t)c.event, (size_t)c.stream);
        s += buf;
    }
    return s.empty() ? "(no calls)" : s;
}

int g_failures = 0;

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
        fprintf(stderr, "FAIL %s\n", name);
        ++g_failures;
    }
}

}  // namespace

extern "C" {

hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned)
{
    const uintptr_t k = g_next_event++;
    g_alive.resize(k + 1, 0);
    g_alive[k] = 1;
    *event = (hipEvent_t)k;
    g_log.push_back({'C', k, 0});
    return hipSuccess;
}

hipError_t hipEventDestroy(hipEvent_t event)
{
    must_be_alive(event, "hipEventDestroy");   // a second destroy of one event ends the program
    g_alive[id(event)] = 0;
    g_log.push_back({'D', id(event), 0});
    return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t event, hipStream_t s)
{
    must_be_alive(event, "hipEventRecord");
    g_log.push_back({'R', id(event), id(s)});
    return g_record_result;
}

hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t event, unsigned)
{
    must_be_alive(event, "hipStreamWaitEvent");
    g_log.push_back({'W', id(event), id(s)});
    return hipSuccess;
}

hipError_t hipEventQuery(hipEvent_t event)
{
    must_be_alive(event, "hipEventQuery");
    g_log.push_back({'Q', id(event), 0});
    return g_query_result;
}

}  // extern "C"

using dpwa::DoneEvent;
using dpwa::StreamMark;

int main()
{
    const hipStream_t a = stream(0xA0), b = stream(0xB0), side = stream(0x51);

    {   // a mark that was never noted makes no calls, created or not
        StreamMark m;
        check("never noted: order", m.order(a) == hipSuccess && m.order(nullptr) == hipSuccess);
        check("never noted: accessors", !m.noted() && !m.crosses(a) && m.stream() == nullptr);
        expect("never noted, no event yet", {});
        check("init", m.init() == hipSuccess && m.init() == hipSuccess);   // the second is a no-op
        const uintptr_t e = g_next_event - 1;
        expect("init creates once", {{'C', e, 0}});
        check("never noted: order after init", m.order(a) == hipSuccess);
        expect("never noted, event made", {});
        m.note(a);
        expect("note records nothing", {});
        check("same stream", m.order(a) == hipSuccess && !m.crosses(a) && m.noted() && m.stream() == a);
        expect("same stream makes no calls", {});
        check("other stream", m.order(b) == hipSuccess && m.crosses(b));
        expect("other stream: one record on the noted stream, then one wait on the waiter",
               {{'R', e, id(a)}, {'W', e, id(b)}});
        // the side stream waits, but the caller's stream order is what would cover the work
        check("covered_by", m.order(side, a) == hipSuccess);
        expect("covered_by equal to the noted stream: no calls", {});
        check("covered_by", m.order(side, b) == hipSuccess);
        expect("covered_by differs from the noted stream: the waiter waits", {{'R', e, id(a)}, {'W', e, id(side)}});
        m.note(side);
        check("waiter is the noted stream, covered_by is not", m.order(side, a) == hipSuccess);
        expect("only covered_by is compared", {{'R', e, id(side)}, {'W', e, id(side)}});
        m.clear();
        check("cleared", m.order(b) == hipSuccess && !m.noted());
        expect("a cleared mark makes no calls", {});
        m.note(a);
        check("noted again", m.order(b) == hipSuccess);
        expect("a mark noted again orders again", {{'R', e, id(a)}, {'W', e, id(b)}});
    }
    {
        const uintptr_t e = g_next_event - 1;
        expect("the mark's event is destroyed once", {{'D', e, 0}});
    }

    {   // the default stream's handle is null: indistinguishable from it when covered_by is null
        StreamMark m;
        m.note(nullptr);
        check("null noted", m.noted() && m.order(side, nullptr) == hipSuccess);
        expect("covered_by = nullptr with a null noted stream makes no calls", {});
        check("null noted, real waiter", m.order(a) == hipSuccess);   // the event is made at first need
        const uintptr_t e = g_next_event - 1;
        expect("a null noted stream and another waiter", {{'C', e, 0}, {'R', e, 0}, {'W', e, id(a)}});
        m.note(a);
        check("covered_by = nullptr, noted elsewhere", m.order(side, nullptr) == hipSuccess);
        expect("covered_by = nullptr with a non-null noted stream waits", {{'R', e, id(a)}, {'W', e, id(side)}});
    }
    g_log.clear();

    {   // a record error is returned and no wait is issued
        StreamMark m;
        check("init", m.init() == hipSuccess);
        const uintptr_t e = g_next_event - 1;
        m.note(a);
        g_log.clear();
        g_record_result = hipErrorInvalidValue;
        check("mark: record error returned", m.order(b) == hipErrorInvalidValue);
        expect("mark: no wait after a failed record", {{'R', e, id(a)}});
        DoneEvent d;
        check("done: record error returned", d.record(a) == hipErrorInvalidValue && !d.recorded());
        const uintptr_t f = g_next_event - 1;
        expect("done: failed record", {{'C', f, 0}, {'R', f, id(a)}});
        check("done: a failed record leaves nothing to wait for", d.wait(b) == hipSuccess && d.query() == hipSuccess);
        expect("done: no wait after a failed record", {});
        g_record_result = hipSuccess;
    }
    g_log.clear();

    {   // DoneEvent
        DoneEvent d;
        check("wait before record", d.wait(a) == hipSuccess && d.query() == hipSuccess && !d.recorded());
        expect("DoneEvent::wait before any record makes no calls", {});
        check("init", d.init() == hipSuccess);
        const uintptr_t e = g_next_event - 1;
        check("wait after init, before record", d.wait(a) == hipSuccess && d.query() == hipSuccess);
        expect("init alone is not a record", {{'C', e, 0}});
        check("record", d.record(a) == hipSuccess && d.recorded() && id(d.event()) == e);
        expect("record records now", {{'R', e, id(a)}});
        check("wait", d.wait(a) == hipSuccess && d.wait(b) == hipSuccess);
        expect("wait waits on whichever stream asks, the recording one included", {{'W', e, id(a)}, {'W', e, id(b)}});
        g_query_result = hipErrorNotReady;
        check("query pending", d.query() == hipErrorNotReady);
        g_query_result = hipSuccess;
        check("query done", d.query() == hipSuccess);
        expect("query", {{'Q', e, 0}, {'Q', e, 0}});
    }
    g_log.clear();

    {   // moves: the event travels, the state with it, and it is destroyed once
        StreamMark m;
        check("init", m.init() == hipSuccess);
        const uintptr_t e = g_next_event - 1;
        m.note(a);
        StreamMark n(std::move(m));
        check("moved-from mark", !m.noted() && m.order(b) == hipSuccess);
        g_log.clear();
        check("moved-to mark", n.noted() && n.stream() == a && n.order(b) == hipSuccess);
        expect("a moved mark orders with the event it was given", {{'R', e, id(a)}, {'W', e, id(b)}});
        StreamMark o;
        check("init", o.init() == hipSuccess);
        const uintptr_t f = g_next_event - 1;
        g_log.clear();
        o = std::move(n);
        expect("move assignment hands the replaced event to the source", {});
        check("assigned mark", !n.noted() && o.order(b) == hipSuccess);
        expect("an assigned mark orders with the event it was given", {{'R', e, id(a)}, {'W', e, id(b)}});

        DoneEvent d;
        check("record", d.record(a) == hipSuccess);
        const uintptr_t g = g_next_event - 1;
        std::vector<DoneEvent> v;
        v.push_back(std::move(d));
        v.emplace_back();
        v.emplace_back();          // growth moves the elements
        g_log.clear();
        check("moved-from done", !d.recorded() && d.wait(b) == hipSuccess);
        check("moved-to done", v[0].recorded() && v[0].wait(b) == hipSuccess && !v[1].recorded());
        expect("a moved DoneEvent waits with the event it was given", {{'W', g, id(b)}});
        v.clear();
        expect("the moved event is destroyed once, by its last owner", {{'D', g, 0}});
        // m owns nothing; o owns e; n left the assignment with f
    }
    expect("scope end: the assigned mark's event, then the one it replaced, once each",
           {{'D', g_next_event - 3, 0}, {'D', g_next_event - 2, 0}});

    for (size_t k = 1; k < g_alive.size(); ++k)
        if (g_alive[k]) {
            fprintf(stderr, "FAIL event %zu never destroyed\n", k);
            ++g_failures;
        }
    if (g_failures) return 1;
    printf("order check ok (%zu events)\n", g_alive.size() - 1);
    return 0;
}
