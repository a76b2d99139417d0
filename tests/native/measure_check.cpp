// measure_check.cpp -- dpwa_amd/csrc/measure.hpp (Measure, measured_average) against recording stand-ins of
// everything it calls: five launch_* functions of kernels.hpp, the three host rules of distance.cpp, six HIP
// runtime calls and set_error.  No HIP runtime is linked: the calls land in the log below, and every case
// asserts the exact log.  The "launch the average" callables here stand for the three sites of learner.cpp
// (dpwa_learner_lerp, average_launch, the batched branch of launch_plans) and log 'A' / 'L' / 'B'.
// Built with AddressSanitizer + UBSan by tests/test_native_sanitizers.py.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../dpwa_amd/csrc/measure.hpp"

using namespace dpwa;

namespace {

struct Call {
    std::string op;                   // P Pf D F T, or what an average callable logs
    const void *a, *b, *c, *d;        // the pointers, in the launch's own order (see the stand-ins)
    int64_t n;                        // n / bytes
    int64_t k;                        // count / dtype
    const void *coef;
    hipStream_t s;
    bool operator==(const Call &o) const
    {
        return op == o.op && a == o.a && b == o.b && c == o.c && d == o.d && n == o.n && k == o.k && coef == o.coef && s == o.s;
    }
};

std::vector<Call> g_log;
std::string g_fail_op;                // the stand-in of this launch fails (once told to)
std::string g_error;
std::vector<void *> g_allocs;         // every hipMalloc so far, in order
int g_live = 0, g_syncs = 0;
int g_failures = 0;

hipError_t record(Call c)
{
    const bool fail = c.op == g_fail_op;
    g_log.push_back(std::move(c));
    return fail ? hipErrorInvalidValue : hipSuccess;
}

std::string show(const std::vector<Call> &v)
{
    std::string out;
    for (const Call &c : v) {
        char buf[256];
        snprintf(buf, sizeof(buf), "\n    %s(%p %p %p %p n=%lld k=%lld coef=%p s=%p)", c.op.c_str(), c.a, c.b, c.c, c.d,
                 (long long)c.n, (long long)c.k, c.coef, (void *)c.s);
        out += buf;
    }
    return out.empty() ? " (no calls)" : out;
}

void expect(const char *name, const std::vector<Call> &want)
{
    if (!(g_log == want)) {
        fprintf(stderr, "FAIL %s\n  want%s\n  got%s\n", name, show(want).c_str(), show(g_log).c_str());
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

hipError_t launch_param_distance(const void *param, const void *peer, int64_t total, const ParamEntry *table, int64_t count,
                                 double *acc, hipStream_t s, const LaunchTiming *timing)
{
    if (timing) abort();   // a learner's pass is never timed
    return record({"P", param, peer, table, acc, total, count, nullptr, s});
}
hipError_t launch_param_distance_finish(double *acc, const ParamEntry *table, int64_t count, dpwa_param_distance_head *out,
                                        const dpwa_coef *coef, hipStream_t s, const LaunchTiming *timing)
{
    if (timing) abort();
    return record({"Pf", acc, table, out, nullptr, 0, count, coef, s});
}
// d: the layout of a segmented payload (k DPWA_MIXED, n its bytes), null for a single dtype
hipError_t launch_distance(const Elems &e, const void *param, const void *peer, double *acc, hipStream_t s)
{
    return record({"D", param, peer, acc, e.layout, e.n, e.dtype, nullptr, s});
}
hipError_t launch_distance_finish(double *acc, dpwa_distance *out, const dpwa_coef *coef, int64_t n, hipStream_t s,
                                  const LaunchTiming *timing)
{
    if (timing) abort();
    return record({"F", acc, out, nullptr, nullptr, n, 0, coef, s});
}
// d: the accumulators; coef: fa.coef_out; k: dtype, + 100 when oop, + 1000 when timed
hipError_t launch_average_tracked(int32_t dtype, void *param, const void *peer, int64_t n, const FusedArgs &fa, void *snap,
                                  bool oop, double *acc, hipStream_t s, const LaunchTiming *timing)
{
    return record({"T", param, peer, snap, acc, n, dtype + (oop ? 100 : 0) + (timing ? 1000 : 0), fa.coef_out, s});
}

// The rules of distance.cpp are not under test: any list passes, one accumulator row per range.
int param_ranges_problem(const char *, const dpwa_param_range *, int64_t, bool, int32_t, int64_t, const dpwa_layout *)
{
    return DPWA_OK;
}
int64_t param_table(const dpwa_param_range *ranges, int64_t count, std::vector<ParamEntry> *out)
{
    if (out) out->assign((size_t)count, ParamEntry{});
    for (int64_t t = 0; out && t < count; ++t)
        (*out)[(size_t)t] = ParamEntry{ranges[t].byte_offset, ranges[t].byte_offset + ranges[t].byte_length, ranges[t].dtype,
                                       (int32_t)t, 1, 0};
    return count;
}
void param_sizes(const dpwa_param_range *, int64_t count, dpwa_param_sizes &z)
{
    z.table_bytes = count * (int64_t)sizeof(ParamEntry);
    z.workspace_bytes = count * DPWA_DISTANCE_ACC_STRIDE;
    z.record_bytes = (int64_t)sizeof(dpwa_param_distance_head) + count * (int64_t)sizeof(dpwa_param_pair);
    z.max_rows = kParamDistRows;
    z.reserved = 0;
}

}  // namespace dpwa

extern "C" {

// host memory, so that AddressSanitizer sees every write, every free and whatever is never freed
hipError_t hipMalloc(void **ptr, size_t bytes)
{
    if (posix_memalign(ptr, 256, bytes)) return hipErrorOutOfMemory;
    g_allocs.push_back(*ptr);
    ++g_live;
    return hipSuccess;
}
hipError_t hipFree(void *ptr)
{
    free(ptr);
    --g_live;
    return hipSuccess;
}
hipError_t hipMemset(void *dst, int value, size_t bytes)
{
    memset(dst, value, bytes);
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind)
{
    memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void)
{
    ++g_syncs;
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t) { return "stand-in error"; }

}  // extern "C"

namespace {

// Operands as learner.cpp's sites hand them over.  Nothing dereferences them.
alignas(64) char g_flat[64], g_peer[64], g_snap[64];
dpwa_coef g_coef[3];
const hipStream_t S = (hipStream_t)0x51;
constexpr int64_t N = 1000;

const dpwa_layout &mixed_layout()
{
    static dpwa_layout y{};
    y.count = 3;
    y.seg[0] = dpwa_segment{DPWA_F32, 0, 0, 4096};
    y.seg[1] = dpwa_segment{DPWA_BF16, 0, 4096, 4096};
    y.seg[2] = dpwa_segment{DPWA_F16, 0, 8192, 4096};
    return y;
}

Payload single(int32_t dtype = DPWA_F32, int who = 0) { return Payload{{dtype, N, nullptr}, &g_coef[who]}; }
Payload mixed() { return Payload{{DPWA_MIXED, 12288, &mixed_layout()}, &g_coef[0]}; }

// "launch the average": logs `op` with the member's operands, as a site's own launch would receive them
struct Average {
    const char *op;
    const Measured &m;
    int operator()() const
    {
        HIP_TRY(record({op, m.flat, m.peer, m.snap, nullptr, m.p.n, m.p.dtype, m.p.coef, S}));
        return DPWA_OK;
    }
};

// the single fused average of learner.cpp (average_launch): fa given, so a fused round gets the tracked kernel
int average(Measure &m, const Payload &p, void *flat, const void *peer, void *snap, bool oop = false,
            const LaunchTiming *timing = nullptr)
{
    static FusedArgs fa{};
    fa.coef_out = const_cast<dpwa_coef *>(p.coef);
    const Measured one{&m, p, flat, peer, snap, &fa, oop, timing};
    return measured_average(&one, 1, S, Average{"A", one});
}

// dpwa_learner_lerp: no fa, never fused
int lerp(Measure &m, const Payload &p, void *flat, const void *peer)
{
    const Measured one{&m, p, flat, peer, nullptr};
    return measured_average(&one, 1, S, Average{"L", one});
}

const dpwa_param_range kRanges[2] = {{0, 1024, DPWA_F32, 0}, {1024, 512, DPWA_F32, 0}};
constexpr int64_t kCount = 2;
// where set_param puts things behind the table of kCount entries (measure.hpp; the sizes above)
constexpr int64_t kWorkspaceOff = 128, kRecordOff = kWorkspaceOff + kCount * DPWA_DISTANCE_ACC_STRIDE;

struct Buffers {   // of a Measure whose allocations were the last one or two
    char *dist = nullptr, *pd = nullptr;
    const void *acc() const { return dist; }
    const void *rec() const { return dist + kDistanceWorkspaceBytes; }
    const void *table() const { return pd; }
    const void *pacc() const { return pd + kWorkspaceOff; }
    const void *prec() const { return pd + kRecordOff; }
};

}  // namespace

int main()
{
    static_assert(kCount * sizeof(ParamEntry) <= (size_t)kWorkspaceOff, "table fits before the workspace");
    void *const flat = g_flat, *const snap = g_snap;
    const void *const peer = g_peer;

    {   // 1. both off: exactly the average, whatever the plan; nothing counted
        Measure m;
        const Payload p = single();
        check("off: plain", average(m, p, flat, peer, nullptr) == DPWA_OK);
        expect("off: plain", {{"A", flat, peer, nullptr, nullptr, N, DPWA_F32, p.coef, S}});
        check("off: write-through", average(m, p, flat, peer, snap) == DPWA_OK);
        expect("off: write-through", {{"A", flat, peer, snap, nullptr, N, DPWA_F32, p.coef, S}});
        check("off: resident", average(m, p, flat, peer, snap, true) == DPWA_OK);
        expect("off: resident", {{"A", flat, peer, snap, nullptr, N, DPWA_F32, p.coef, S}});
        check("off: mixed", average(m, mixed(), flat, peer, snap) == DPWA_OK);
        expect("off: mixed", {{"A", flat, peer, snap, nullptr, 12288, DPWA_MIXED, p.coef, S}});
        check("off: relay", average(m, p, flat, nullptr, snap) == DPWA_OK);   // a relay plan has no contiguous peer
        expect("off: relay", {{"A", flat, nullptr, snap, nullptr, N, DPWA_F32, p.coef, S}});
        check("off: lerp", lerp(m, p, flat, peer) == DPWA_OK);
        expect("off: lerp", {{"L", flat, peer, nullptr, nullptr, N, DPWA_F32, p.coef, S}});
        check("off: no state", !m.whole() && !m.param() && m.rounds() == 0 && m.measured() == 0 && !m.record() &&
                                   !m.param_record() && g_allocs.empty());
        check("off: never fused", !m.fused(p, flat, peer, snap));
    }

    {   // 2. whole-model on, one dtype: the tracked kernel when all three operands are aligned
        Measure m;
        check("whole: on", m.set_whole("fn", true, false) == DPWA_OK && m.whole() && g_allocs.size() == 1 && g_syncs == 1);
        Buffers b;
        b.dist = (char *)g_allocs.back();
        check("whole: record", m.record() == b.rec() && m.acc() == b.acc());
        const Payload p = single(DPWA_BF16);
        const Call F{"F", b.acc(), b.rec(), nullptr, nullptr, N, 0, p.coef, S};
        LaunchTiming timing{};
        check("whole: plain", average(m, p, flat, peer, nullptr, false, &timing) == DPWA_OK);
        expect("whole: plain = T F", {{"T", flat, peer, nullptr, b.acc(), N, DPWA_BF16 + 1000, p.coef, S}, F});
        check("whole: write-through", average(m, p, flat, peer, snap) == DPWA_OK);
        expect("whole: write-through = T F", {{"T", flat, peer, snap, b.acc(), N, DPWA_BF16, p.coef, S}, F});
        check("whole: resident", average(m, p, flat, peer, snap, true) == DPWA_OK);
        expect("whole: resident = T F", {{"T", flat, peer, snap, b.acc(), N, DPWA_BF16 + 100, p.coef, S}, F});
        const Call D{"D", nullptr, nullptr, b.acc(), nullptr, N, DPWA_BF16, nullptr, S};
        for (int which = 0; which < 3; ++which) {   // one operand 4 bytes off: the stand-alone pass, any other average
            void *f = which == 0 ? g_flat + 4 : flat, *w = which == 2 ? g_snap + 4 : snap;
            const void *q = which == 1 ? g_peer + 4 : peer;
            check("whole: unaligned is not fused", !m.fused(p, f, q, w) && m.fused(p, flat, peer, snap));
            check("whole: unaligned", average(m, p, f, q, w) == DPWA_OK);
            Call d = D;
            d.a = f;
            d.b = q;
            expect("whole: one operand 4 bytes off = D A F", {d, {"A", f, q, w, nullptr, N, DPWA_BF16, p.coef, S}, F});
        }
        check("whole: nothing counted", m.rounds() == 0 && m.measured() == 0);

        // 6. the split path never fuses: D L F
        check("whole: lerp", lerp(m, p, flat, peer) == DPWA_OK);
        Call d = D;
        d.a = flat;
        d.b = peer;
        expect("whole: lerp = D L F", {d, {"L", flat, peer, nullptr, nullptr, N, DPWA_BF16, p.coef, S}, F});

        // 3. DPWA_MIXED: the pass gets the layout, and the finish counts the element slots of the segments
        const Payload x = mixed();
        check("whole: mixed", average(m, x, flat, peer, snap) == DPWA_OK);
        expect("whole: mixed = D A F(5120)", {{"D", flat, peer, b.acc(), &mixed_layout(), 12288, DPWA_MIXED, nullptr, S},
                                              {"A", flat, peer, snap, nullptr, 12288, DPWA_MIXED, x.coef, S},
                                              {"F", b.acc(), b.rec(), nullptr, nullptr, 1024 + 2048 + 2048, 0, x.coef, S}});

        // 9. off and on again keeps the buffer
        check("whole: off", m.set_whole("fn", false, false) == DPWA_OK && !m.whole() && m.record() == b.rec());
        check("whole: off runs the average alone", average(m, p, flat, peer, snap) == DPWA_OK);
        expect("whole: off = A", {{"A", flat, peer, snap, nullptr, N, DPWA_BF16, p.coef, S}});
        check("whole: on again", m.set_whole("fn", true, false) == DPWA_OK && m.record() == b.rec() && g_allocs.size() == 1);
    }
    check("whole: its buffer is freed with it", g_live == 0);

    {   // 4. per-parameter on, every = 1
        Measure m;
        const Payload p = single(DPWA_F16);
        check("param: on", m.set_param("fn", kRanges, kCount, 1, p, false) == DPWA_OK && m.param() && g_allocs.size() == 2);
        Buffers b;
        b.pd = (char *)g_allocs.back();
        check("param: record", m.param_record() == b.prec() && m.param_count() == kCount);
        check("param: table written", ((const ParamEntry *)b.pd)[1].begin == 1024 && ((const ParamEntry *)b.pd)[1].end == 1536);
        const Call P{"P", flat, peer, b.table(), b.pacc(), N * 2, kCount, nullptr, S};   // n * size bytes
        const Call Pf{"Pf", b.pacc(), b.table(), b.prec(), nullptr, 0, kCount, p.coef, S};
        check("param: alone", average(m, p, flat, peer, snap) == DPWA_OK);
        expect("param: alone = P A Pf", {P, {"A", flat, peer, snap, nullptr, N, DPWA_F16, p.coef, S}, Pf});

        check("param: whole on", m.set_whole("fn", true, false) == DPWA_OK && g_allocs.size() == 3);
        b.dist = (char *)g_allocs.back();
        const Call F{"F", b.acc(), b.rec(), nullptr, nullptr, N, 0, p.coef, S};
        check("both: aligned", average(m, p, flat, peer, snap) == DPWA_OK);
        expect("both: aligned = P T F Pf", {P, {"T", flat, peer, snap, b.acc(), N, DPWA_F16, p.coef, S}, F, Pf});
        const Payload x = mixed();
        Call Pm = P;
        Pm.n = 12288;   // a mixed payload's n is its bytes
        check("both: mixed", average(m, x, flat, peer, snap) == DPWA_OK);
        expect("both: mixed = P D A F Pf", {Pm,
                                            {"D", flat, peer, b.acc(), &mixed_layout(), 12288, DPWA_MIXED, nullptr, S},
                                            {"A", flat, peer, snap, nullptr, 12288, DPWA_MIXED, x.coef, S},
                                            {"F", b.acc(), b.rec(), nullptr, nullptr, 5120, 0, x.coef, S},
                                            Pf});
        // 6. the split path, both on: P D L F Pf
        check("both: lerp", lerp(m, p, flat, peer) == DPWA_OK);
        expect("both: lerp = P D L F Pf", {P,
                                           {"D", flat, peer, b.acc(), nullptr, N, DPWA_F16, nullptr, S},
                                           {"L", flat, peer, nullptr, nullptr, N, DPWA_F16, p.coef, S},
                                           F,
                                           Pf});
        check("both: four rounds counted and measured", m.rounds() == 4 && m.measured() == 4);

        // the unaligned refusal comes before the round is counted
        check("param: unaligned parameters are refused", m.operands_problem("dpwa_learner_average", g_flat + 4) == DPWA_ERR_ARG &&
                                                             g_error == "dpwa_learner_average: the per-parameter distance "
                                                                        "(dpwa_learner_set_param_distance) has no form for "
                                                                        "parameters that are not 16-byte aligned");
        check("param: aligned ones are not", m.operands_problem("fn", flat) == DPWA_OK && m.rounds() == 4);

        // 9. off and on again replaces the buffer and restarts the count
        check("param: off", m.set_param("fn", nullptr, 0, 1, p, false) == DPWA_OK && !m.param() && m.param_record() == b.prec());
        const int live = g_live;
        check("param: on again", m.set_param("fn", kRanges, kCount, 3, p, false) == DPWA_OK && g_allocs.size() == 4 &&
                                     g_live == live && m.rounds() == 0 && m.measured() == 0);
        b.pd = (char *)g_allocs.back();
        check("param: new record", m.param_record() == b.prec());
        check("param: whole off", m.set_whole("fn", false, false) == DPWA_OK);

        // 5. every = 3 over seven rounds: P .. Pf on rounds 3 and 6 only
        const Call P3{"P", flat, peer, b.table(), b.pacc(), N * 2, kCount, nullptr, S};
        const Call Pf3{"Pf", b.pacc(), b.table(), b.prec(), nullptr, 0, kCount, p.coef, S};
        const Call A{"A", flat, peer, nullptr, nullptr, N, DPWA_F16, p.coef, S};
        for (int round = 1; round <= 7; ++round) {
            check("every 3: round", average(m, p, flat, peer, nullptr) == DPWA_OK);
            if (round % 3 == 0) expect("every 3: a measured round = P A Pf", {P3, A, Pf3});
            else expect("every 3: a skipped round = A", {A});
        }
        check("every 3: seven counted, two measured", m.rounds() == 7 && m.measured() == 2);

        // 8. a failing launch: DPWA_ERR_HIP comes back and nothing after it is launched.  As in the code this
        // replaced, the round is counted before its pass is launched and counted as measured only after the
        // launch succeeded, and the finishing step of a round whose average never ran is not launched later: the
        // next round decides anew.
        check("fail: every = 1", m.set_param("fn", kRanges, kCount, 1, p, false) == DPWA_OK);
        b.pd = (char *)g_allocs.back();
        const Call P1{"P", flat, peer, b.table(), b.pacc(), N * 2, kCount, nullptr, S};
        g_fail_op = "P";
        check("fail: the pass", average(m, p, flat, peer, nullptr) == DPWA_ERR_HIP && g_error.find("launch_param_distance") != std::string::npos);
        expect("fail: the pass = P and no more", {P1});
        check("fail: counted, not measured", m.rounds() == 1 && m.measured() == 0);
        g_fail_op = "A";
        check("fail: the average", average(m, p, flat, peer, nullptr) == DPWA_ERR_HIP);
        expect("fail: the average = P A and no finish", {P1, A});
        check("fail: counted and measured", m.rounds() == 2 && m.measured() == 1);
        g_fail_op.clear();
        check("fail: the next round", average(m, p, flat, peer, nullptr) == DPWA_OK);
        expect("fail: the next round = P A Pf", {P1, A, {"Pf", b.pacc(), b.table(), b.prec(), nullptr, 0, kCount, p.coef, S}});
    }
    check("param: its buffers are freed with it", g_live == 0);

    {   // 7. a batch of three: whole-model on, per-parameter on, neither.  Member by member: the passes of
        // member 0, then of member 1; the one dispatch; the finishes of member 0, then of member 1.
        Measure m0, m1, m2;
        const Payload p0 = single(DPWA_F32, 0), p1 = single(DPWA_F32, 1), p2 = single(DPWA_F32, 2);
        check("batch: switches", m0.set_whole("fn", true, false) == DPWA_OK);
        Buffers b0, b1;
        b0.dist = (char *)g_allocs.back();
        check("batch: switches", m1.set_param("fn", kRanges, kCount, 1, p1, false) == DPWA_OK);
        b1.pd = (char *)g_allocs.back();
        const Measured members[3] = {{&m0, p0, g_flat, g_peer, g_snap},
                                     {&m1, p1, g_flat + 16, g_peer + 16, g_snap + 16},
                                     {&m2, p2, g_flat + 32, g_peer + 32, g_snap + 32}};
        check("batch", measured_average(members, 3, S, Average{"B", members[0]}) == DPWA_OK);
        expect("batch = D0 P1 B F0 Pf1",   // aligned operands, yet no tracked kernel: a dispatch never fuses
               {{"D", g_flat, g_peer, b0.acc(), nullptr, N, DPWA_F32, nullptr, S},
                {"P", g_flat + 16, g_peer + 16, b1.table(), b1.pacc(), N * 4, kCount, nullptr, S},
                {"B", g_flat, g_peer, g_snap, nullptr, N, DPWA_F32, p0.coef, S},
                {"F", b0.acc(), b0.rec(), nullptr, nullptr, N, 0, p0.coef, S},
                {"Pf", b1.pacc(), b1.table(), b1.prec(), nullptr, 0, kCount, p1.coef, S}});
        check("batch: counted for the second member only", m0.rounds() == 0 && m1.rounds() == 1 && m1.measured() == 1 &&
                                                               m2.rounds() == 0 && !m2.record() && !m2.param_record());
        g_fail_op = "D";   // the first member's pass fails: nothing for the others, no dispatch
        check("batch: failing pass", measured_average(members, 3, S, Average{"B", members[0]}) == DPWA_ERR_HIP);
        expect("batch: failing pass = D0 and no more", {{"D", g_flat, g_peer, b0.acc(), nullptr, N, DPWA_F32, nullptr, S}});
        check("batch: the second member's round was not counted", m1.rounds() == 1);
        g_fail_op.clear();
    }

    {   // 9. refusals: the switch stays off and nothing is allocated
        Measure m;
        const size_t allocs = g_allocs.size();
        const Payload p = single();
        check("refuse: whole, relay pending", m.set_whole("dpwa_learner_set_distance", true, true) == DPWA_ERR_STATE && !m.whole());
        const std::string sentence = g_error.substr(g_error.find(": "));
        check("refuse: the sentence", g_error == "dpwa_learner_set_distance: a fused relay second phase is pending "
                                                 "(dpwa_learner_relay_phase2 with fuse != 0), which reads no contiguous peer "
                                                 "snapshot to measure against");
        check("refuse: param, relay pending", m.set_param("dpwa_learner_set_param_distance", kRanges, kCount, 1, p, true) == DPWA_ERR_STATE &&
                                                  !m.param() && g_error == "dpwa_learner_set_param_distance" + sentence);
        check("refuse: every = 0", m.set_param("fn", kRanges, kCount, 0, p, false) == DPWA_ERR_ARG && !m.param() &&
                                       g_error == "fn: every = 0, it must be >= 1");
        const Payload no_layout{{DPWA_MIXED, 12288, nullptr}, &g_coef[0]};
        check("refuse: no layout yet", m.set_param("fn", kRanges, kCount, 1, no_layout, false) == DPWA_ERR_STATE && !m.param() &&
                                           g_error == "fn: a DPWA_MIXED learner has no layout yet (dpwa_learner_set_layout)");
        check("refuse: switching off with a relay pending is fine", m.set_whole("fn", false, true) == DPWA_OK);
        check("refuse: nothing allocated", g_allocs.size() == allocs && !m.record() && !m.param_record());
        check("refuse: nothing launched", average(m, p, flat, peer, snap) == DPWA_OK);
        expect("refuse: the average alone", {{"A", flat, peer, snap, nullptr, N, DPWA_F32, p.coef, S}});
    }

    if (g_live != 0) {
        fprintf(stderr, "FAIL %d device buffers never freed\n", g_live);
        ++g_failures;
    }
    if (g_failures) return 1;
    printf("measure check ok (%zu buffers)\n", g_allocs.size());
    return 0;
}
