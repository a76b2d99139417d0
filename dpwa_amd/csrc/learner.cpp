// learner.cpp -- the per-node runtime behind DpwaConnection (dpwa/dpwa.py:54-156) on MI355X.
//
// The reference keeps, per node, an RxThread that serves the latest (state, payload)
// under a lock (conn.py:51-172) and a TxThread that fetches one peer's (state, payload)
// over TCP (conn.py:197-334).  Here a node (learner) owns, on its GPU:
//   slots    two snapshot slots [header 256 B | pad to 4 KiB | payload] -- RxThread.state/payload,
//            double-buffered so a publish never overwrites the slot a peer may be reading
//   staging  one slot-sized buffer receiving a peer's snapshot -- TxThread.peer_payload (fetch.hpp)
//   ctl      the device clock and the averaging coefficients (dpwa_coef)
// and a side stream on which fetches (xGMI pulls for peers on other GPUs) overlap the
// training step.  Nothing here synchronises the host with the device except the explicit
// read/write helpers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <set>
#include <unistd.h>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "fetch.hpp"
#include "kernels.hpp"
#include "measure.hpp"
#include "order.hpp"

namespace {

thread_local std::string g_last_error;

}  // namespace

namespace dpwa {

int set_error(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

}  // namespace dpwa

using namespace dpwa;

namespace {

constexpr size_t kHeader = sizeof(dpwa_header);
constexpr size_t kPayloadOff = DPWA_SLOT_PAYLOAD_OFFSET;   // [header | pad | payload]
static_assert(kPayloadOff >= kHeader && kPayloadOff % 1024 == 0, "payload offset");
static_assert(sizeof(dpwa_header) == 256, "dpwa_header must be 256 bytes");
constexpr uint64_t kIpcMagic = 0x445057414950430aULL;  // "DPWAIPC\n"

struct IpcBlob {
    hipIpcMemHandle_t handle;   // 64 B
    uint64_t magic;
    int64_t slot_stride;
    int64_t n;
    int32_t dtype;
    int32_t device;
    int32_t pid;
    int32_t vmm;                // 1: the allocation is shared as fds (dpwa_learner_export_fds)
    int32_t layout_digest;      // DPWA_MIXED: dpwa_layout_digest of the payload's layout; else 0
};
static_assert(sizeof(IpcBlob) <= DPWA_IPC_HANDLE_BYTES, "IPC blob too large");

// An exportable device allocation (snapshot slots, relay buffer).  Ordinary allocations come
// from hipMalloc and are shared with hipIpcGetMemHandle / hipIpcOpenMemHandle.  On this ROCm
// stack hipIpcOpenMemHandle never returns for allocations above ~2 GiB (tools/ipc_size_probe.py),
// so allocations from kVmmMinBytes up (or any size with DPWA_VMM=1) are built from hipMemCreate
// chunks mapped contiguously, and shared as one POSIX fd per chunk (hipMemExportToShareableHandle)
// that the peer maps contiguously again (tools/vmm_probe.cpp; streaming rates equal hipMalloc's,
// tools/vmm_perf.hip).
size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

constexpr size_t kVmmMinBytes = (size_t)3 << 29;     // 1.5 GiB
constexpr size_t kVmmChunk = (size_t)1 << 30;        // 1 GiB per exported chunk
constexpr size_t kVmmAlign = (size_t)2 << 20;

struct DevMem {
    char *ptr = nullptr;
    size_t bytes = 0;                                   // mapped bytes (VMM: chunk multiple)
    size_t chunk = 0;
    std::vector<hipMemGenericAllocationHandle_t> handles;   // VMM chunks; empty: hipMalloc
    bool vmm() const { return !handles.empty(); }

    DevMem() = default;
    DevMem(DevMem &&o) noexcept { *this = std::move(o); }
    DevMem &operator=(DevMem &&o) noexcept   // `o` leaves with what this held, and frees it
    {
        std::swap(ptr, o.ptr);
        std::swap(bytes, o.bytes);
        std::swap(chunk, o.chunk);
        handles.swap(o.handles);
        return *this;
    }
    ~DevMem()
    {
        if (!ptr) return;
        if (vmm()) {
            (void)hipMemUnmap(ptr, bytes);
            for (auto h : handles) (void)hipMemRelease(h);
            (void)hipMemAddressFree(ptr, bytes);
        } else {
            (void)hipFree(ptr);
        }
    }
};

// One pinned 32-bit word, zero at first, that the device writes through `dev` and the host polls
// through host() without waiting for anything.
template <class T> struct HostWord : Owned<void *, hipHostFree> {
    static_assert(sizeof(T) == 4, "a 32-bit word");
    T *dev = nullptr;
    T *host() const { return (T *)h; }
    hipError_t alloc()
    {
        hipError_t e = hipHostMalloc(&h, sizeof(T), hipHostMallocMapped);
        if (e != hipSuccess) return e;
        *host() = 0;
        return hipHostGetDevicePointer((void **)&dev, h, 0);
    }
};

hipMemAllocationProp vmm_prop(int device)
{
    hipMemAllocationProp p;
    memset(&p, 0, sizeof(p));
    p.type = hipMemAllocationTypePinned;
    p.requestedHandleType = hipMemHandleTypePosixFileDescriptor;
    p.location.type = hipMemLocationTypeDevice;
    p.location.id = device;
    return p;
}

hipError_t vmm_grant(const DevMem &m, int device)
{
    hipMemAccessDesc a;
    memset(&a, 0, sizeof(a));
    a.location.type = hipMemLocationTypeDevice;
    a.location.id = device;
    a.flags = hipMemAccessFlagsProtReadWrite;
    return hipMemSetAccess(m.ptr, m.bytes, &a, 1);
}

// Maps `n` chunks (VMM handles in h[]) contiguously into a fresh reservation, readable and
// writable from `device`; releases the handles on failure.
hipError_t vmm_map(DevMem &m, std::vector<hipMemGenericAllocationHandle_t> &h, size_t chunk, int device)
{
    m = DevMem();
    const size_t total = chunk * h.size();
    void *va = nullptr;
    hipError_t e = hipMemAddressReserve(&va, total, kVmmAlign, nullptr, 0);
    size_t mapped = 0;
    if (e == hipSuccess) {
        for (; mapped < h.size(); ++mapped)
            if ((e = hipMemMap((char *)va + mapped * chunk, chunk, 0, h[mapped], 0)) != hipSuccess) break;
    }
    if (e == hipSuccess) {   // fully mapped: `m` owns it, and gives it back if the grant fails
        m.ptr = (char *)va;
        m.bytes = total;
        m.chunk = chunk;
        m.handles = h;
        if ((e = vmm_grant(m, device)) == hipSuccess) return hipSuccess;
        m = DevMem();
    } else {
        if (va) {
            if (mapped) (void)hipMemUnmap(va, mapped * chunk);
            (void)hipMemAddressFree(va, total);
        }
        for (auto x : h) (void)hipMemRelease(x);
    }
    h.clear();
    return e;
}

bool use_vmm(size_t bytes)
{
    const char *e = getenv("DPWA_VMM");
    if (e && e[0] == '1') return true;
    if (e && e[0] == '0') return false;
    return bytes >= kVmmMinBytes;
}

hipError_t devmem_alloc(DevMem &m, size_t bytes, int device)
{
    m = DevMem();
    if (!use_vmm(bytes)) {
        hipError_t e = hipMalloc(&m.ptr, bytes);
        if (e == hipSuccess) m.bytes = bytes;
        return e;
    }
    const hipMemAllocationProp prop = vmm_prop(device);
    size_t gran = 0;
    hipError_t e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended);
    if (e != hipSuccess) return e;
    const size_t unit = std::max(gran, kVmmAlign);
    size_t chunk = std::min(kVmmChunk, round_up(bytes, unit));
    chunk = round_up(chunk, unit);
    const size_t n = (bytes + chunk - 1) / chunk;
    std::vector<hipMemGenericAllocationHandle_t> h;
    for (size_t i = 0; i < n; ++i) {
        hipMemGenericAllocationHandle_t x;
        if ((e = hipMemCreate(&x, chunk, &prop, 0)) != hipSuccess) {
            for (auto y : h) (void)hipMemRelease(y);
            return e;
        }
        h.push_back(x);
    }
    return vmm_map(m, h, chunk, device);
}

// One POSIX fd per chunk of a VMM allocation (the caller closes them).
int devmem_export(const DevMem &m, int *fds, int max_fds, int *n_fds, int64_t *chunk_bytes)
{
    *n_fds = 0;
    if (chunk_bytes) *chunk_bytes = (int64_t)m.chunk;
    if (!m.vmm()) return DPWA_OK;
    if ((int)m.handles.size() > max_fds)
        return set_error(DPWA_ERR_ARG, "export: %zu chunks, room for %d fds", m.handles.size(), max_fds);
    for (size_t i = 0; i < m.handles.size(); ++i) {
        int fd = -1;
        hipError_t e = hipMemExportToShareableHandle(&fd, m.handles[i], hipMemHandleTypePosixFileDescriptor, 0);
        if (e != hipSuccess) {
            for (int j = 0; j < (int)i; ++j) close(fds[j]);
            return set_error(DPWA_ERR_HIP, "hipMemExportToShareableHandle: %s", hipGetErrorString(e));
        }
        fds[i] = fd;
    }
    *n_fds = (int)m.handles.size();
    return DPWA_OK;
}

// Maps a peer's exported chunks (fds from devmem_export, received over a Unix socket) into
// this process, readable and writable from `device`.  The fds stay the caller's.
int devmem_import(DevMem &m, const int *fds, int n_fds, int64_t chunk, size_t need_bytes, int device)
{
    if (n_fds < 1 || chunk <= 0 || (size_t)chunk * (size_t)n_fds < need_bytes)
        return set_error(DPWA_ERR_ARG, "import: %d chunks of %lld bytes for %zu bytes", n_fds, (long long)chunk,
                         need_bytes);
    // How the fd is handed over depends on the runtime in the process (a torch process runs the
    // HIP runtime torch bundles): 7.0 reads the fd through the pointer (and faults on an fd
    // passed as the pointer value), 7.2 takes the fd as the pointer value (and rejects an
    // address as an invalid fd) -- tools/vmm_torch_probe.py, tools/vmm_probe.cpp.
    int rt = 0;
    (void)hipRuntimeGetVersion(&rt);
    const bool fd_by_value = rt >= 70200000;
    std::vector<hipMemGenericAllocationHandle_t> h;
    for (int i = 0; i < n_fds; ++i) {
        hipMemGenericAllocationHandle_t x;
        int fd = fds[i];
        hipError_t e = hipMemImportFromShareableHandle(&x, fd_by_value ? (void *)(intptr_t)fd : (void *)&fd,
                                                       hipMemHandleTypePosixFileDescriptor);
        if (e == hipErrorInvalidValue && fd_by_value)   // a runtime of the older convention
            e = hipMemImportFromShareableHandle(&x, (void *)&fd, hipMemHandleTypePosixFileDescriptor);
        if (e != hipSuccess) {
            for (auto y : h) (void)hipMemRelease(y);
            return set_error(DPWA_ERR_HIP, "hipMemImportFromShareableHandle: %s", hipGetErrorString(e));
        }
        h.push_back(x);
    }
    hipError_t e = vmm_map(m, h, (size_t)chunk, device);
    if (e != hipSuccess) return set_error(DPWA_ERR_HIP, "import: mapping the peer's chunks: %s", hipGetErrorString(e));
    return DPWA_OK;
}

struct Ctl {            // device control block
    double clock[4];    // a ring: a factor reads clock[cur] and writes clock[cur+1]; a
                        // write-through average also writes the next publish's clock+1 into
                        // clock[cur+2], which that publish then selects without a kernel
    dpwa_coef coef;
    int32_t guard_dirty;   // reuse guard: the generation (publish number) of the last publish that found
                           // the parameters changed (kernels.hip k_guard_publish)
    uint32_t guard_hits;   // ... and how many publishes did
    int32_t window_dirty;  // window guard (resident): the generation of the last window found written
    uint32_t window_hits;  // ... and how many windows were
    // the non-finite peer check (dpwa_learner_set_finite_check): the stamp of the last checked round whose peer
    // snapshot held a NaN or an inf (kernels.hip k_peer_finite; never cleared), and the rounds skipped for it
    uint32_t finite_veto;
    uint32_t reserved;
    uint64_t finite_skips;
};


// Registry of live learners, so a learner never dereferences a destroyed local peer.
std::mutex g_reg_mu;
std::set<dpwa_learner *> g_live;

class DeviceGuard {
public:
    explicit DeviceGuard(int dev)
    {
        (void)hipGetDevice(&prev_);
        if (prev_ != dev) (void)hipSetDevice(dev);
        dev_ = dev;
    }
    ~DeviceGuard()
    {
        if (prev_ != dev_) (void)hipSetDevice(prev_);
    }

private:
    int prev_ = 0, dev_ = 0;
};

}  // namespace

struct Endpoint {
    int kind = 0;                    // 1 local learner, 2 IPC-mapped
    dpwa_learner *local = nullptr;
    char *base = nullptr;            // slot 0 in this process's address space
    int device = -1;
    int64_t slot_stride = 0;
    int64_t n = 0;
    int32_t dtype = 0;
    DevMem imported;                 // kind 2 through fds (VMM); empty: hipIpc-opened `base`
};

static void close_endpoint(Endpoint &ep)
{
    if (ep.kind != 2 || !ep.base) return;
    if (ep.imported.vmm())
        ep.imported = DevMem();
    else
        (void)hipIpcCloseMemHandle(ep.base);
    ep.base = nullptr;
}

namespace {

// Window guard (resident, with reuse_guard): each publish checks the payload published last time
// against the samples saved then and saves the new payload's (kernels.hip k_window_roll); written
// windows are counted on the device and mirrored into a host-mapped word the next publishes read
// without waiting.  Made at first use (window_alloc).
struct WindowGuard {
    DevBuf sample;                      // kWindowSampleBytes
    HostWord<uint32_t> hits;            // windows found written (device-written)
    StreamMark rolled;                  // the last roll: a roll on another stream runs after it
    const char *src = nullptr;          // payload the samples were taken from (NULL: none)
    int32_t gen = 0;
    uint32_t reported = 0;
};

// Begin/end event pairs for timed launches (bench), handed out in order.
struct TimingRing {
    std::vector<LaunchTiming> pairs;
    int used = 0;

    TimingRing() = default;
    TimingRing(const TimingRing &) = delete;
    ~TimingRing() { (void)reserve(0); }
    // `capacity` fresh pairs in place of the old ones (the caller has synchronised the device)
    hipError_t reserve(int capacity)
    {
        for (auto &t : pairs) {
            if (t.start) (void)hipEventDestroy(t.start);
            if (t.stop) (void)hipEventDestroy(t.stop);
        }
        pairs.assign((size_t)capacity, LaunchTiming{});
        used = 0;
        hipError_t e = hipSuccess;
        for (auto &t : pairs)
            if (e == hipSuccess && (e = hipEventCreate(&t.start)) == hipSuccess) e = hipEventCreate(&t.stop);
        if (e != hipSuccess) (void)reserve(0);   // none rather than some
        return e;
    }
    // the next unused pair, or NULL when all are taken
    const LaunchTiming *take() { return used < (int)pairs.size() ? &pairs[used++] : nullptr; }
    // microseconds of the pairs taken so far, at most `max` (waits for each to complete)
    hipError_t read(float *us_out, int max, int *count) const
    {
        const int k = used < max ? used : max;
        for (int i = 0; i < k; ++i) {
            float ms = 0.f;
            hipError_t e = hipEventSynchronize(pairs[i].stop);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, pairs[i].start, pairs[i].stop);
            if (e != hipSuccess) return e;
            us_out[i] = ms * 1000.f;
        }
        *count = k;
        return hipSuccess;
    }
};

}  // namespace

struct dpwa_learner {
    int device = 0;
    int64_t n = 0;
    int32_t dtype = DPWA_F32;
    // DPWA_MIXED: which bytes of the payload hold which type (dpwa_learner_set_layout); the
    // digest is what peers compare, 0 until the layout is set
    dpwa_layout layout{};
    uint32_t layout_digest = 0;
    dpwa_interp cfg{};
    size_t payload_bytes = 0;
    size_t slot_stride = 0;
    // Every HIP object below has an owner that frees it: `delete` tears a learner down (after
    // dpwa_learner_destroy's device sync nothing is in flight, so the members go in any order).
    DevMem slot_mem;                // 2 slots
    Ctl *ctl = nullptr;             // (= ctl_mem.ptr())
    DevBuf ctl_mem;
    uint64_t version = 0;
    int cur = 0;                        // index of the live clock in ctl->clock (mod 4)
    bool exported = false;
    Stream side;
    // who waits for whom across streams (order.hpp)
    StreamMark published[2];            // slot k's publish (noted under pub_mu)
    // the fetch in flight: its source, staging buffers and rescue lanes, who waits for it and when
    // its buffer may be refilled (fetch.hpp)
    Fetch fetch;
    DoneEvent factor_done;              // last factor computation done
    int pull_mode = DPWA_PULL_COPY_ENGINE;   // how cross-device fetches move bytes
    int pull_blocks = 512;
    bool loss_f32 = false;              // device loss pointers point at a float32
    // write-through snapshot: the last average also wrote its result into the slot of the
    // next publish (for the flat buffer `wt_flat`; noted while that holds: set_written_through)
    StreamMark written_through;
    const void *wt_flat = nullptr;
    bool wt_header = false;             // the write-through average also wrote the next header
    bool header_on_publish = false;     // never write the next header ahead (served to wire peers)
    bool reuse_guard = false;           // check a header-only publish's parameters on the device
    // resident parameters (dpwa_learner_set_resident): they live in slot res_slot's payload and
    // move to the other slot at every average (or relocate)
    bool resident = false;
    int res_slot = 0;
    WindowGuard window;
    // timing of the averaging launches (bench): kernel begin/end events, filled in order
    TimingRing avg_times;
    bool timing_armed = false;   // time the next averaging launch (one-shot)
    // timing of copying fetches (bench at N > 1: the pull over xGMI), filled in order
    TimingRing fetch_times;
    // relay transport (multi-link lock-step pulls), see kernels.hip
    bool relay_on = false;
    int relay_world = 0, relay_rank = 0;
    int64_t relay_stripe = 0;
    DevMem relay_mem;                        // world x stripe, IPC-exported
    std::vector<const char *> relay_slots;   // per rank: slot 0 base (own or IPC-mapped)
    std::vector<const char *> relay_bufs;    // per rank: relay buffer (own or IPC-mapped)
    std::vector<char *> relay_opened;        // IPC mappings to close (dpwa_learner_destroy)
    std::vector<DevMem> relay_imported;      // fd-imported relay buffers
    DoneEvent relay_done;                    // all relay work of the last round
    // phase 2 deferred into the average (dpwa_learner_relay_phase2 with fuse != 0): the stripes
    // are read where phase 1 left them by the next fused average, or gathered into staging
    // first if the fetch is consumed any other way (relay_materialize)
    bool relay_deferred = false;
    RelayArgs relay_saved{};
    int relay_saved_pick = -1, relay_saved_blocks = 0;
    // host readers of published slots (wire bridge) run on other threads; their stream is created
    // at the first read, under pub_mu
    std::mutex pub_mu;
    Stream read_stream;
    Event ev_read;
    std::unordered_map<int, Endpoint> peers;
    // learners (local) that read our slot k and must be waited for before rewriting it
    std::mutex readers_mu;
    std::vector<dpwa_learner *> readers[2];
    // the distances to the peer (dpwa_learner_set_distance, dpwa_learner_set_param_distance) and all
    // that is launched for them around an average (measure.hpp)
    Measure measure;
    // skip a round whose peer snapshot is not finite (dpwa_learner_set_finite_check); the stamp of the last
    // checked round: never 0, so the zeroed veto word matches no round
    bool finite_check = false;
    uint32_t finite_stamp = 0;
    HostWord<int32_t> status;           // pinned mirror of coef.status for non-blocking polls
    // the consensus of a group (dpwa_learner_consensus): its accumulator rows, made and zeroed at the
    // first call that measures; where its last pass ran, for whoever rewrites a slot it read
    DevBuf consensus_rows;
    StreamMark consensus_read;
};

static char *slot_payload(const dpwa_learner *l, int k)
{
    return l->slot_mem.ptr + (size_t)k * l->slot_stride + kPayloadOff;
}

// What the learner averages, as its launches and its measurements see it.
static Payload payload(const dpwa_learner *l)
{
    return Payload{{l->dtype, l->n, l->layout_digest ? &l->layout : nullptr}, &l->ctl->coef};
}

int64_t dpwa::now_ns()
{
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

static bool is_live(dpwa_learner *l)
{
    std::lock_guard<std::mutex> g(g_reg_mu);
    return g_live.count(l) != 0;
}

// ---------------------------------------------------------------- stateless entry points
// (What they share: kernels.hpp.)  The six lerp wrappers' body; `fn` names the entry in messages.
static int lerp_entry(const char *fn, int32_t dtype, void *param, const void *peer, int64_t n,
                      const dpwa_coef *coef_dev, const double *factor, dpwa_stream_t stream)
{
    if (n < 0 || (n > 0 && (!param || !peer || (!factor && !coef_dev)))) return set_error(DPWA_ERR_ARG, "%s: bad arguments", fn);
    const float f = factor ? (float)*factor : 0.f, g = factor ? (float)(1.0 - *factor) : 0.f;
    HIP_TRY(launch_lerp(Elems{dtype, n, nullptr}, param, peer, factor ? nullptr : coef_dev, f, g, (hipStream_t)stream));
    return DPWA_OK;
}

extern "C" {

const char *dpwa_last_error(void) { return g_last_error.c_str(); }

int dpwa_abi_version(void) { return DPWA_ABI_VERSION; }

int dpwa_lerp_f32(float *param, const float *peer, int64_t n, const dpwa_coef *coef_dev, dpwa_stream_t stream)
{
    return lerp_entry("dpwa_lerp_f32", DPWA_F32, param, peer, n, coef_dev, nullptr, stream);
}

int dpwa_lerp_bf16(uint16_t *param, const uint16_t *peer, int64_t n, const dpwa_coef *coef_dev,
                   dpwa_stream_t stream)
{
    return lerp_entry("dpwa_lerp_bf16", DPWA_BF16, param, peer, n, coef_dev, nullptr, stream);
}

int dpwa_lerp_f16(uint16_t *param, const uint16_t *peer, int64_t n, const dpwa_coef *coef_dev,
                  dpwa_stream_t stream)
{
    return lerp_entry("dpwa_lerp_f16", DPWA_F16, param, peer, n, coef_dev, nullptr, stream);
}

int dpwa_lerp_f32_host(float *param, const float *peer, int64_t n, double factor, dpwa_stream_t stream)
{
    return lerp_entry("dpwa_lerp_f32_host", DPWA_F32, param, peer, n, nullptr, &factor, stream);
}

int dpwa_lerp_bf16_host(uint16_t *param, const uint16_t *peer, int64_t n, double factor, dpwa_stream_t stream)
{
    return lerp_entry("dpwa_lerp_bf16_host", DPWA_BF16, param, peer, n, nullptr, &factor, stream);
}

int dpwa_lerp_f16_host(uint16_t *param, const uint16_t *peer, int64_t n, double factor, dpwa_stream_t stream)
{
    return lerp_entry("dpwa_lerp_f16_host", DPWA_F16, param, peer, n, nullptr, &factor, stream);
}

int dpwa_factor(const dpwa_interp *cfg, double *clock_dev, const dpwa_header *peer_header_dev, double loss,
                const double *loss_dev, dpwa_coef *coef_dev, dpwa_stream_t stream)
{
    if (!cfg || !clock_dev || !peer_header_dev || !coef_dev) return set_error(DPWA_ERR_ARG, "dpwa_factor: NULL argument");
    if (int rc = check_method(cfg, "dpwa_factor")) return rc;
    FusedArgs fa = stateless_args(cfg, clock_dev, peer_header_dev, loss, coef_dev);
    fa.clock_out = clock_dev;   // the clock moves in place
    fa.loss_d = loss_dev;
    HIP_TRY(launch_factor(fa, (hipStream_t)stream));
    return DPWA_OK;
}

int dpwa_average(int32_t dtype, void *param, const void *peer_slot, int64_t n, const dpwa_interp *cfg,
                 double *clock_dev, double loss, dpwa_coef *coef_dev, void *snap_payload, dpwa_stream_t stream,
                 void *start_event, void *stop_event)
{
    if (!cfg || !clock_dev || !coef_dev || !peer_slot || n < 0 || (n > 0 && !param) || dtype_size(dtype) == 0 ||
        (!start_event) != (!stop_event))
        return set_error(DPWA_ERR_ARG, "dpwa_average: bad arguments");
    if (dtype == DPWA_MIXED)
        return set_error(DPWA_ERR_ARG, "dpwa_average: a DPWA_MIXED payload needs its layout (dpwa_average_mixed)");
    if (int rc = check_method(cfg, "dpwa_average")) return rc;
    const FusedArgs fa = stateless_args(cfg, clock_dev, peer_slot, loss, coef_dev);
    HIP_TRY(launch_average(Elems{dtype, n, nullptr}, param, (const char *)peer_slot + kPayloadOff, fa, snap_payload,
                           (hipStream_t)stream, CallerTiming(start_event, stop_event)));
    return DPWA_OK;
}

static uint32_t layout_fnv(const dpwa_layout &layout)
{
    uint32_t h = 2166136261u;
    auto mix = [&h](uint64_t v, int bytes) {
        for (int k = 0; k < bytes; ++k) {
            h ^= (uint32_t)((v >> (8 * k)) & 0xffu);
            h *= 16777619u;
        }
    };
    for (int i = 0; i < layout.count; ++i) {
        mix((uint64_t)(uint32_t)layout.seg[i].dtype, 4);
        mix((uint64_t)layout.seg[i].byte_offset, 8);
        mix((uint64_t)layout.seg[i].byte_length, 8);
    }
    return h ? h : 1u;
}

int dpwa_layout_digest(const dpwa_layout *layout, int64_t total_bytes, uint32_t *digest)
{
    if (!layout || !digest) return set_error(DPWA_ERR_ARG, "dpwa_layout_digest: NULL argument");
    if (const char *why = layout_problem(*layout, total_bytes)) return set_error(DPWA_ERR_ARG, "dpwa_layout_digest: %s", why);
    *digest = layout_fnv(*layout);
    return DPWA_OK;
}

int dpwa_average_mixed(const dpwa_layout *layout, void *param, const void *peer_slot, const dpwa_interp *cfg,
                       double *clock_dev, double loss, dpwa_coef *coef_dev, void *snap_payload, dpwa_stream_t stream,
                       void *start_event, void *stop_event)
{
    if (!layout || !cfg || !clock_dev || !coef_dev || !peer_slot || !param || (!start_event) != (!stop_event))
        return set_error(DPWA_ERR_ARG, "dpwa_average_mixed: bad arguments");
    if (const char *why = layout_problem(*layout, -1)) return set_error(DPWA_ERR_ARG, "dpwa_average_mixed: %s", why);
    if (!aligned16(param, peer_slot, snap_payload))
        return set_error(DPWA_ERR_ARG, "dpwa_average_mixed: a segmented payload is 16-byte aligned");
    if (int rc = check_method(cfg, "dpwa_average_mixed")) return rc;
    const FusedArgs fa = stateless_args(cfg, clock_dev, peer_slot, loss, coef_dev);
    HIP_TRY(launch_average(Elems{DPWA_MIXED, layout_bytes(*layout), layout}, param, (const char *)peer_slot + kPayloadOff,
                           fa, snap_payload, (hipStream_t)stream, CallerTiming(start_event, stop_event)));
    return DPWA_OK;
}

int dpwa_stream_mix(void *const *dst, int nw, const void *const *src, int nr, int64_t nbytes, dpwa_stream_t stream,
                    void *start_event, void *stop_event)
{
    if (!dst || !src || nr < 1 || nr > 2 || nw < 1 || nw > 2 || nbytes < 0 || (nbytes & 15) ||
        (!start_event) != (!stop_event))
        return set_error(DPWA_ERR_ARG, "dpwa_stream_mix: bad arguments");
    StreamMixArgs a{};
    for (int i = 0; i < nr; ++i) a.src[i] = (const char *)src[i];
    for (int j = 0; j < nw; ++j) a.dst[j] = (char *)dst[j];
    for (int i = 0; i < nr; ++i)
        if (!a.src[i] || !aligned16(a.src[i])) return set_error(DPWA_ERR_ARG, "dpwa_stream_mix: source %d", i);
    for (int j = 0; j < nw; ++j)
        if (!a.dst[j] || !aligned16(a.dst[j])) return set_error(DPWA_ERR_ARG, "dpwa_stream_mix: destination %d", j);
    a.nbytes = nbytes;
    a.nr = nr;
    a.nw = nw;
    HIP_TRY(launch_stream_mix(a, (hipStream_t)stream, CallerTiming(start_event, stop_event)));
    return DPWA_OK;
}

int dpwa_learner_create(dpwa_learner **out, int device, int64_t n, int32_t dtype, const dpwa_interp *cfg)
{
    if (!out || n < 0 || !cfg || dtype_size(dtype) == 0) return set_error(DPWA_ERR_ARG, "dpwa_learner_create: bad arguments");
    if (cfg->method < 0 || cfg->method > 2) return set_error(DPWA_ERR_ARG, "dpwa_learner_create: unknown method");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return set_error(DPWA_ERR_ARG, "dpwa_learner_create: device %d of %d", device, ndev);
    DeviceGuard dg(device);
    dpwa_learner *l = new (std::nothrow) dpwa_learner();
    if (!l) return set_error(DPWA_ERR_NOMEM, "dpwa_learner_create: out of memory");
    l->device = device;
    l->n = n;
    l->dtype = dtype;
    l->cfg = *cfg;
    l->payload_bytes = (size_t)n * dtype_size(dtype);
    l->slot_stride = kPayloadOff + round_up(l->payload_bytes, kPayloadOff);
    // what a learner holds from its creation on (the rest is made at first use); the first failure ends it
    hipError_t e = hipSuccess;
    auto ok = [&e](hipError_t r) { return (e = r) == hipSuccess; };
    if (ok(devmem_alloc(l->slot_mem, 2 * l->slot_stride, device)) && ok(l->side.create()) &&
        ok(l->fetch.init(l->slot_stride, l->side.h)) && ok(l->ctl_mem.alloc(sizeof(Ctl)))) {
        l->ctl = (Ctl *)l->ctl_mem.ptr();
        if (ok(hipMemset(l->slot_mem.ptr, 0, kPayloadOff)) && ok(hipMemset(l->slot_mem.ptr + l->slot_stride, 0, kPayloadOff)) &&
            ok(hipMemset(l->fetch.staging(), 0, kPayloadOff)) && ok(hipMemset(l->ctl, 0, sizeof(Ctl))) &&
            ok(l->published[0].init()) && ok(l->published[1].init()) && ok(l->factor_done.init()) &&
            ok(l->written_through.init()) && ok(l->status.alloc()))
            ok(hipDeviceSynchronize());
    }
    if (e != hipSuccess) {   // the owners give back whatever was made
        int rc = set_error(DPWA_ERR_HIP, "dpwa_learner_create: %s (slot %zu bytes)", hipGetErrorString(e), l->slot_stride);
        dpwa_learner_destroy(l);
        return rc;
    }
    {
        std::lock_guard<std::mutex> g(g_reg_mu);
        g_live.insert(l);
    }
    *out = l;
    return DPWA_OK;
}

int dpwa_learner_destroy(dpwa_learner *l)
{
    if (!l) return DPWA_OK;
    {
        std::lock_guard<std::mutex> g(g_reg_mu);
        g_live.erase(l);
        for (dpwa_learner *o : g_live) {   // forget `l` as a reader of anyone's slot
            std::lock_guard<std::mutex> r(o->readers_mu);
            for (auto &v : o->readers) v.erase(std::remove(v.begin(), v.end(), l), v.end());
        }
    }
    DeviceGuard dg(l->device);
    (void)hipDeviceSynchronize();
    for (auto &kv : l->peers) close_endpoint(kv.second);
    for (char *p : l->relay_opened) (void)hipIpcCloseMemHandle(p);
    delete l;   // every member frees what it owns, on l's device (dg)
    return DPWA_OK;
}

// Local learners that read slot k (two publishes ago) must have finished before it is
// rewritten (WAR); the wait is enqueued on `s` only for readers on another stream.
static int wait_slot_readers(dpwa_learner *l, int k, hipStream_t s)
{
    std::lock_guard<std::mutex> g(l->readers_mu);
    for (dpwa_learner *r : l->readers[k]) {
        if (r->fetch.reads(l, k))
            return set_error(DPWA_ERR_STATE,
                             "a peer still has an unconsumed fetch of the snapshot slot about to be rewritten "
                             "(publish at most once per round)");
        if (r->fetch.consumed_mark().crosses(s)) {
            DeviceGuard rg(r->device);
            HIP_TRY(r->fetch.consumed_mark().order(s));
        }
        if (r->consensus_read.crosses(s)) {   // (never noted by a learner that never called dpwa_learner_consensus)
            DeviceGuard rg(r->device);
            HIP_TRY(r->consensus_read.order(s));
        }
    }
    l->readers[k].clear();
    return DPWA_OK;
}

static int relocate_impl(dpwa_learner *l, hipStream_t s);

// `flat` is in the next publish's slot, written there on `s` (`header`: with its header and clock)
static void set_written_through(dpwa_learner *l, const void *flat, bool header, hipStream_t s)
{
    l->written_through.note(s);
    l->wt_flat = flat;
    l->wt_header = header;
}

// ---------------------------------------------------------------- window guard (resident)
// Between update_send and update_wait resident parameters ARE the snapshot peers read (the
// reference snapshots at update_send, pytorch.py:49-53, so a step in that window never reaches a
// peer there).  The adapter catches optimizer steps by version counter; writes through
// `param.data` move none, so with the reuse guard on every publish runs one small kernel
// (kernels.hip k_window_roll): the payload published last time -- its window closed at the
// average, which wrote the other slot, and nothing writes it again before the average after this
// publish -- is compared with the reuse guard's 4,096 sampled words saved when it was published,
// and the new payload's samples are saved.  A written window is counted on the device and
// mirrored into a host-mapped word; a publish that finds the count grown (never waiting for a
// check) fails with DPWA_ERR_STATE before publishing, and the one after proceeds.  Writes that
// change none of the sampled words are not seen.
static int window_alloc(dpwa_learner *l)
{
    if (l->window.sample.ptr()) return DPWA_OK;
    WindowGuard w;   // built aside: a failure leaves the learner without one, and nothing to free
    hipError_t e = w.sample.alloc(kWindowSampleBytes);
    if (e == hipSuccess) e = w.hits.alloc();
    if (e == hipSuccess) e = w.rolled.init();
    if (e != hipSuccess) return set_error(DPWA_ERR_HIP, "window guard: %s", hipGetErrorString(e));
    l->window = std::move(w);
    return DPWA_OK;
}

// Work on `s` that overwrites slot version % 2 -- the payload the window guard's last roll read
// (the one published before the last publish): an average's write-through store or a relocation --
// runs after that roll when the roll went to another stream.
static int wait_window_roll(dpwa_learner *l, hipStream_t s)
{
    // a null handle counts as "no roll yet": the default stream is indistinguishable from "never"
    if (l->resident && l->window.rolled.stream()) HIP_TRY(l->window.rolled.order(s));
    return DPWA_OK;
}

// One roll on `s`: check the last window (if any), then sample `cur` (if not NULL).
static int window_roll(dpwa_learner *l, const char *cur, hipStream_t s)
{
    if (int rc = window_alloc(l)) return rc;
    if (int rc = wait_window_roll(l, s)) return rc;   // (only a resident learner rolls)
    WindowGuard &w = l->window;
    HIP_TRY(launch_window_roll(w.src, cur, (int64_t)l->payload_bytes, w.sample.ptr(), &l->ctl->window_dirty,
                               &l->ctl->window_hits, w.hits.dev, w.gen, (int32_t)(l->version + 1), s));
    w.rolled.note(s);
    if (cur) {
        w.src = cur;
        w.gen = (int32_t)(l->version + 1);
    }
    return DPWA_OK;
}

// Reports written windows counted since the last report; never waits for a check.
static int window_report(dpwa_learner *l)
{
    WindowGuard &w = l->window;
    if (!w.hits.host()) return DPWA_OK;
    const uint32_t seen = __atomic_load_n(w.hits.host(), __ATOMIC_ACQUIRE);
    if (seen == w.reported) return DPWA_OK;
    const uint32_t newly = seen - w.reported;
    w.reported = seen;
    return set_error(DPWA_ERR_STATE,
                     "resident parameters were written between update_send and update_wait (%u more window(s); "
                     "through param.data, which moves no version counter): peers may have averaged with a partly "
                     "written snapshot. With resident parameters the loop must run update_send -> update_wait -> "
                     "step", newly);
}

static int publish_impl(dpwa_learner *l, const void *flat, double loss, const double *loss_dev, hipStream_t s,
                        bool reuse)
{
    TraceRange tr(reuse ? "dpwa.learner_publish.reuse" : "dpwa.learner_publish");
    l->timing_armed = false;   // armed for the last round's average, which did not happen
    if (l->resident && l->reuse_guard) {   // the window guard's buffers, before anything is queued
        if (int rc = window_alloc(l)) return rc;
    }
    const int k = (int)(l->version % 2);   // slot of publish number version+1
    char *slot = l->slot_mem.ptr + (size_t)k * l->slot_stride;
    if (l->resident) {
        if (int rc = window_report(l)) return rc;
        // the parameters are the payload already: publish the header of the slot they are in
        // (after a publish with no average since, they first move on by one copy)
        if (flat != slot_payload(l, l->res_slot))
            return set_error(DPWA_ERR_ARG, "resident learner: publish the parameters where they are "
                                           "(dpwa_learner_resident_params)");
        if (int rc = relocate_impl(l, s)) return rc;
        flat = slot_payload(l, l->res_slot);
        reuse = true;
    }
    const bool header_only = reuse && l->written_through.noted() && l->wt_flat == flat;
    if (header_only) {
        // the payload was written by the last average (readers of slot k were waited for then);
        // work on `s` after this publish (the next factor reads the clock the average wrote) is
        // ordered after the average
        HIP_TRY(l->written_through.order(s));
        if (l->reuse_guard && !l->resident)
            HIP_TRY(launch_guard_payload(slot + kPayloadOff, flat, (int64_t)l->payload_bytes, &l->ctl->guard_dirty,
                                         &l->ctl->guard_hits, (int32_t)(l->version + 1), s));
        if (l->wt_header) {
            // header and clock of this publish were written by the last average too: nothing
            // moves (IPC-exported slots still get their system-scope write-back)
            if (l->exported) HIP_TRY(launch_release_system(s));
            l->cur = (l->cur + 1) & 3;
        } else {
            HIP_TRY(launch_publish_header(slot, l->n, l->dtype, &l->ctl->clock[l->cur], loss, loss_dev, l->loss_f32,
                                          l->version + 1, l->exported, s));
        }
    } else {
        if (l->resident) return set_error(DPWA_ERR_STATE, "resident learner: parameters not in the next slot");
        if (int rc = wait_slot_readers(l, k, s)) return rc;
        HIP_TRY(launch_publish(slot, flat, (int64_t)l->payload_bytes, l->n, l->dtype, &l->ctl->clock[l->cur], loss,
                               loss_dev, l->loss_f32, l->version + 1, l->exported, s));
    }
    l->written_through.clear();
    l->wt_header = false;
    if (l->resident && l->reuse_guard) {   // the last window's check; this window's samples
        if (int rc = window_roll(l, (const char *)flat, s)) return rc;
    }
    std::lock_guard<std::mutex> g(l->pub_mu);
    l->published[k].note(s);
    l->version++;
    return DPWA_OK;
}

int dpwa_learner_publish(dpwa_learner *l, const void *flat, double loss, const double *loss_dev, dpwa_stream_t stream)
{
    if (!l || (!flat && l->n > 0)) return set_error(DPWA_ERR_ARG, "dpwa_learner_publish: NULL argument");
    DeviceGuard dg(l->device);
    return publish_impl(l, flat, loss, loss_dev, (hipStream_t)stream, false);
}

int dpwa_learner_publish_reuse(dpwa_learner *l, const void *flat, double loss, const double *loss_dev,
                               dpwa_stream_t stream)
{
    if (!l || (!flat && l->n > 0)) return set_error(DPWA_ERR_ARG, "dpwa_learner_publish_reuse: NULL argument");
    DeviceGuard dg(l->device);
    return publish_impl(l, flat, loss, loss_dev, (hipStream_t)stream, true);
}

// A DPWA_MIXED learner averages only once it knows its layout.
static int need_layout(const dpwa_learner *l, const char *fn) { return payload(l).need_layout(fn); }

int dpwa_learner_set_layout(dpwa_learner *l, const dpwa_layout *layout)
{
    if (!l || !layout) return set_error(DPWA_ERR_ARG, "dpwa_learner_set_layout: NULL argument");
    if (l->dtype != DPWA_MIXED)
        return set_error(DPWA_ERR_ARG, "dpwa_learner_set_layout: the learner holds dtype %d, not DPWA_MIXED", l->dtype);
    if (const char *why = layout_problem(*layout, l->n))
        return set_error(DPWA_ERR_ARG, "dpwa_learner_set_layout: %s (%lld payload bytes)", why, (long long)l->n);
    const uint32_t digest = layout_fnv(*layout);
    if (l->layout_digest && l->layout_digest != digest)
        return set_error(DPWA_ERR_STATE, "dpwa_learner_set_layout: the learner already has another layout");
    l->layout = *layout;
    l->layout_digest = digest;
    return DPWA_OK;
}

// The node's forwarder lives here, over the node's public handles: node.cpp is also built against
// a host-only stand-in of the learner (tests/native), which knows no layouts.
int dpwa_node_set_layout(dpwa_node *n, const dpwa_layout *layout)
{
    dpwa_learner *l = nullptr;
    if (!n || dpwa_node_handles(n, &l, nullptr) != DPWA_OK || !l)
        return set_error(DPWA_ERR_STATE, "dpwa_node_set_layout: node not bound");
    return dpwa_learner_set_layout(l, layout);
}

int dpwa_learner_version(const dpwa_learner *l, uint64_t *version)
{
    if (!l || !version) return set_error(DPWA_ERR_ARG, "dpwa_learner_version: NULL argument");
    *version = l->version;
    return DPWA_OK;
}

// peer == l is the self-peer (the learner's own published slot, read like any local peer's)
int dpwa_learner_attach_local(dpwa_learner *l, int peer_id, dpwa_learner *peer)
{
    if (!l || !peer) return set_error(DPWA_ERR_ARG, "dpwa_learner_attach_local: bad peer");
    if (peer->n != l->n || peer->dtype != l->dtype)
        return set_error(DPWA_ERR_ARG, "dpwa_learner_attach_local: peer holds %lld elements of dtype %d, this learner %lld of %d",
                         (long long)peer->n, peer->dtype, (long long)l->n, l->dtype);
    if (peer->layout_digest != l->layout_digest)
        return set_error(DPWA_ERR_ARG, "dpwa_learner_attach_local: peer's layout (digest %08x) is not this learner's (%08x)",
                         peer->layout_digest, l->layout_digest);
    if (peer->device != l->device) {
        DeviceGuard dg(l->device);
        int can = 0;
        HIP_TRY(hipDeviceCanAccessPeer(&can, l->device, peer->device));
        if (!can) return set_error(DPWA_ERR_ARG, "dpwa_learner_attach_local: device %d cannot access device %d", l->device, peer->device);
        hipError_t e = hipDeviceEnablePeerAccess(peer->device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
            return set_error(DPWA_ERR_HIP, "hipDeviceEnablePeerAccess: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        if (peer->slot_mem.vmm()) HIP_TRY(vmm_grant(peer->slot_mem, l->device));   // VMM: per-device access
        peer->exported = true;   // read by another GPU: its publishes release at system scope
    }
    Endpoint ep;
    ep.kind = 1;
    ep.local = peer;
    ep.base = peer->slot_mem.ptr;
    ep.device = peer->device;
    ep.slot_stride = (int64_t)peer->slot_stride;
    ep.n = peer->n;
    ep.dtype = peer->dtype;
    l->peers[peer_id] = std::move(ep);
    return DPWA_OK;
}

static IpcBlob make_blob(const dpwa_learner *l, const DevMem &m, int64_t stride)
{
    IpcBlob b;
    memset(&b, 0, sizeof(b));
    b.magic = kIpcMagic;
    b.slot_stride = stride;
    b.n = l->n;
    b.dtype = l->dtype;
    b.device = l->device;
    b.pid = (int32_t)getpid();
    b.vmm = m.vmm() ? 1 : 0;
    b.layout_digest = (int32_t)l->layout_digest;
    return b;
}

int dpwa_learner_ipc_handle(dpwa_learner *l, void *handle_out, int64_t handle_len)
{
    if (!l || !handle_out || handle_len < (int64_t)sizeof(IpcBlob))
        return set_error(DPWA_ERR_ARG, "dpwa_learner_ipc_handle: need %zu bytes", sizeof(IpcBlob));
    DeviceGuard dg(l->device);
    IpcBlob b = make_blob(l, l->slot_mem, (int64_t)l->slot_stride);
    if (!b.vmm) HIP_TRY(hipIpcGetMemHandle(&b.handle, l->slot_mem.ptr));   // else: fds, dpwa_learner_export_fds
    memset(handle_out, 0, (size_t)handle_len);
    memcpy(handle_out, &b, sizeof(b));
    l->exported = true;   // from now on publishes release at system scope
    return DPWA_OK;
}

int dpwa_learner_export_fds(dpwa_learner *l, int which, int *fds, int max_fds, int *n_fds, int64_t *chunk_bytes)
{
    if (!l || (which != 0 && which != 1) || !n_fds || (max_fds > 0 && !fds) || (which == 1 && !l->relay_on))
        return set_error(DPWA_ERR_ARG, "dpwa_learner_export_fds: bad arguments");
    DeviceGuard dg(l->device);
    const int rc = devmem_export(which == 0 ? l->slot_mem : l->relay_mem, fds, max_fds, n_fds, chunk_bytes);
    if (rc == DPWA_OK) l->exported = true;
    return rc;
}

static int check_blob(const dpwa_learner *l, const void *handle, int64_t handle_len, IpcBlob &b, const char *fn)
{
    if (!handle || handle_len < (int64_t)sizeof(IpcBlob)) return set_error(DPWA_ERR_ARG, "%s: bad handle", fn);
    memcpy(&b, handle, sizeof(b));
    if (b.magic != kIpcMagic) return set_error(DPWA_ERR_ARG, "%s: not a dpwa handle", fn);
    if (b.n != l->n || b.dtype != l->dtype)
        return set_error(DPWA_ERR_ARG, "%s: peer holds %lld elements of dtype %d, this learner %lld of %d", fn,
                         (long long)b.n, b.dtype, (long long)l->n, l->dtype);
    if ((uint32_t)b.layout_digest != l->layout_digest)
        return set_error(DPWA_ERR_ARG, "%s: peer's layout (digest %08x) is not this learner's (%08x)", fn,
                         (uint32_t)b.layout_digest, l->layout_digest);
    return DPWA_OK;
}

static void set_remote(dpwa_learner *l, int peer_id, const IpcBlob &b, char *base, DevMem &&imported)
{
    auto it = l->peers.find(peer_id);
    if (it != l->peers.end()) close_endpoint(it->second);
    Endpoint ep;
    ep.kind = 2;
    ep.base = base;
    ep.device = b.device;
    ep.slot_stride = b.slot_stride;
    ep.n = b.n;
    ep.dtype = b.dtype;
    ep.imported = std::move(imported);
    l->peers[peer_id] = std::move(ep);
}

int dpwa_learner_attach_ipc(dpwa_learner *l, int peer_id, const void *handle, int64_t handle_len)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_attach_ipc: NULL learner");
    IpcBlob b;
    int rc = check_blob(l, handle, handle_len, b, "dpwa_learner_attach_ipc");
    if (rc) return rc;
    if (b.vmm) return set_error(DPWA_ERR_ARG, "dpwa_learner_attach_ipc: the peer shares its slots as fds (dpwa_learner_attach_fds)");
    DeviceGuard dg(l->device);
    void *ptr = nullptr;
    HIP_TRY(hipIpcOpenMemHandle(&ptr, b.handle, hipIpcMemLazyEnablePeerAccess));
    set_remote(l, peer_id, b, (char *)ptr, DevMem());
    return DPWA_OK;
}

int dpwa_learner_attach_fds(dpwa_learner *l, int peer_id, const void *handle, int64_t handle_len, const int *fds,
                            int n_fds, int64_t chunk_bytes)
{
    if (!l || !fds) return set_error(DPWA_ERR_ARG, "dpwa_learner_attach_fds: bad arguments");
    IpcBlob b;
    int rc = check_blob(l, handle, handle_len, b, "dpwa_learner_attach_fds");
    if (rc) return rc;
    if (!b.vmm) return set_error(DPWA_ERR_ARG, "dpwa_learner_attach_fds: the peer shares a hipIpc handle (dpwa_learner_attach_ipc)");
    DeviceGuard dg(l->device);
    DevMem m;
    if ((rc = devmem_import(m, fds, n_fds, chunk_bytes, 2 * (size_t)b.slot_stride, l->device))) return rc;
    char *base = m.ptr;
    set_remote(l, peer_id, b, base, std::move(m));
    return DPWA_OK;
}

int dpwa_learner_fetch(dpwa_learner *l, int peer_id, uint64_t peer_version, int flags, dpwa_stream_t stream)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_fetch: NULL learner");
    auto it = l->peers.find(peer_id);
    if (it == l->peers.end()) return set_error(DPWA_ERR_ARG, "dpwa_learner_fetch: peer %d not attached", peer_id);
    if (peer_version == 0) return set_error(DPWA_ERR_STATE, "dpwa_learner_fetch: peer %d has not published", peer_id);
    Endpoint &ep = it->second;
    if (ep.kind == 1 && !is_live(ep.local)) return set_error(DPWA_ERR_STATE, "dpwa_learner_fetch: peer %d was destroyed", peer_id);
    // The non-finite check of a split round ran in dpwa_learner_factor, on the snapshot then in flight: a lerp
    // with those coefficients against a snapshot that no pass has read could write a NaN the check promises not to
    if (l->finite_check && l->fetch.factored())
        return set_error(DPWA_ERR_STATE, "dpwa_learner_fetch: a factor is computed and the learner skips non-finite peers "
                                         "(dpwa_learner_set_finite_check): lerp or cancel first");
    DeviceGuard dg(l->device);
    hipStream_t s = (hipStream_t)stream;
    const int k = (int)((peer_version - 1) % 2);
    const char *peer_slot = ep.base + (size_t)k * (size_t)ep.slot_stride;
    if (ep.kind == 1) {
        // RAW: the peer's publish of that slot must be complete before anyone reads it.
        dpwa_learner *pl = ep.local;
        if (!pl->published[k].noted()) return set_error(DPWA_ERR_STATE, "dpwa_learner_fetch: peer %d slot %d never published", peer_id, k);
        if (pl->published[k].crosses(s)) {
            DeviceGuard pg(pl->device);
            HIP_TRY(pl->published[k].order(s));
        }
        std::lock_guard<std::mutex> g(ep.local->readers_mu);
        auto &rv = ep.local->readers[k];
        if (std::find(rv.begin(), rv.end(), l) == rv.end()) rv.push_back(l);
    }
    dpwa_learner *const owner = ep.kind == 1 ? ep.local : nullptr;
    const Pull pull{peer_slot, kPayloadOff + round_up(l->payload_bytes, 16), l->pull_mode, l->pull_blocks,
                    ep.kind == 2 || ep.device != l->device};
    if (flags & DPWA_FETCH_RESCUE) return l->fetch.pull_rescue(pull, s, !(flags & DPWA_FETCH_PUBLISHED), owner, k);
    if ((flags & DPWA_FETCH_ZERO_COPY) && ep.kind == 1 && ep.device == l->device) {
        l->fetch.read_in_place(peer_slot, owner, k);
        return DPWA_OK;
    }
    // a staging pull takes the next fetch-timing pair, if one is left
    if ((flags & DPWA_FETCH_PUBLISHED) && ep.kind == 2) return l->fetch.pull_published(pull, l->fetch_times.take(), owner, k);
    return l->fetch.pull_ordered(pull, l->fetch_times.take(), s, owner, k);
}

static int relay_materialize(dpwa_learner *l);

static FusedArgs fused_args(dpwa_learner *l, double loss, const double *loss_dev)
{
    FusedArgs fa{};
    fa.cfg = l->cfg;
    fa.clock_in = &l->ctl->clock[l->cur];
    fa.clock_out = &l->ctl->clock[(l->cur + 1) & 3];
    fa.hdr = (const dpwa_header *)l->fetch.source().ptr;
    fa.loss_h = loss;
    fa.loss_d = loss_dev;
    fa.loss_f32 = l->loss_f32 ? 1 : 0;
    fa.coef_out = &l->ctl->coef;
    fa.status_mirror = l->status.dev;
    if (l->finite_check) {   // a checked round: its stamp, handed to finite_pass and to the factor
        if (++l->finite_stamp == 0) l->finite_stamp = 1;
        fa.veto = &l->ctl->finite_veto;
        fa.stamp = l->finite_stamp;
        fa.skips = &l->ctl->finite_skips;
    }
    return fa;
}

// The non-finite check of a checked round (fa.veto set): one read of the fetched peer payload on `s`, behind
// fetch.wait_landed and before the round's factor, average and distance passes.
static int finite_pass(dpwa_learner *l, const FusedArgs &fa, const void *peer, hipStream_t s)
{
    if (!fa.veto) return DPWA_OK;
    HIP_TRY(launch_peer_finite(payload(l), peer, &l->ctl->finite_veto, fa.stamp, s));
    return DPWA_OK;
}

int dpwa_learner_factor(dpwa_learner *l, double loss, const double *loss_dev, dpwa_stream_t stream)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_factor: NULL learner");
    if (!l->fetch.fetched()) return set_error(DPWA_ERR_STATE, "dpwa_learner_factor: no fetch in flight");
    if (l->fetch.factored()) return set_error(DPWA_ERR_STATE, "dpwa_learner_factor: factor already computed for this fetch");
    if (int rc = need_layout(l, "dpwa_learner_factor")) return rc;
    DeviceGuard dg(l->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = relay_materialize(l)) return rc;
    HIP_TRY(l->fetch.wait_landed(s));
    const FusedArgs fa = fused_args(l, loss, loss_dev);
    if (int rc = finite_pass(l, fa, l->fetch.source().ptr + kPayloadOff, s)) return rc;
    HIP_TRY(launch_factor(fa, s));
    HIP_TRY(l->factor_done.record(s));
    HIP_TRY(l->fetch.factored_on(s));   // the header has been read on s: a later pull into this buffer waits for it
    l->cur = (l->cur + 1) & 3;
    // A header that a write-through average wrote ahead carries that average's clock, and the clock it
    // wrote ahead lay in the ring place this factor has just written: the next publish writes both anew
    l->wt_header = false;   // (as dpwa_learner_write_clock does, for the same reason)
    return DPWA_OK;
}

int dpwa_learner_lerp(dpwa_learner *l, void *flat, dpwa_stream_t stream)
{
    if (!l || (!flat && l->n > 0)) return set_error(DPWA_ERR_ARG, "dpwa_learner_lerp: NULL argument");
    if (!l->fetch.factored()) return set_error(DPWA_ERR_STATE, "dpwa_learner_lerp: no factor computed for this fetch");
    if (l->resident)
        return set_error(DPWA_ERR_STATE, "dpwa_learner_lerp: a resident learner averages with dpwa_learner_average");
    DeviceGuard dg(l->device);
    hipStream_t s = (hipStream_t)stream;
    if (l->dtype == DPWA_MIXED && !aligned16(flat))   // (its layout is known: the factor was computed)
        return set_error(DPWA_ERR_ARG, "dpwa_learner_lerp: a segmented payload is 16-byte aligned");
    if (int rc = l->measure.operands_problem("dpwa_learner_lerp", flat)) return rc;
    const Measured m{&l->measure, payload(l), flat, l->fetch.source().ptr + kPayloadOff, nullptr};
    int rc = measured_average(&m, 1, s, [&]() -> int {
        HIP_TRY(launch_lerp(m.p, flat, m.peer, m.p.coef, 0.f, 0.f, s));
        return DPWA_OK;
    });
    if (rc) return rc;
    HIP_TRY(l->fetch.note_consumed(s));
    l->written_through.clear();
    l->fetch.finish();
    return DPWA_OK;
}

// One fused average, split so that several learners' averages can share a dispatch:
// average_prepare orders `s` after everything the kernel reads or overwrites and builds its
// arguments; the caller launches; average_commit does the learner's bookkeeping.
struct AvgPlan {
    void *flat = nullptr;
    const char *peer = nullptr;   // payload averaged with (contiguous source)
    char *snap = nullptr;         // write-through destination
    FusedArgs fa{};
    bool relay = false;           // the relay's phase 2 fused into this average (k_lerp_relay)
    bool write_through = false;
    bool oop = false;             // resident: the result goes to `snap` only
    int snap_slot = -1;
};

static int average_prepare(dpwa_learner *l, void *flat, double loss, const double *loss_dev, hipStream_t s,
                           bool write_through, AvgPlan &p)
{
    if (!l->fetch.fetched() || l->fetch.factored()) return set_error(DPWA_ERR_STATE, "dpwa_learner_average: no fetch in flight");
    if (int rc = need_layout(l, "dpwa_learner_average")) return rc;
    if (l->dtype == DPWA_MIXED && !aligned16(flat))
        return set_error(DPWA_ERR_ARG, "dpwa_learner_average: a segmented payload is 16-byte aligned");
    if (int rc = l->measure.operands_problem("dpwa_learner_average", flat)) return rc;
    p = AvgPlan();
    if (l->resident) {   // read where the parameters are (the published slot), write the next slot
        if (flat != slot_payload(l, l->res_slot))
            return set_error(DPWA_ERR_ARG, "resident learner: average the parameters where they are "
                                           "(dpwa_learner_resident_params)");
        write_through = true;
        p.oop = true;
    }
    p.flat = flat;
    p.write_through = write_through;
    p.fa = fused_args(l, loss, loss_dev);
    if (write_through) {
        const int k = (int)(l->version % 2);   // slot of the next publish
        if (int rc = wait_slot_readers(l, k, s)) return rc;
        if (int rc = wait_window_roll(l, s)) return rc;
        p.snap = slot_payload(l, k);
        p.snap_slot = k;
        if (l->cfg.method != DPWA_INTERP_LOSS && !l->header_on_publish) {   // peers never read this header's loss
            p.fa.next_header = (dpwa_header *)(p.snap - kPayloadOff);
            p.fa.clock_next = &l->ctl->clock[(l->cur + 2) & 3];
            p.fa.next_version = l->version + 1;
            p.fa.n = l->n;
            p.fa.dtype = l->dtype;
        }
    }
    if (l->relay_deferred && aligned16(flat, p.snap)) {
        // the relay's phase 2 fused into the average: stripes read where phase 1 left them
        const RelayArgs &a = l->relay_saved;
        p.fa.hdr = (const dpwa_header *)(a.slots[l->relay_saved_pick] + a.slot_off);
        p.relay = true;
    } else {
        if (int rc = relay_materialize(l)) return rc;
        p.peer = l->fetch.source().ptr + kPayloadOff;
    }
    HIP_TRY(l->fetch.wait_landed(s));
    return DPWA_OK;
}

static const LaunchTiming *take_timing(dpwa_learner *l)
{
    return l->timing_armed ? l->avg_times.take() : nullptr;
}

static int average_commit(dpwa_learner *l, const AvgPlan &p, hipStream_t s)
{
    if (p.relay) {
        HIP_TRY(l->relay_done.record(s));   // the next round's barrier waits for these reads
        l->relay_deferred = false;
        l->fetch.note_consumed_in_place(s);
    } else {
        HIP_TRY(l->fetch.note_consumed(s));
    }
    l->timing_armed = false;
    l->cur = (l->cur + 1) & 3;
    if (p.oop) l->res_slot = p.snap_slot;   // the parameters moved into the next publish's slot
    set_written_through(l, p.oop ? p.snap : p.flat, p.fa.next_header != nullptr, s);
    if (!p.write_through) l->written_through.clear();
    l->fetch.finish();
    return DPWA_OK;
}

// The averaging launch of plan p with the learner's measurements around it (measured_average); a
// fused whole-model record gets the tracked kernel in its place.
static int average_launch(dpwa_learner *l, const AvgPlan &p, hipStream_t s)
{
    // (the unaligned launch_average is not timed; p.relay: relay_phase2 refuses to defer for a
    // segmented payload or a measuring learner)
    const Payload e = payload(l);
    const LaunchTiming *timing = e.segmented() || p.relay || aligned16(p.flat) ? take_timing(l) : nullptr;
    if (int rc = finite_pass(l, p.fa, p.peer, s)) return rc;   // (never with p.relay: relay_phase2 refuses)
    const Measured m{&l->measure, e, p.flat, p.peer, p.snap, &p.fa, p.oop, timing};
    return measured_average(&m, 1, s, [&]() -> int {
        if (p.relay) {   // (never a segmented payload: relay_phase2 refuses)
            HIP_TRY(launch_average_relay(l->dtype, p.flat, l->n, p.fa, p.snap, l->relay_saved, l->relay_saved_pick, s,
                                         timing, p.oop));
        } else {
            HIP_TRY(launch_average(e, p.flat, p.peer, p.fa, p.snap, s, timing, p.oop));
        }
        return DPWA_OK;
    });
}

static int average_impl(dpwa_learner *l, void *flat, double loss, const double *loss_dev, hipStream_t s,
                        bool write_through)
{
    TraceRange tr("dpwa.average");
    AvgPlan p;
    if (int rc = average_prepare(l, flat, loss, loss_dev, s, write_through, p)) return rc;
    if (int rc = average_launch(l, p, s)) return rc;
    return average_commit(l, p, s);
}

// Can plan p join a batched dispatch (k_lerp_batch)?  Contiguous source, 16-B aligned operands, one
// element type (a segmented payload is not batched).
static bool batchable(const dpwa_learner *l, const AvgPlan &p)
{
    return !p.relay && !payload(l).segmented() && aligned16(p.flat, p.peer, p.snap);
}

// Launches the batchable plans in groups of the same (dtype, write-through), up to
// kMaxAvgBatch per dispatch, and every other plan on its own.  Timed like a single average:
// the first armed learner of a dispatch lends it its timing pair.
static int launch_plans(dpwa_learner *const *ls, const AvgPlan *plans, const int *idx, int count, hipStream_t s)
{
    std::vector<char> done((size_t)count, 0);
    for (int a = 0; a < count; ++a) {
        if (done[a]) continue;
        const int ia = idx[a];
        dpwa_learner *la = ls[ia];
        const AvgPlan &pa = plans[ia];
        done[a] = 1;
        if (!batchable(la, pa)) {
            int rc = average_launch(la, pa, s);
            if (rc) return rc;
            continue;
        }
        AvgBatch b{};
        const LaunchTiming *timing = take_timing(la);
        Measured member[kMaxAvgBatch];   // the dispatch stays as it is: their measurements go around it
        dpwa_learner *checker[kMaxAvgBatch];
        auto add = [&](dpwa_learner *l, const AvgPlan &p) {
            checker[b.count] = l;
            member[b.count] = Measured{&l->measure, payload(l), p.flat, p.peer, p.snap};
            AvgEntry &e = b.e[b.count++];
            e.param = p.flat;
            e.peer = p.peer;
            e.snap = p.snap;
            e.n = l->n;
            e.fa = p.fa;
        };
        add(la, pa);
        for (int c = a + 1; c < count && b.count < kMaxAvgBatch; ++c) {
            const int ic = idx[c];
            if (done[c] || !batchable(ls[ic], plans[ic]) || ls[ic]->dtype != la->dtype ||
                plans[ic].write_through != pa.write_through || plans[ic].oop != pa.oop)
                continue;
            if (!timing) timing = take_timing(ls[ic]);
            add(ls[ic], plans[ic]);
            done[c] = 1;
        }
        for (int i = 0; i < b.count; ++i)   // each checking member's snapshot, before anything of the dispatch
            if (int rc = finite_pass(checker[i], b.e[i].fa, b.e[i].peer, s)) return rc;
        int rc = measured_average(member, b.count, s, [&]() -> int {
            HIP_TRY(launch_average_batch(la->dtype, pa.write_through, b, s, timing, pa.oop));
            return DPWA_OK;
        });
        if (rc) return rc;
    }
    return DPWA_OK;
}

int dpwa_learner_average(dpwa_learner *l, void *flat, double loss, const double *loss_dev, dpwa_stream_t stream)
{
    if (!l || (!flat && l->n > 0)) return set_error(DPWA_ERR_ARG, "dpwa_learner_average: NULL argument");
    DeviceGuard dg(l->device);
    return average_impl(l, flat, loss, loss_dev, (hipStream_t)stream, false);
}

int dpwa_learner_average_through(dpwa_learner *l, void *flat, double loss, const double *loss_dev,
                                 dpwa_stream_t stream)
{
    if (!l || (!flat && l->n > 0)) return set_error(DPWA_ERR_ARG, "dpwa_learner_average_through: NULL argument");
    DeviceGuard dg(l->device);
    return average_impl(l, flat, loss, loss_dev, (hipStream_t)stream, true);
}

int dpwa_learner_average_many(dpwa_learner *const *ls, void *const *flats, const double *loss,
                              const double *const *loss_dev, const int *write_through, int count, dpwa_stream_t stream)
{
    if (count < 0 || (count > 0 && (!ls || !flats || !loss || !write_through)))
        return set_error(DPWA_ERR_ARG, "dpwa_learner_average_many: bad arguments");
    if (count == 0) return DPWA_OK;
    for (int i = 0; i < count; ++i) {
        if (!ls[i] || (!flats[i] && ls[i]->n > 0))
            return set_error(DPWA_ERR_ARG, "dpwa_learner_average_many: NULL learner or buffer at %d", i);
        if (ls[i]->device != ls[0]->device)
            return set_error(DPWA_ERR_ARG, "dpwa_learner_average_many: learners on devices %d and %d share one stream",
                             ls[0]->device, ls[i]->device);
        for (int j = 0; j < i; ++j)
            if (ls[j] == ls[i]) return set_error(DPWA_ERR_ARG, "dpwa_learner_average_many: learner %d given twice", i);
    }
    DeviceGuard dg(ls[0]->device);
    hipStream_t s = (hipStream_t)stream;
    std::vector<AvgPlan> plans((size_t)count);
    std::vector<int> idx;
    idx.reserve((size_t)count);
    for (int i = 0; i < count; ++i) {
        int rc = average_prepare(ls[i], flats[i], loss[i], loss_dev ? loss_dev[i] : nullptr, s, write_through[i] != 0,
                                 plans[i]);
        if (rc) return rc;   // nothing launched yet for this learner; earlier ones are prepared only
        idx.push_back(i);
    }
    int rc = launch_plans(ls, plans.data(), idx.data(), count, s);
    if (rc) return rc;
    for (int i = 0; i < count; ++i)
        if ((rc = average_commit(ls[i], plans[i], s))) return rc;
    return DPWA_OK;
}

static int average_many_impl(const char *fn, int32_t dtype, const dpwa_average_desc *descs, int count,
                             const dpwa_interp *cfg, dpwa_stream_t stream, void *start_event, void *stop_event,
                             bool oop)
{
    if (count < 1 || count > kMaxAvgBatch || !descs || !cfg || dtype_size(dtype) == 0 || (!start_event) != (!stop_event))
        return set_error(DPWA_ERR_ARG, "%s: bad arguments (1..%d descriptors)", fn, kMaxAvgBatch);
    if (dtype == DPWA_MIXED) return set_error(DPWA_ERR_ARG, "%s: segmented (DPWA_MIXED) payloads are not batched", fn);
    if (int rc = check_method(cfg, fn)) return rc;
    AvgBatch b{};
    bool dual = oop;   // an empty entry may pass no buffers at all
    for (int i = 0; i < count; ++i) dual = dual || descs[i].snap_payload != nullptr;
    for (int i = 0; i < count; ++i) {
        const dpwa_average_desc &d = descs[i];
        if ((!d.param && d.n > 0) || !d.peer_slot || !d.clock_dev || !d.coef_dev || d.n < 0 ||
            (d.snap_payload == nullptr && d.n > 0 && dual) ||
            !aligned16(d.param, d.peer_slot, d.snap_payload))
            return set_error(DPWA_ERR_ARG, "%s: descriptor %d: NULL, unaligned or mixed write-through", fn, i);
        AvgEntry &e = b.e[b.count++];
        e.param = d.param;
        e.peer = (const char *)d.peer_slot + kPayloadOff;
        e.snap = d.snap_payload;
        e.n = d.n;
        e.fa = stateless_args(cfg, d.clock_dev, d.peer_slot, d.loss, d.coef_dev);
    }
    const CallerTiming timing(start_event, stop_event);
    if (oop && count == 1) {   // one resident average: the single kernel, as a resident learner runs it
        const AvgEntry &e = b.e[0];
        HIP_TRY(launch_average(Elems{dtype, e.n, nullptr}, e.param, e.peer, e.fa, e.snap, (hipStream_t)stream, timing, true));
        return DPWA_OK;
    }
    HIP_TRY(launch_average_batch(dtype, dual, b, (hipStream_t)stream, timing, oop));
    return DPWA_OK;
}

int dpwa_average_many(int32_t dtype, const dpwa_average_desc *descs, int count, const dpwa_interp *cfg,
                      dpwa_stream_t stream, void *start_event, void *stop_event)
{
    return average_many_impl("dpwa_average_many", dtype, descs, count, cfg, stream, start_event, stop_event, false);
}

int dpwa_average_many_resident(int32_t dtype, const dpwa_average_desc *descs, int count, const dpwa_interp *cfg,
                               dpwa_stream_t stream, void *start_event, void *stop_event)
{
    return average_many_impl("dpwa_average_many_resident", dtype, descs, count, cfg, stream, start_event, stop_event,
                             true);
}

int dpwa_learner_set_distance(dpwa_learner *l, int on)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_set_distance: NULL learner");
    DeviceGuard dg(l->device);
    return l->measure.set_whole("dpwa_learner_set_distance", on != 0, l->relay_deferred);
}

int dpwa_learner_set_finite_check(dpwa_learner *l, int on)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_set_finite_check: NULL learner");
    if (on && l->relay_deferred)
        return set_error(DPWA_ERR_STATE, "dpwa_learner_set_finite_check: a fused relay second phase is pending "
                                         "(dpwa_learner_relay_phase2 with fuse != 0), which reads no contiguous peer "
                                         "snapshot to check");
    // (coefficients computed while the check was off come from no pass: the lerp they belong to would go unchecked)
    if (on && l->fetch.factored())
        return set_error(DPWA_ERR_STATE, "dpwa_learner_set_finite_check: a factor is computed for the fetch in flight: "
                                         "lerp or cancel first");
    l->finite_check = on != 0;
    return DPWA_OK;
}

// (Here and not in node.cpp: the node's host-only stand-in learner of tests/native has no such entry.)
int dpwa_node_set_finite_check(dpwa_node *n, int on)
{
    dpwa_learner *l = nullptr;
    if (!n || dpwa_node_handles(n, &l, nullptr) || !l)
        return set_error(DPWA_ERR_STATE, "dpwa_node_set_finite_check: node not bound");
    return dpwa_learner_set_finite_check(l, on);
}

int dpwa_learner_finite_skips(dpwa_learner *l, uint64_t *count)
{
    if (!l || !count) return set_error(DPWA_ERR_ARG, "dpwa_learner_finite_skips: NULL argument");
    DeviceGuard dg(l->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(count, &l->ctl->finite_skips, sizeof(uint64_t), hipMemcpyDeviceToHost));
    return DPWA_OK;
}

int dpwa_learner_distance(dpwa_learner *l, const dpwa_distance **dev)
{
    if (!l || !dev) return set_error(DPWA_ERR_ARG, "dpwa_learner_distance: NULL argument");
    if (!l->measure.record())
        return set_error(DPWA_ERR_STATE, "dpwa_learner_distance: distance tracking was never switched on "
                                         "(dpwa_learner_set_distance)");
    *dev = l->measure.record();
    return DPWA_OK;
}

int dpwa_learner_set_param_distance(dpwa_learner *l, const dpwa_param_range *ranges, int64_t count, int every)
{
    const char *fn = "dpwa_learner_set_param_distance";
    if (!l) return set_error(DPWA_ERR_ARG, "%s: NULL learner", fn);
    DeviceGuard dg(l->device);
    return l->measure.set_param(fn, ranges, count, every, payload(l), l->relay_deferred);
}

int dpwa_learner_param_distance(dpwa_learner *l, const dpwa_param_distance_head **dev, int64_t *count)
{
    if (!l || !dev || !count) return set_error(DPWA_ERR_ARG, "dpwa_learner_param_distance: NULL argument");
    if (!l->measure.param_record())
        return set_error(DPWA_ERR_STATE, "dpwa_learner_param_distance: the per-parameter distance was never switched on "
                                         "(dpwa_learner_set_param_distance)");
    *dev = l->measure.param_record();
    *count = l->measure.param_count();
    return DPWA_OK;
}

int dpwa_learner_param_distance_rounds(dpwa_learner *l, int64_t *averaged, int64_t *measured)
{
    if (!l || !averaged || !measured) return set_error(DPWA_ERR_ARG, "dpwa_learner_param_distance_rounds: NULL argument");
    *averaged = l->measure.rounds();
    *measured = l->measure.measured();
    return DPWA_OK;
}

int dpwa_learner_set_header_publish(dpwa_learner *l, int always)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_set_header_publish: NULL learner");
    l->header_on_publish = always != 0;
    return DPWA_OK;
}

int dpwa_learner_set_reuse_guard(dpwa_learner *l, int on)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_set_reuse_guard: NULL learner");
    l->reuse_guard = on != 0;
    l->window.src = nullptr;   // a resident learner's window guard starts afresh at the next publish
    return DPWA_OK;
}

// Moves resident parameters from the published slot into the next publish's slot (a round
// without an average; two publishes in a row).  No-op when they are there already.
static int relocate_impl(dpwa_learner *l, hipStream_t s)
{
    const int k = (int)(l->version % 2);
    if (!l->resident || l->res_slot == k) return DPWA_OK;
    if (int rc = wait_slot_readers(l, k, s)) return rc;
    if (int rc = wait_window_roll(l, s)) return rc;
    HIP_TRY(launch_copy_payload(slot_payload(l, k), slot_payload(l, l->res_slot), (int64_t)l->payload_bytes, s));
    l->res_slot = k;
    set_written_through(l, slot_payload(l, k), false, s);   // the publish writes the header (the clock did not move)
    return DPWA_OK;
}

int dpwa_learner_set_resident(dpwa_learner *l, const void *init, dpwa_stream_t stream)
{
    if (!l || (!init && l->n > 0)) return set_error(DPWA_ERR_ARG, "dpwa_learner_set_resident: NULL argument");
    if (l->resident) return set_error(DPWA_ERR_STATE, "dpwa_learner_set_resident: already resident");
    if (l->version != 0 || l->fetch.fetched())
        return set_error(DPWA_ERR_STATE, "dpwa_learner_set_resident: only before the first publish");
    DeviceGuard dg(l->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = wait_slot_readers(l, 0, s)) return rc;
    char *dst = slot_payload(l, 0);
    if (l->payload_bytes && dst != init)
        HIP_TRY(hipMemcpyAsync(dst, init, l->payload_bytes, hipMemcpyDeviceToDevice, s));
    l->resident = true;
    l->res_slot = 0;
    set_written_through(l, dst, false, s);
    return DPWA_OK;
}

int dpwa_learner_resident_params(dpwa_learner *l, void **params, int *slot)
{
    if (!l || !params) return set_error(DPWA_ERR_ARG, "dpwa_learner_resident_params: NULL argument");
    *params = l->resident ? (void *)slot_payload(l, l->res_slot) : nullptr;
    if (slot) *slot = l->resident ? l->res_slot : -1;
    return DPWA_OK;
}

int dpwa_learner_relocate(dpwa_learner *l, dpwa_stream_t stream)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_relocate: NULL learner");
    if (l->fetch.fetched()) return set_error(DPWA_ERR_STATE, "dpwa_learner_relocate: a fetch is in flight (average it)");
    DeviceGuard dg(l->device);
    return relocate_impl(l, (hipStream_t)stream);
}

int dpwa_learner_window_hits(dpwa_learner *l, uint32_t *hits)
{
    if (!l || !hits) return set_error(DPWA_ERR_ARG, "dpwa_learner_window_hits: NULL argument");
    DeviceGuard dg(l->device);
    *hits = 0;
    WindowGuard &w = l->window;
    if (!w.sample.ptr()) return DPWA_OK;
    if (w.src) {   // check the window open now (or closed, not yet checked); keep its samples
        hipStream_t s = w.rolled.stream();
        HIP_TRY(launch_window_roll(w.src, nullptr, (int64_t)l->payload_bytes, w.sample.ptr(), &l->ctl->window_dirty,
                                   &l->ctl->window_hits, w.hits.dev, w.gen, 0, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    *hits = __atomic_load_n(w.hits.host(), __ATOMIC_ACQUIRE);
    return DPWA_OK;
}

int dpwa_learner_reuse_guard_hits(dpwa_learner *l, uint32_t *hits)
{
    if (!l || !hits) return set_error(DPWA_ERR_ARG, "dpwa_learner_reuse_guard_hits: NULL argument");
    DeviceGuard dg(l->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hits, &l->ctl->guard_hits, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DPWA_OK;
}

int dpwa_learner_read_snapshot(dpwa_learner *l, void *header_out, void *payload_out, int64_t payload_bytes,
                               uint64_t *version_out)
{
    if (!l || !header_out || !version_out || payload_bytes < 0 || (payload_bytes > 0 && !payload_out))
        return set_error(DPWA_ERR_ARG, "dpwa_learner_read_snapshot: bad arguments");
    if ((size_t)payload_bytes > l->payload_bytes) payload_bytes = (int64_t)l->payload_bytes;
    DeviceGuard dg(l->device);
    for (int attempt = 0; attempt < 8; ++attempt) {
        uint64_t v;
        int k;
        {
            std::lock_guard<std::mutex> g(l->pub_mu);
            v = l->version;
            if (v == 0) {
                *version_out = 0;
                return DPWA_OK;   // nothing published: the reference replies without state
            }
            k = (int)((v - 1) % 2);
            if (!l->read_stream.h) {   // created at the first host read: no stream (and no hardware
                                       // queue share) for learners nobody reads over the wire
                HIP_TRY(l->ev_read.init());
                HIP_TRY(l->read_stream.create());
            }
            // order after the publish (and everything before it) on the publisher's stream
            HIP_TRY(hipEventRecord(l->ev_read.h, l->published[k].stream()));
        }
        hipStream_t rs = l->read_stream.h;
        HIP_TRY(hipStreamWaitEvent(rs, l->ev_read.h, 0));
        const char *slot = l->slot_mem.ptr + (size_t)k * l->slot_stride;
        HIP_TRY(hipMemcpyAsync(header_out, slot, kHeader, hipMemcpyDeviceToHost, rs));
        if (payload_bytes)
            HIP_TRY(hipMemcpyAsync(payload_out, slot + kPayloadOff, (size_t)payload_bytes, hipMemcpyDeviceToHost,
                                   rs));
        HIP_TRY(hipStreamSynchronize(rs));
        // a slot is rewritten two publishes later: if that happened meanwhile, read again
        std::lock_guard<std::mutex> g(l->pub_mu);
        if (l->version < v + 2 && ((const dpwa_header *)header_out)->version == v) {
            *version_out = v;
            return DPWA_OK;
        }
    }
    return set_error(DPWA_ERR_STATE, "dpwa_learner_read_snapshot: publishes outran the reader");
}

int dpwa_learner_fetch_host(dpwa_learner *l, const void *header, const void *payload, int64_t payload_bytes,
                            dpwa_stream_t stream)
{
    if (!l || !header || payload_bytes != (int64_t)l->payload_bytes || (payload_bytes > 0 && !payload))
        return set_error(DPWA_ERR_ARG, "dpwa_learner_fetch_host: need a header and %zu payload bytes",
                         l ? l->payload_bytes : (size_t)0);
    DeviceGuard dg(l->device);
    (void)stream;
    // The copy waits only for the last reader of the staging buffer (every consumer of a fetch
    // records stage_done), not for all the work queued on the caller's stream: it starts
    // at once, beside a training step already enqueued.
    hipStream_t side = l->side.h;
    HIP_TRY(l->fetch.staging_writable());
    // Pageable host sources: the calls return once the host bytes have been taken.  A
    // page-locked source is copied asynchronously, so the copy is waited for: either way the
    // caller may reuse its buffer when this returns.
    hipPointerAttribute_t attr{};
    const bool pinned = payload_bytes > 0 && hipPointerGetAttributes(&attr, payload) == hipSuccess &&
                        attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();   // a pageable pointer is "invalid" to hipPointerGetAttributes
    HIP_TRY(hipMemcpyAsync(l->fetch.staging(), header, kHeader, hipMemcpyHostToDevice, side));
    if (payload_bytes)
        HIP_TRY(hipMemcpyAsync(l->fetch.staging() + kPayloadOff, payload, (size_t)payload_bytes, hipMemcpyHostToDevice, side));
    HIP_TRY(l->fetch.landed_on_side());
    if (pinned) HIP_TRY(l->fetch.host_wait_landed());
    l->fetch.arrived_in_staging();
    return DPWA_OK;
}

int dpwa_learner_relay_enable(dpwa_learner *l, int world, int rank)
{
    if (!l || world < 2 || world > kMaxRelayRanks || rank < 0 || rank >= world)
        return set_error(DPWA_ERR_ARG, "dpwa_learner_relay_enable: bad world/rank");
    if (l->relay_on) return set_error(DPWA_ERR_STATE, "dpwa_learner_relay_enable: already enabled");
    DeviceGuard dg(l->device);
    const int64_t payload16 = (int64_t)round_up(l->payload_bytes, 16);
    l->relay_stripe = (int64_t)round_up((size_t)((payload16 + world - 1) / world), kPayloadOff);
    HIP_TRY(devmem_alloc(l->relay_mem, (size_t)l->relay_stripe * world, l->device));
    HIP_TRY(l->relay_done.init());
    l->relay_world = world;
    l->relay_rank = rank;
    l->relay_slots.assign((size_t)world, nullptr);
    l->relay_bufs.assign((size_t)world, nullptr);
    l->relay_slots[rank] = l->slot_mem.ptr;
    l->relay_bufs[rank] = l->relay_mem.ptr;
    l->relay_on = true;
    return DPWA_OK;
}

int dpwa_learner_relay_handle(dpwa_learner *l, void *handle_out, int64_t handle_len)
{
    if (!l || !l->relay_on || !handle_out || handle_len < (int64_t)sizeof(IpcBlob))
        return set_error(DPWA_ERR_ARG, "dpwa_learner_relay_handle: relay not enabled or short buffer");
    DeviceGuard dg(l->device);
    IpcBlob b = make_blob(l, l->relay_mem, l->relay_stripe);
    if (!b.vmm) HIP_TRY(hipIpcGetMemHandle(&b.handle, l->relay_mem.ptr));
    memset(handle_out, 0, (size_t)handle_len);
    memcpy(handle_out, &b, sizeof(b));
    l->exported = true;
    return DPWA_OK;
}

static int relay_check(dpwa_learner *l, int rank, int peer_id, const void *relay_handle, int64_t handle_len,
                       IpcBlob &b, Endpoint *&slots_ep, const char *fn)
{
    if (!l || !l->relay_on || rank < 0 || rank >= l->relay_world || rank == l->relay_rank || !relay_handle ||
        handle_len < (int64_t)sizeof(IpcBlob))
        return set_error(DPWA_ERR_ARG, "%s: bad arguments", fn);
    auto it = l->peers.find(peer_id);
    if (it == l->peers.end() || it->second.kind != 2)
        return set_error(DPWA_ERR_STATE, "%s: peer %d's slots are not IPC-attached", fn, peer_id);
    memcpy(&b, relay_handle, sizeof(b));
    if (b.magic != kIpcMagic || b.slot_stride != l->relay_stripe || b.n != l->n || b.dtype != l->dtype)
        return set_error(DPWA_ERR_ARG, "%s: relay buffer of rank %d does not match", fn, rank);
    slots_ep = &it->second;
    return DPWA_OK;
}

int dpwa_learner_relay_attach(dpwa_learner *l, int rank, int peer_id, const void *relay_handle, int64_t handle_len)
{
    IpcBlob b;
    Endpoint *ep = nullptr;
    int rc = relay_check(l, rank, peer_id, relay_handle, handle_len, b, ep, "dpwa_learner_relay_attach");
    if (rc) return rc;
    if (b.vmm) return set_error(DPWA_ERR_ARG, "dpwa_learner_relay_attach: rank %d shares its relay buffer as fds", rank);
    DeviceGuard dg(l->device);
    void *ptr = nullptr;
    HIP_TRY(hipIpcOpenMemHandle(&ptr, b.handle, hipIpcMemLazyEnablePeerAccess));
    l->relay_opened.push_back((char *)ptr);
    l->relay_slots[rank] = ep->base;
    l->relay_bufs[rank] = (const char *)ptr;
    return DPWA_OK;
}

int dpwa_learner_relay_attach_fds(dpwa_learner *l, int rank, int peer_id, const void *relay_handle,
                                  int64_t handle_len, const int *fds, int n_fds, int64_t chunk_bytes)
{
    IpcBlob b;
    Endpoint *ep = nullptr;
    int rc = relay_check(l, rank, peer_id, relay_handle, handle_len, b, ep, "dpwa_learner_relay_attach_fds");
    if (rc) return rc;
    if (!b.vmm || !fds) return set_error(DPWA_ERR_ARG, "dpwa_learner_relay_attach_fds: rank %d shares a hipIpc handle", rank);
    DeviceGuard dg(l->device);
    DevMem m;
    if ((rc = devmem_import(m, fds, n_fds, chunk_bytes, (size_t)l->relay_stripe * l->relay_world, l->device))) return rc;
    l->relay_slots[rank] = ep->base;
    l->relay_bufs[rank] = m.ptr;
    l->relay_imported.push_back(std::move(m));
    return DPWA_OK;
}

static int relay_args(dpwa_learner *l, const int32_t *picks_dev, uint64_t version, RelayArgs &a)
{
    for (int r = 0; r < l->relay_world; ++r)
        if (!l->relay_slots[r] || !l->relay_bufs[r])
            return set_error(DPWA_ERR_STATE, "relay: rank %d not attached", r);
    if (version == 0) return set_error(DPWA_ERR_STATE, "relay: nothing published");
    memset(&a, 0, sizeof(a));
    for (int r = 0; r < l->relay_world; ++r) {
        a.slots[r] = l->relay_slots[r];
        a.relays[r] = l->relay_bufs[r];
    }
    a.relay_mine = l->relay_mem.ptr;
    a.staging = l->fetch.staging();
    a.picks = picks_dev;
    a.slot_off = (int64_t)((version - 1) % 2) * (int64_t)l->slot_stride;
    a.stripe = l->relay_stripe;
    a.payload = (int64_t)round_up(l->payload_bytes, 16);
    a.world = l->relay_world;
    a.rank = l->relay_rank;
    return DPWA_OK;
}

int dpwa_learner_relay_wait(dpwa_learner *l, dpwa_stream_t stream)
{
    if (!l || !l->relay_on) return set_error(DPWA_ERR_STATE, "dpwa_learner_relay_wait: relay not enabled");
    if (l->relay_done.recorded()) {
        DeviceGuard dg(l->device);
        HIP_TRY(l->relay_done.wait((hipStream_t)stream));
    }
    return DPWA_OK;
}

int dpwa_learner_relay_phase1(dpwa_learner *l, const int32_t *picks_dev, uint64_t version, int blocks,
                              dpwa_stream_t stream)
{
    if (!l || !l->relay_on || !picks_dev || blocks < 1)
        return set_error(DPWA_ERR_ARG, "dpwa_learner_relay_phase1: bad arguments");
    RelayArgs a;
    if (int rc = relay_args(l, picks_dev, version, a)) return rc;
    DeviceGuard dg(l->device);
    HIP_TRY(l->fetch.side_after((hipStream_t)stream));
    HIP_TRY(launch_relay(1, a, blocks, l->side.h));
    HIP_TRY(l->relay_done.record(l->side.h));
    return DPWA_OK;
}

// Phase 2 on the side stream: my_pick's stripes gathered into staging.
static int relay_phase2_now(dpwa_learner *l, const RelayArgs &a, int my_pick, int blocks)
{
    hipStream_t side = l->side.h;
    if (my_pick >= 0) HIP_TRY(l->fetch.staging_writable_after_consumption());   // WAR on staging
    HIP_TRY(launch_relay(2, a, blocks, side));
    HIP_TRY(l->relay_done.record(side));
    if (my_pick >= 0) HIP_TRY(l->fetch.landed_on_side());
    return DPWA_OK;
}

// A deferred phase 2 whose fetch is consumed other than by the fused average (the split
// update_wait, a copy of the payload, an unaligned buffer): gather into staging now.  The side
// stream is still ordered after phase 1 and the round's barrier.
static int relay_materialize(dpwa_learner *l)
{
    if (!l->relay_deferred) return DPWA_OK;
    l->relay_deferred = false;
    return relay_phase2_now(l, l->relay_saved, l->relay_saved_pick, l->relay_saved_blocks);
}

int dpwa_learner_relay_phase2(dpwa_learner *l, const int32_t *picks_dev, int my_pick, uint64_t version, int blocks,
                              int fuse)
{
    if (!l || !l->relay_on || !picks_dev || blocks < 1 || my_pick >= l->relay_world || my_pick == l->relay_rank)
        return set_error(DPWA_ERR_ARG, "dpwa_learner_relay_phase2: bad arguments");
    if (fuse && l->dtype == DPWA_MIXED)
        return set_error(DPWA_ERR_ARG, "dpwa_learner_relay_phase2: the fused second phase is not built for segmented "
                                       "(DPWA_MIXED) payloads; gather (fuse = 0)");
    if (fuse && l->measure.whole())
        return set_error(DPWA_ERR_STATE, "dpwa_learner_relay_phase2: the fused second phase reads no contiguous peer "
                                         "snapshot, so a learner that tracks the distance (dpwa_learner_set_distance) "
                                         "cannot use it; gather (fuse = 0)");
    if (fuse && l->measure.param())
        return set_error(DPWA_ERR_STATE, "dpwa_learner_relay_phase2: the fused second phase reads no contiguous peer "
                                         "snapshot, so a learner that measures the per-parameter distance "
                                         "(dpwa_learner_set_param_distance) cannot use it; gather (fuse = 0)");
    if (fuse && l->finite_check)
        return set_error(DPWA_ERR_STATE, "dpwa_learner_relay_phase2: the fused second phase reads no contiguous peer "
                                         "snapshot, so a learner that skips non-finite peers "
                                         "(dpwa_learner_set_finite_check) cannot use it; gather (fuse = 0)");
    RelayArgs a;
    int rc = relay_args(l, picks_dev, version, a);
    if (rc) return rc;
    DeviceGuard dg(l->device);
    l->relay_deferred = false;
    if (fuse && my_pick >= 0) {
        // everything the fused average needs is on the side stream now (phase 1, the barrier)
        HIP_TRY(l->fetch.landed_on_side());
        l->relay_saved = a;
        l->relay_saved_pick = my_pick;
        l->relay_saved_blocks = blocks;
        l->relay_deferred = true;
    } else if (!fuse || my_pick >= 0) {
        if ((rc = relay_phase2_now(l, a, my_pick, blocks))) return rc;
    }
    if (my_pick >= 0) l->fetch.arrived_in_staging();
    return DPWA_OK;
}

int dpwa_learner_time_averages(dpwa_learner *l, int capacity)
{
    if (!l || capacity < 0) return set_error(DPWA_ERR_ARG, "dpwa_learner_time_averages: bad arguments");
    DeviceGuard dg(l->device);
    HIP_TRY(hipDeviceSynchronize());
    l->timing_armed = false;
    HIP_TRY(l->avg_times.reserve(capacity));
    return DPWA_OK;
}

int dpwa_learner_arm_timing(dpwa_learner *l)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_arm_timing: NULL learner");
    l->timing_armed = true;
    return DPWA_OK;
}

int dpwa_learner_read_average_times(dpwa_learner *l, float *us_out, int max, int *count)
{
    if (!l || !count || (max > 0 && !us_out)) return set_error(DPWA_ERR_ARG, "dpwa_learner_read_average_times: bad arguments");
    DeviceGuard dg(l->device);
    HIP_TRY(l->avg_times.read(us_out, max, count));
    l->avg_times.used = 0;   // the pairs are handed out again (a fetch's are not)
    return DPWA_OK;
}

int dpwa_learner_time_fetches(dpwa_learner *l, int capacity)
{
    if (!l || capacity < 0) return set_error(DPWA_ERR_ARG, "dpwa_learner_time_fetches: bad arguments");
    DeviceGuard dg(l->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(l->fetch_times.reserve(capacity));
    return DPWA_OK;
}

int dpwa_learner_read_fetch_times(dpwa_learner *l, float *us_out, int max, int *count)
{
    if (!l || !count || (max > 0 && !us_out)) return set_error(DPWA_ERR_ARG, "dpwa_learner_read_fetch_times: bad arguments");
    DeviceGuard dg(l->device);
    HIP_TRY(l->fetch_times.read(us_out, max, count));
    return DPWA_OK;
}

int dpwa_learner_side_stream(dpwa_learner *l, dpwa_stream_t *stream)
{
    if (!l || !stream) return set_error(DPWA_ERR_ARG, "dpwa_learner_side_stream: NULL argument");
    *stream = l->side.h;
    return DPWA_OK;
}

int dpwa_learner_wait_fetch(dpwa_learner *l, dpwa_stream_t stream)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_wait_fetch: NULL learner");
    if (l->fetch.awaits_copy()) {
        DeviceGuard dg(l->device);
        if (int rc = relay_materialize(l)) return rc;
        HIP_TRY(l->fetch.wait_landed((hipStream_t)stream));
    }
    return DPWA_OK;
}

int dpwa_learner_set_loss_dtype(dpwa_learner *l, int32_t dtype)
{
    if (!l || (dtype != DPWA_F32 && dtype != DPWA_F64)) return set_error(DPWA_ERR_ARG, "dpwa_learner_set_loss_dtype: bad arguments");
    l->loss_f32 = dtype == DPWA_F32;
    return DPWA_OK;
}

int dpwa_learner_set_pull(dpwa_learner *l, int mode, int max_blocks)
{
    if (!l || (mode != DPWA_PULL_COPY_ENGINE && mode != DPWA_PULL_KERNEL) || max_blocks < 1)
        return set_error(DPWA_ERR_ARG, "dpwa_learner_set_pull: bad arguments");
    l->pull_mode = mode;
    l->pull_blocks = max_blocks;
    return DPWA_OK;
}

int dpwa_learner_copy_factor(dpwa_learner *l, double *dst_dev, dpwa_stream_t stream)
{
    if (!l || !dst_dev) return set_error(DPWA_ERR_ARG, "dpwa_learner_copy_factor: NULL argument");
    DeviceGuard dg(l->device);
    HIP_TRY(hipMemcpyAsync(dst_dev, &l->ctl->coef.factor, sizeof(double), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return DPWA_OK;
}

int dpwa_learner_copy_fetched(dpwa_learner *l, void *dst_dev, dpwa_stream_t stream)
{
    if (!l || (!dst_dev && l->n > 0)) return set_error(DPWA_ERR_ARG, "dpwa_learner_copy_fetched: NULL argument");
    if (!l->fetch.fetched()) return set_error(DPWA_ERR_STATE, "dpwa_learner_copy_fetched: no fetch in flight");
    DeviceGuard dg(l->device);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = relay_materialize(l)) return rc;
    HIP_TRY(l->fetch.wait_landed(s));
    if (l->payload_bytes)
        HIP_TRY(hipMemcpyAsync(dst_dev, l->fetch.source().ptr + kPayloadOff, l->payload_bytes, hipMemcpyDeviceToDevice, s));
    HIP_TRY(l->fetch.note_consumed(s));   // a later pull into this staging buffer waits for this copy
    return DPWA_OK;
}

int dpwa_learner_fetch_state(dpwa_learner *l, int64_t timeout_ms, int *state)
{
    if (!l || !state) return set_error(DPWA_ERR_ARG, "dpwa_learner_fetch_state: NULL argument");
    *state = DPWA_FETCH_LANDED;
    if (!l->fetch.awaits_copy() || l->relay_deferred) return DPWA_OK;   // (no device call)
    DeviceGuard dg(l->device);
    return l->fetch.state(timeout_ms, l->relay_deferred, state);
}

int dpwa_learner_rescue_free(dpwa_learner *l, int *free_out)
{
    if (!l || !free_out) return set_error(DPWA_ERR_ARG, "dpwa_learner_rescue_free: NULL argument");
    DeviceGuard dg(l->device);
    int lane = -1;
    // makes a lane now if one is needed and can be made: at most one allocation per wait (the
    // node's poll ends as soon as a lane is free); with the lanes at their cap a poll only queries
    const int rc = l->fetch.lanes().acquire(l->slot_stride, &lane);
    *free_out = lane >= 0 ? 1 : 0;
    return rc;
}

int dpwa_learner_rescue_lanes(dpwa_learner *l, int *lanes, int *cap)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_rescue_lanes: NULL learner");
    if (lanes) *lanes = l->fetch.lanes().count();
    if (cap) *cap = l->fetch.lanes().cap();
    return DPWA_OK;
}

int dpwa_learner_set_rescue_cap(dpwa_learner *l, int cap)
{
    if (!l || cap < 0) return set_error(DPWA_ERR_ARG, "dpwa_learner_set_rescue_cap: bad arguments");
    l->fetch.lanes().set_cap(cap);
    return DPWA_OK;
}

int dpwa_learner_fetch_stream(dpwa_learner *l, dpwa_stream_t *stream)
{
    if (!l || !stream) return set_error(DPWA_ERR_ARG, "dpwa_learner_fetch_stream: NULL argument");
    *stream = l->fetch.stream();
    return DPWA_OK;
}

int dpwa_learner_cancel(dpwa_learner *l)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_cancel: NULL learner");
    l->relay_deferred = false;   // nothing reads the stripes: no gather
    l->fetch.finish();
    return DPWA_OK;
}

int dpwa_learner_pointers(dpwa_learner *l, double **clock_dev, dpwa_coef **coef_dev, dpwa_header **staging_header_dev,
                          void **staging_payload_dev)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_pointers: NULL learner");
    if (clock_dev) *clock_dev = &l->ctl->clock[l->cur];
    if (coef_dev) *coef_dev = &l->ctl->coef;
    if (staging_header_dev) *staging_header_dev = (dpwa_header *)l->fetch.staging();
    if (staging_payload_dev) *staging_payload_dev = l->fetch.staging() + kPayloadOff;
    return DPWA_OK;
}

int dpwa_learner_status_word(dpwa_learner *l, int32_t **status_word)
{
    if (!l || !status_word) return set_error(DPWA_ERR_ARG, "dpwa_learner_status_word: NULL argument");
    *status_word = l->status.host();
    return DPWA_OK;
}

int dpwa_learner_read_clock(dpwa_learner *l, double *clock)
{
    if (!l || !clock) return set_error(DPWA_ERR_ARG, "dpwa_learner_read_clock: NULL argument");
    DeviceGuard dg(l->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(clock, &l->ctl->clock[l->cur], sizeof(double), hipMemcpyDeviceToHost));
    return DPWA_OK;
}

int dpwa_learner_write_clock(dpwa_learner *l, double clock)
{
    if (!l) return set_error(DPWA_ERR_ARG, "dpwa_learner_write_clock: NULL learner");
    DeviceGuard dg(l->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&l->ctl->clock[l->cur], &clock, sizeof(double), hipMemcpyHostToDevice));
    l->wt_header = false;   // the next header was written from the old clock: publish it anew
    return DPWA_OK;
}

int dpwa_learner_read_coef(dpwa_learner *l, dpwa_coef *coef)
{
    if (!l || !coef) return set_error(DPWA_ERR_ARG, "dpwa_learner_read_coef: NULL argument");
    DeviceGuard dg(l->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(coef, &l->ctl->coef, sizeof(dpwa_coef), hipMemcpyDeviceToHost));
    return DPWA_OK;
}

int dpwa_learner_poll_status(dpwa_learner *l, int *done, int32_t *status)
{
    if (!l || !done || !status) return set_error(DPWA_ERR_ARG, "dpwa_learner_poll_status: NULL argument");
    DeviceGuard dg(l->device);
    hipError_t e = l->factor_done.query();
    if (e != hipSuccess && e != hipErrorNotReady) return set_error(DPWA_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(e));
    *done = e == hipSuccess ? 1 : 0;
    // Sticky word: the factor kernel writes only non-OK statuses; reading clears it.
    volatile int32_t *w = l->status.host();
    *status = *w;
    if (*status != DPWA_STATUS_OK) *w = DPWA_STATUS_OK;
    return DPWA_OK;
}

// The consensus of this learner and attached peers over the published slots of `version`
// (include/dpwa_hip.h).  Read-only: no clock, slot, fetch or record of any learner changes.  What it
// reads is ordered as a zero-copy fetch's source is: behind a local peer's publish mark (RAW), and
// registered as a reader of the peer's slot, so that the publish or write-through average that
// rewrites it orders its stream behind this pass (WAR: the learner's consensus_read mark).
int dpwa_learner_consensus(dpwa_learner *l, const int32_t *peer_ids, int count, uint64_t version, void *out,
                           dpwa_consensus_record *record_dev, dpwa_stream_t stream)
{
    const char *fn = "dpwa_learner_consensus";
    if (!l || !peer_ids) return set_error(DPWA_ERR_ARG, "%s: NULL argument", fn);
    if (count < 1 || count > DPWA_CONSENSUS_MAX)
        return set_error(DPWA_ERR_ARG, "%s: %d members (1..%d)", fn, count, DPWA_CONSENSUS_MAX);
    if ((!out && !record_dev) || !aligned16(out) || ((uintptr_t)record_dev & 7))
        return set_error(DPWA_ERR_ARG, "%s: neither out nor a record, or a misaligned one", fn);
    if (version == 0) return set_error(DPWA_ERR_STATE, "%s: nothing published", fn);
    if (int rc = need_layout(l, fn)) return rc;
    if (l->relay_deferred)
        return set_error(DPWA_ERR_STATE, "%s: a fused relay phase is pending (no contiguous snapshot exists)", fn);
    const int k = (int)((version - 1) % 2);
    const void *src[DPWA_CONSENSUS_MAX];
    dpwa_learner *owner[DPWA_CONSENSUS_MAX];
    bool remote = false;
    for (int i = 0; i < count; ++i) {
        const int id = peer_ids[i];
        owner[i] = nullptr;
        if (id == -1) {
            owner[i] = l;
        } else {
            auto it = l->peers.find(id);
            if (it == l->peers.end()) return set_error(DPWA_ERR_ARG, "%s: peer %d not attached", fn, id);
            const Endpoint &ep = it->second;
            if (ep.kind == 1) {
                if (!is_live(ep.local)) return set_error(DPWA_ERR_STATE, "%s: peer %d was destroyed", fn, id);
                if (ep.local->n != l->n || ep.local->dtype != l->dtype || ep.local->layout_digest != l->layout_digest)
                    return set_error(DPWA_ERR_ARG, "%s: peer %d holds another n, dtype or layout", fn, id);
                if (ep.device != l->device)
                    return set_error(DPWA_ERR_ARG, "%s: peer %d is a learner of this process on device %d, not %d", fn, id,
                                     ep.device, l->device);
                owner[i] = ep.local;
            } else {
                if (ep.n != l->n || ep.dtype != l->dtype)   // (its layout digest was compared when it was attached)
                    return set_error(DPWA_ERR_ARG, "%s: peer %d holds another n or dtype", fn, id);
                src[i] = ep.base + (size_t)k * (size_t)ep.slot_stride + kPayloadOff;
                remote = true;
            }
        }
        if (dpwa_learner *o = owner[i]) {
            if (o->version != version)
                return set_error(DPWA_ERR_STATE, "%s: member %d (peer %d) is at version %llu, not %llu", fn, i, id,
                                 (unsigned long long)o->version, (unsigned long long)version);
            if (!o->published[k].noted()) return set_error(DPWA_ERR_STATE, "%s: peer %d slot %d never published", fn, id, k);
            src[i] = slot_payload(o, k);
        }
        for (int j = 0; j < i; ++j)
            if (src[j] == src[i]) return set_error(DPWA_ERR_ARG, "%s: members %d and %d name the same slot", fn, j, i);
    }
    const Payload p = payload(l);
    for (int i = 0; i < count; ++i) {
        const uintptr_t a = (uintptr_t)src[i], o = (uintptr_t)out;
        if (out && a < o + l->payload_bytes && o < a + l->payload_bytes)
            return set_error(DPWA_ERR_ARG, "%s: out overlaps member %d's slot", fn, i);
    }
    DeviceGuard dg(l->device);
    hipStream_t s = (hipStream_t)stream;
    if (record_dev && !l->consensus_rows.h) {   // the first call that measures; never again
        HIP_TRY(l->consensus_rows.alloc((size_t)kDistanceWorkspaceBytes));
        HIP_TRY(hipMemset(l->consensus_rows.h, 0, (size_t)kDistanceWorkspaceBytes));
        HIP_TRY(hipDeviceSynchronize());
    }
    for (int i = 0; i < count; ++i) {
        dpwa_learner *o = owner[i];
        if (!o) continue;
        HIP_TRY(o->published[k].order(s));   // RAW
        std::lock_guard<std::mutex> g(o->readers_mu);
        auto &rv = o->readers[k];
        if (std::find(rv.begin(), rv.end(), l) == rv.end()) rv.push_back(l);
    }
    double *rows = record_dev ? (double *)l->consensus_rows.h : nullptr;
    HIP_TRY(launch_consensus(p, src, count, 1.0 / (double)count, out, rows, remote, s));
    if (record_dev) HIP_TRY(launch_consensus_finish(rows, record_dev, p.elements(), count, version, s));
    // WAR: whoever rewrites a slot read here finds this learner among the slot's readers and orders its
    // stream behind this mark (wait_slot_readers), whatever the learner's fetches do to theirs meanwhile.
    l->consensus_read.note(s);
    return DPWA_OK;
}

}  // extern "C"
