// kernels.hpp -- internal launch API of the HIP kernels (kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

namespace dpwa {

// Size in bytes of one element of `dtype`, 0 if unknown.
inline size_t dtype_size(int32_t dtype)
{
    return dtype == DPWA_F32 ? 4 : dtype == DPWA_BF16 || dtype == DPWA_F16 ? 2 : dtype == DPWA_MIXED ? 1 : 0;
}
// One of the element types a kernel averages and measures (not DPWA_MIXED, which names a layout of them).
inline bool is_float_dtype(int32_t dtype) { return dtype == DPWA_F32 || dtype == DPWA_BF16 || dtype == DPWA_F16; }
// Is every one of the pointers 16-byte aligned (a null one is)?
template <class... P> inline bool aligned16(const P *...p) { return ((... | (uintptr_t)p) & 15) == 0; }

// The rules of a dpwa_layout (include/dpwa_hip.h); total_bytes >= 0: it must cover exactly that
// many.  Returns null when valid, else the rule broken.  Host only, no HIP call.
const char *layout_problem(const dpwa_layout &layout, int64_t total_bytes);
// Total bytes of a valid layout.
inline int64_t layout_bytes(const dpwa_layout &layout)
{
    const dpwa_segment &last = layout.seg[layout.count - 1];
    return last.byte_offset + last.byte_length;
}
// The element slots of a valid layout's segments.
inline int64_t layout_elements(const dpwa_layout &layout)
{
    int64_t n = 0;
    for (int i = 0; i < layout.count; ++i) n += layout.seg[i].byte_length / (int64_t)dtype_size(layout.seg[i].dtype);
    return n;
}

// What a launch averages, measures or checks: `n` elements of one dtype, or (DPWA_MIXED, "segmented") `n` bytes
// whose `layout` says which 4-KiB segments hold which dtype.  A segmented payload runs the k_*_mixed kernels:
// every 1-KiB span takes the element op of the segment it lies in, and param / peer / snap are non-null and
// 16-B aligned.  Those rules broken, a segmented payload without its layout, an invalid layout (layout_problem)
// and an unknown dtype are hipErrorInvalidValue to every launch that takes one.
struct Elems {
    int32_t dtype;
    int64_t n;
    const dpwa_layout *layout;   // of a DPWA_MIXED payload (null until it is known), else unused
    bool segmented() const { return dtype == DPWA_MIXED; }
    int64_t bytes() const { return segmented() ? n : n * (int64_t)dtype_size(dtype); }
    int64_t elements() const { return segmented() ? layout_elements(*layout) : n; }
};

// Inputs/outputs of the device factor computation (dpwa.py:139-155).  clock_in and
// clock_out may alias only for the one-thread factor kernel.
struct FusedArgs {
    dpwa_interp cfg;
    const double *clock_in;
    double *clock_out;
    const dpwa_header *hdr;     // the peer's published state
    double loss_h;              // used when loss_d is null
    const double *loss_d;       // a device float64, or a float32 when loss_f32
    int32_t loss_f32;
    dpwa_coef *coef_out;
    int32_t *status_mirror;     // nullable device-visible pinned host word (sticky errors)
    // Write-through averages (the next publish then moves no bytes): the header of the next
    // snapshot {new clock + 1, version, n, dtype; loss NaN -- the peers' factor math reads a
    // peer's loss only under loss interpolation, which keeps the header publish} and that
    // clock into *clock_next.  Null: nothing beyond the average.
    dpwa_header *next_header;
    double *clock_next;
    uint64_t next_version;
    int64_t n;
    int32_t dtype;
    // A learner that skips non-finite peers (launch_peer_finite ran earlier on the stream): the round
    // is a no-op with status DPWA_STATUS_PEER_NONFINITE, counted in *skips, when *veto == stamp.
    // Null veto: no check.
    const uint32_t *veto;
    uint32_t stamp;
    uint64_t *skips;
};

// Lerp over the payload; coefficients from `coef` (device) or, when coef is null, from (a, b) -- a single dtype
// only: a segmented payload needs `coef`.
hipError_t launch_lerp(const Elems &e, void *param, const void *peer, const dpwa_coef *coef, float a, float b,
                       hipStream_t s);

// Optional timing of one launch: HIP records the kernel's own begin/end in the two events
// (hipExtLaunchKernelGGL), so the figure excludes the dispatch gaps an event pair around the
// launch would add.
struct LaunchTiming {
    hipEvent_t start, stop;
};

// Fused factor + lerp (one launch); a non-null `snap` also receives the result.  `oop` (the
// resident form): the result goes to `snap` only and `param` is read, never written.
hipError_t launch_average(const Elems &e, void *param, const void *peer, const FusedArgs &fa, void *snap,
                          hipStream_t s, const LaunchTiming *timing = nullptr, bool oop = false);

// The distance to the peer (dpwa_distance, include/dpwa_hip.h; kernels.hip "distance to the peer").
// `acc`: kDistanceWorkspaceBytes of device memory, zero before the first use; every finish leaves
// it zero again.
//   average_tracked   launch_average with the sums added by the same kernel (k_lerp_tracked):
//                     16-B aligned operands and a single dtype only, else hipErrorInvalidValue
//   distance          the stand-alone pass over (param, peer payload); any element alignment for a single
//                     dtype
//   distance_finish   sums the accumulators into *out when the round averaged (`coef` null, or its
//                     status OK; the record's clock is coef->new_clock, 0 without a coef)
constexpr int64_t kDistanceWorkspaceBytes = 128 << 10;
hipError_t launch_average_tracked(int32_t dtype, void *param, const void *peer, int64_t n, const FusedArgs &fa,
                                  void *snap, bool oop, double *acc, hipStream_t s,
                                  const LaunchTiming *timing = nullptr);
hipError_t launch_distance(const Elems &e, const void *param, const void *peer, double *acc, hipStream_t s);
hipError_t launch_distance_finish(double *acc, dpwa_distance *out, const dpwa_coef *coef, int64_t n, hipStream_t s,
                                  const LaunchTiming *timing = nullptr);

// The consensus of a group (dpwa_consensus, include/dpwa_hip.h; kernels.hip "consensus of a group"):
// the element-wise mean of `count` (1..kMaxConsensus) payloads src[0..count), summed in that order
// in fp64 and scaled by `r` (the host's 1.0 / count), stored into `out` (null: measure only), and
// with `acc` (null: the mean only; kDistanceWorkspaceBytes, zero before the first use, left zero by
// the finish) the sums norm2 and spread2_i.  `remote`: some source is another GPU's memory -- the
// launch is preceded by the system-scope acquire of launch_pull.  hipErrorInvalidValue, nothing
// queued: a count outside 1..8, a null or not 16-B aligned pointer, `out` overlapping a source,
// neither `out` nor `acc`.  There is no unaligned form.
//   consensus_finish   sums the rows into *out (members = count of the pass) and zeroes them
constexpr int kMaxConsensus = 8;
hipError_t launch_consensus(const Elems &e, const void *const *src, int count, double r, void *out, double *acc,
                            bool remote, hipStream_t s, const LaunchTiming *timing = nullptr);
hipError_t launch_consensus_finish(double *acc, dpwa_consensus_record *out, int64_t n, int members, uint64_t version,
                                   hipStream_t s, const LaunchTiming *timing = nullptr);

// The non-finite peer check (kernels.hip "non-finite peer check"): one read of the peer payload; a
// lane that finds a NaN or an inf stores `stamp` (non-zero) into *veto (device memory, 4-B aligned).
// Any element alignment for a single dtype; a segmented payload is 16-B aligned.
hipError_t launch_peer_finite(const Elems &e, const void *peer, uint32_t *veto, uint32_t stamp, hipStream_t s,
                              const LaunchTiming *timing = nullptr);

// The distance to the peer for every parameter tensor (dpwa_param_range, include/dpwa_hip.h;
// kernels.hip "distance to the peer, per tensor").  The device table has one ParamEntry per
// tensor, sorted by `begin`; tensor t adds into rows [first_row, first_row + rows) of `acc`
// (DPWA_DISTANCE_ACC_STRIDE bytes each, zero before the first use and after every finish),
// rows = min(the 1-KiB spans of the payload it touches, kParamDistRows).
//   param_distance         the pass over `total` payload bytes of (param, peer), both 16-B aligned
//   param_distance_finish  one workgroup per tensor: the pairs behind *out, its clock and count,
//                          written when the round averaged (`coef` null, or its status OK)
constexpr int kParamDistRows = 1024;
constexpr int kParamDistEntryBytes = 32;
struct ParamEntry {
    int64_t begin, end;   // payload bytes [begin, end); begin a multiple of 256
    int32_t dtype;
    int32_t first_row;
    int32_t rows;         // 0: an empty tensor
    int32_t reserved;
};
static_assert(sizeof(ParamEntry) == kParamDistEntryBytes, "table entry size");
hipError_t launch_param_distance(const void *param, const void *peer, int64_t total, const ParamEntry *table,
                                 int64_t count, double *acc, hipStream_t s, const LaunchTiming *timing = nullptr);
hipError_t launch_param_distance_finish(double *acc, const ParamEntry *table, int64_t count,
                                        dpwa_param_distance_head *out, const dpwa_coef *coef, hipStream_t s,
                                        const LaunchTiming *timing = nullptr);

// Several fused averages (co-resident learners) in one dispatch: entry i's workgroups follow
// entry i-1's.  Every pointer 16-B aligned; `dual` = every entry writes through (snap non-null).
constexpr int kMaxAvgBatch = 8;
struct AvgEntry {
    void *param;
    const void *peer;    // payload of the snapshot averaged with
    void *snap;          // write-through destination, or null
    int64_t n;
    FusedArgs fa;
};
struct AvgBatch {
    int32_t count;
    // span order over equal-size entries (launcher): 0 one entry after the other, 1 dealt
    // round-robin, 2 XCD-grouped (every entry's span s on XCD s % 8, one after the other: entries
    // that read the same buffer -- resident learners that picked each other -- share it in L2)
    int32_t interleave;
    uint32_t spans;                 // spans per entry (XCD-grouped: equal sizes; the last may be empty)
    uint32_t begin[kMaxAvgBatch];   // first workgroup of each entry (filled by the launcher)
    // a group (k_lerp_pair / k_lerp_group: resident entries of equal size whose reads overlap):
    // the distinct buffers its entries read, src[0..count) the entries' parameters and then the
    // peer snapshots of no entry's parameters; entry i's peer is src[peer_of[i]] (filled by the
    // launcher)
    int8_t peer_of[kMaxAvgBatch];
    const void *src[kMaxAvgBatch];
    AvgEntry e[kMaxAvgBatch];
};
hipError_t launch_average_batch(int32_t dtype, bool dual, const AvgBatch &b, hipStream_t s,
                                const LaunchTiming *timing = nullptr, bool oop = false);

// Factor + clock only (one thread).
hipError_t launch_factor(const FusedArgs &fa, hipStream_t s);

// Snapshot publish: slot header {clock+1, loss, version, n, dtype} + payload copy of `nbytes`.
// `system_release` follows it with a system-scope L2 write-back on every XCD so other
// devices (IPC peers) read the bytes from HBM.
hipError_t launch_publish(char *slot, const void *flat, int64_t nbytes, int64_t n, int32_t dtype,
                          double *clock, double loss, const double *loss_dev, bool loss_f32, uint64_t version,
                          bool system_release, hipStream_t s);
// Local streaming copy of `nbytes` (a resident learner's relocation between its slots).
hipError_t launch_copy_payload(void *dst, const void *src, int64_t nbytes, hipStream_t s);
// Pull of `nbytes` (multiple of 16, 16-B aligned) from a peer's slot into local staging with
// a copy kernel of at most `max_blocks` workgroups.  `remote`: the source is another GPU's
// memory -- the kernel is preceded by a system-scope acquire on every XCD, so no L2 line of
// that memory cached by an earlier round is read.
hipError_t launch_pull(void *dst, const void *src, int64_t nbytes, int max_blocks, bool remote, hipStream_t s);
// Relay (multi-link) pull of a lock-step round; see kernels.hip.  All pointers are in this
// process's address space (IPC-mapped for other ranks).
constexpr int kMaxRelayRanks = 64;
struct RelayArgs {
    const char *slots[kMaxRelayRanks];    // slot 0 of every rank's snapshot allocation
    const char *relays[kMaxRelayRanks];   // every rank's relay buffer
    char *relay_mine;
    char *staging;                        // header + payload destination (phase 2)
    const int32_t *picks;                 // device: the peer every rank averages with, -1 none
    int64_t slot_off;                     // byte offset of this round's slot from slot 0
    int64_t stripe;                       // bytes per stripe (multiple of 16)
    int64_t payload;                      // payload bytes to move (multiple of 16)
    int32_t world, rank;
};
hipError_t launch_relay(int phase, const RelayArgs &a, int blocks_per_part, hipStream_t s);
// The relay's phase 2 fused into the average: the fused average of `param` reading stripe r of
// my_pick's snapshot where phase 1 left it (k_lerp_relay), preceded by a system-scope acquire.
// The header is read from fa.hdr (my_pick's slot).  param / snap 16-B aligned.
hipError_t launch_average_relay(int32_t dtype, void *param, int64_t n, const FusedArgs &fa, void *snap,
                                const RelayArgs &a, int my_pick, hipStream_t s, const LaunchTiming *timing = nullptr,
                                bool oop = false);
// Publish of the header only (the payload was written through by the last average).
hipError_t launch_publish_header(char *slot, int64_t n, int32_t dtype, double *clock, double loss,
                                 const double *loss_dev, bool loss_f32, uint64_t version, bool system_release,
                                 hipStream_t s);

// dpwa_stream_mix: the averaging kernels' access mix alone (measurement only).
struct StreamMixArgs {
    const char *src[2];
    char *dst[2];
    int64_t nbytes;   // a multiple of 16
    int32_t nr, nw;
};
hipError_t launch_stream_mix(const StreamMixArgs &a, hipStream_t s, const LaunchTiming *timing);

// Reuse guard of a header-only publish: sampled words of `flat` against the snapshot `payload`
// the last average wrote; on a difference the payload is copied from `flat` and *hits += 1
// (*dirty: the verdict, device memory; both written by the device).
hipError_t launch_guard_payload(char *payload, const void *flat, int64_t nbytes, int32_t *dirty, uint32_t *hits,
                                int32_t gen, hipStream_t s);

// Window guard of resident parameters (learner.cpp): one launch per publish compares the payload
// published last time (`old`) with the samples saved then -- on a difference stamping *dirty with
// `gen`, counting the window in *hits and mirroring the count into the host-mapped word *host --
// and saves the samples of the payload published now (`cur`) into `sample` (kWindowSampleBytes).
// Payloads 16-B aligned; either may be NULL.
constexpr int64_t kWindowSampleBytes = (4096 + 3) * 16;   // samples, tail bytes, first and last word
hipError_t launch_window_roll(const char *old, const char *cur, int64_t nbytes, char *sample, int32_t *dirty,
                              uint32_t *hits, uint32_t *host, int32_t gen, int32_t cur_gen, hipStream_t s);

// A system-scope L2 write-back on every XCD after the work already on `s` (a publish whose
// bytes were written by an earlier kernel, read by other devices).
hipError_t launch_release_system(hipStream_t s);

// A system-scope release store of one 64-bit word after the work already on `s`.
hipError_t launch_store_u64(uint64_t *p, uint64_t v, hipStream_t s);

// What the stateless entry points (learner.cpp, distance.cpp) share; `fn` names the entry in messages.
// The caller's begin/end events as a launch's timing argument: NULL when none were given.
struct CallerTiming {
    LaunchTiming t;
    CallerTiming(void *start_event, void *stop_event) : t{(hipEvent_t)start_event, (hipEvent_t)stop_event} {}
    operator const LaunchTiming *() const { return t.start ? &t : nullptr; }
};

inline int check_method(const dpwa_interp *cfg, const char *fn)
{
    if (cfg->method < 0 || cfg->method > 2) return set_error(DPWA_ERR_ARG, "%s: unknown method %d", fn, cfg->method);
    return DPWA_OK;
}

// Factor from the header of `peer_slot`, clock read at clock_dev and written behind it.
inline FusedArgs stateless_args(const dpwa_interp *cfg, double *clock_dev, const void *peer_slot, double loss,
                                dpwa_coef *coef_dev)
{
    FusedArgs fa{};
    fa.cfg = *cfg;
    fa.clock_in = clock_dev;
    fa.clock_out = clock_dev + 1;
    fa.hdr = (const dpwa_header *)peer_slot;
    fa.loss_h = loss;
    fa.coef_out = coef_dev;
    return fa;
}

}  // namespace dpwa
