// measure.hpp -- the distance measurements of one learner (learner.cpp): which of the two records are on, the
// device buffers behind them, the distance_every count, and everything launched for them around an average.
// Both passes read operands that the in-place averages overwrite, so they run before the average on its stream;
// both finishing steps read the coefficients that average committed, so they run after it.
// Host only; tests/native/measure_check.cpp pins the exact calls.
#pragma once

#include <utility>
#include <vector>

#include "kernels.hpp"
#include "order.hpp"

namespace dpwa {

// The rules of a list of dpwa_param_range, the device table of a valid list (returns the accumulator rows it
// needs) and the buffer sizes that follow (distance.cpp; host only, no HIP call).
int param_ranges_problem(const char *fn, const dpwa_param_range *ranges, int64_t count, bool payload, int32_t dtype,
                         int64_t n, const dpwa_layout *layout);
int64_t param_table(const dpwa_param_range *ranges, int64_t count, std::vector<ParamEntry> *out);
void param_sizes(const dpwa_param_range *ranges, int64_t count, dpwa_param_sizes &z);

// What a learner averages (as every launch takes it: Elems, kernels.hpp), and where its round's coefficients land.
struct Payload : Elems {
    const dpwa_coef *coef;
    int need_layout(const char *fn) const
    {
        if (!segmented() || layout) return DPWA_OK;
        return set_error(DPWA_ERR_STATE, "%s: a DPWA_MIXED learner has no layout yet (dpwa_learner_set_layout)", fn);
    }
};

class Measure {
public:
    // dpwa_learner_set_distance: the accumulators and, behind them, the record; allocated when first switched
    // on, kept until destroy.  `relay_pending`: a fused relay second phase is.
    int set_whole(const char *fn, bool on, bool relay_pending)
    {
        if (on && relay_pending) return relay_refusal(fn);
        if (on && !dist_.ptr())
            if (int rc = zeroed(fn, (size_t)kDistanceWorkspaceBytes + sizeof(dpwa_distance), nullptr, 0, dist_)) return rc;
        whole_ = on;
        return DPWA_OK;
    }

    // dpwa_learner_set_param_distance: table, workspace and record in one allocation made whenever it is switched
    // on; the pass runs on every `every`-th round that launches an average.
    int set_param(const char *fn, const dpwa_param_range *ranges, int64_t count, int every, const Payload &p,
                  bool relay_pending)
    {
        if (count == 0) {
            param_ = false;
            return DPWA_OK;
        }
        if (every < 1) return set_error(DPWA_ERR_ARG, "%s: every = %d, it must be >= 1", fn, every);
        if (int rc = p.need_layout(fn)) return rc;
        if (int rc = param_ranges_problem(fn, ranges, count, true, p.dtype, p.n, p.layout)) return rc;
        if (relay_pending) return relay_refusal(fn);
        dpwa_param_sizes z;
        param_sizes(ranges, count, z);
        std::vector<ParamEntry> table;
        param_table(ranges, count, &table);
        const int64_t workspace_off = (z.table_bytes + 127) / 128 * 128, record_off = workspace_off + z.workspace_bytes;
        if (int rc = zeroed(fn, (size_t)(record_off + z.record_bytes), table.data(), table.size() * sizeof(ParamEntry), pd_mem_))
            return rc;
        pd_ = Param{count, workspace_off, record_off, every};
        param_ = true;
        return DPWA_OK;
    }

    bool whole() const { return whole_; }
    bool param() const { return param_; }
    // The records (null: never switched on); the rounds counted and measured since the per-parameter option was
    // last switched on.
    dpwa_distance *record() const { return dist_.ptr() ? (dpwa_distance *)(dist_.ptr() + kDistanceWorkspaceBytes) : nullptr; }
    dpwa_param_distance_head *param_record() const
    {
        return pd_mem_.ptr() ? (dpwa_param_distance_head *)(pd_mem_.ptr() + pd_.record_off) : nullptr;
    }
    int64_t param_count() const { return pd_.count; }
    int64_t rounds() const { return pd_.rounds; }
    int64_t measured() const { return pd_.measured; }

    // The per-parameter pass has no form for unaligned parameters: refused before anything is queued or counted.
    int operands_problem(const char *fn, const void *flat) const
    {
        if (!param_ || aligned16(flat)) return DPWA_OK;
        return set_error(DPWA_ERR_ARG, "%s: the per-parameter distance (dpwa_learner_set_param_distance) has no form "
                                       "for parameters that are not 16-byte aligned", fn);
    }

    // Does the averaging kernel itself produce this round's whole-model sums (launch_average_tracked: one element
    // type and, like a batched dispatch, aligned16 operands)?
    bool fused(const Payload &p, const void *flat, const void *peer, const void *snap) const
    {
        return whole_ && !p.segmented() && aligned16(flat, peer, snap);
    }

    // Before the average: counts the round, then the passes that are due (none for a fused whole-model record).
    int before(const Payload &p, const void *flat, const void *peer, bool fused, hipStream_t s)
    {
        if (param_) pd_.due = ++pd_.rounds % pd_.every == 0;
        if (param_ && pd_.due) {
            HIP_TRY(launch_param_distance(flat, peer, p.bytes(), table(), pd_.count, param_acc(), s));
            ++pd_.measured;
        }
        if (whole_ && !fused) HIP_TRY(launch_distance(p, flat, peer, acc(), s));
        return DPWA_OK;
    }

    // After it: the finishing steps, the per-parameter one only where this round's pass ran.
    int after(const Payload &p, hipStream_t s)
    {
        if (whole_) HIP_TRY(launch_distance_finish(acc(), record(), p.coef, p.elements(), s));
        if (!param_ || !pd_.due) return DPWA_OK;
        pd_.due = false;
        HIP_TRY(launch_param_distance_finish(param_acc(), table(), pd_.count, param_record(), p.coef, s));
        return DPWA_OK;
    }

    double *acc() const { return (double *)dist_.ptr(); }

private:
    static int relay_refusal(const char *fn)
    {
        return set_error(DPWA_ERR_STATE, "%s: a fused relay second phase is pending (dpwa_learner_relay_phase2 with "
                                         "fuse != 0), which reads no contiguous peer snapshot to measure against", fn);
    }
    // `bytes` of zeroed device memory beginning with `head`, complete on return (here, never inside a round).
    static int zeroed(const char *fn, size_t bytes, const void *head, size_t head_bytes, DevBuf &out)
    {
        DevBuf mem;
        HIP_TRY(mem.alloc(bytes));
        hipError_t e = hipMemset(mem.ptr(), 0, bytes);
        if (e == hipSuccess && head_bytes) e = hipMemcpy(mem.ptr(), head, head_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipDeviceSynchronize();   // (and nothing in flight reads the buffer replaced below)
        if (e != hipSuccess) return set_error(DPWA_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
        out = std::move(mem);
        return DPWA_OK;
    }
    const ParamEntry *table() const { return (const ParamEntry *)pd_mem_.ptr(); }
    double *param_acc() const { return (double *)(pd_mem_.ptr() + pd_.workspace_off); }

    bool whole_ = false, param_ = false;
    DevBuf dist_, pd_mem_;
    struct Param {
        int64_t count = 0, workspace_off = 0, record_off = 0;
        int every = 1;
        int64_t rounds = 0, measured = 0;
        bool due = false;   // this round's pass was launched: its finishing step is due
    } pd_;
};

// One member of an averaging launch: whose measurements, over which payload and operands; for a single fused
// average (`fa`; null for a lerp and a batched dispatch, which never fuse) also what the tracked kernel takes.
struct Measured {
    Measure *m;
    Payload p;
    void *flat;
    const void *peer;
    void *snap;
    const FusedArgs *fa = nullptr;
    bool oop = false;
    const LaunchTiming *timing = nullptr;
};

// The one place the measurements are launched from: every member's passes, the average (`average`, or the
// tracked kernel in its place when the member's round is fused), every member's finishing steps; in member order.
template <class Average> int measured_average(const Measured *ms, int count, hipStream_t s, Average &&average)
{
    const bool fused = ms->fa && ms->m->fused(ms->p, ms->flat, ms->peer, ms->snap);
    for (int i = 0; i < count; ++i)
        if (int rc = ms[i].m->before(ms[i].p, ms[i].flat, ms[i].peer, fused, s)) return rc;
    if (fused) {
        HIP_TRY(launch_average_tracked(ms->p.dtype, ms->flat, ms->peer, ms->p.n, *ms->fa, ms->snap, ms->oop,
                                       ms->m->acc(), s, ms->timing));
    } else if (int rc = average()) {
        return rc;
    }
    for (int i = 0; i < count; ++i)
        if (int rc = ms[i].m->after(ms[i].p, s)) return rc;
    return DPWA_OK;
}

}  // namespace dpwa
