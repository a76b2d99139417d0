// consensus.cpp -- the consensus of a group without a learner: the stateless entry points of
// include/dpwa_hip.h (dpwa_consensus, dpwa_consensus_mixed).  A learner's own call over published
// slots (dpwa_learner_consensus) is in learner.cpp, beside the slots and marks it reads.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

using namespace dpwa;

extern "C" {

static_assert(sizeof(dpwa_consensus_record) == 128, "dpwa_consensus_record must be 128 bytes");
static_assert(DPWA_CONSENSUS_MAX == kMaxConsensus, "members of one pass");
static_assert((DPWA_CONSENSUS_MAX + 1) * sizeof(double) <= DPWA_DISTANCE_ACC_STRIDE, "the sums of a span share a row");

int dpwa_consensus_workspace(int64_t *bytes)
{
    if (!bytes) return set_error(DPWA_ERR_ARG, "dpwa_consensus_workspace: NULL argument");
    *bytes = kDistanceWorkspaceBytes;
    return DPWA_OK;
}

// What both entries check before a launch: the rule broken, or null.  Host only.
static const char *consensus_problem(const void *const *payloads, int count, int64_t bytes, const void *out,
                                     const void *workspace, const dpwa_consensus_record *record_dev,
                                     const void *start_event, const void *stop_event)
{
    if (count < 1 || count > DPWA_CONSENSUS_MAX) return "count is outside 1..8";
    if (!payloads) return "NULL payloads";
    if ((!workspace) != (!record_dev)) return "a workspace and a record go together (both or neither)";
    if (!out && !record_dev) return "neither out nor a record: nothing to do";
    if ((!start_event) != (!stop_event)) return "one event without the other";
    if (!aligned16(out, workspace) || ((uintptr_t)record_dev & 7)) return "out, the workspace or the record is misaligned";
    for (int i = 0; i < count; ++i) {
        if (!payloads[i]) return "a NULL payload";
        if (!aligned16(payloads[i])) return "a payload is not 16-byte aligned (there is no unaligned form)";
        const uintptr_t p = (uintptr_t)payloads[i], o = (uintptr_t)out;
        if (out && (p == o || (p < o + (uintptr_t)bytes && o < p + (uintptr_t)bytes))) return "out overlaps a payload";
    }
    return nullptr;
}

static int run_consensus(const Elems &e, const void *const *payloads, int count, void *out,
                         void *workspace, dpwa_consensus_record *record_dev, dpwa_stream_t stream, void *start_event,
                         void *stop_event)
{
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_consensus(e, payloads, count, 1.0 / (double)count, out, (double *)workspace, false, s,
                             CallerTiming(start_event, stop_event)));
    if (record_dev) HIP_TRY(launch_consensus_finish((double *)workspace, record_dev, e.elements(), count, 0, s));
    return DPWA_OK;
}

int dpwa_consensus(int32_t dtype, const void *const *payloads, int count, int64_t n, void *out, void *workspace,
                   dpwa_consensus_record *record_dev, dpwa_stream_t stream, void *start_event, void *stop_event)
{
    if (dtype == DPWA_MIXED)
        return set_error(DPWA_ERR_ARG, "dpwa_consensus: a DPWA_MIXED payload needs its layout (dpwa_consensus_mixed)");
    if (!is_float_dtype(dtype)) return set_error(DPWA_ERR_ARG, "dpwa_consensus: unknown dtype %d", dtype);
    if (n < 0 || n > INT64_MAX / 4) return set_error(DPWA_ERR_ARG, "dpwa_consensus: n < 0 or too large");
    const Elems e{dtype, n, nullptr};
    if (const char *why = consensus_problem(payloads, count, e.bytes(), out, workspace, record_dev, start_event, stop_event))
        return set_error(DPWA_ERR_ARG, "dpwa_consensus: %s", why);
    return run_consensus(e, payloads, count, out, workspace, record_dev, stream, start_event, stop_event);
}

int dpwa_consensus_mixed(const dpwa_layout *layout, const void *const *payloads, int count, void *out, void *workspace,
                         dpwa_consensus_record *record_dev, dpwa_stream_t stream, void *start_event, void *stop_event)
{
    if (!layout) return set_error(DPWA_ERR_ARG, "dpwa_consensus_mixed: NULL layout");
    if (const char *why = layout_problem(*layout, -1)) return set_error(DPWA_ERR_ARG, "dpwa_consensus_mixed: %s", why);
    const Elems e{DPWA_MIXED, layout_bytes(*layout), layout};
    if (const char *why = consensus_problem(payloads, count, e.bytes(), out, workspace, record_dev, start_event, stop_event))
        return set_error(DPWA_ERR_ARG, "dpwa_consensus_mixed: %s", why);
    return run_consensus(e, payloads, count, out, workspace, record_dev, stream, start_event,
                         stop_event);
}

}  // extern "C"
