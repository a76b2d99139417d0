// distance.cpp -- the distance to the peer without a learner: the stateless entry points of
// include/dpwa_hip.h (whole-model and per-parameter) and the host-only rules of dpwa_param_range.
// A learner's own measurements: measure.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "measure.hpp"

namespace dpwa {

// The rules of a list of dpwa_param_range (include/dpwa_hip.h).  `payload`: also the rules that
// need one -- `dtype` and `n` of a single-dtype payload, or DPWA_MIXED with `layout`.  Returns
// DPWA_OK or DPWA_ERR_ARG with the rule broken.  Host only, no HIP call.
int param_ranges_problem(const char *fn, const dpwa_param_range *ranges, int64_t count, bool payload,
                                int32_t dtype, int64_t n, const dpwa_layout *layout)
{
    if (count < 0 || (count > 0 && !ranges)) return set_error(DPWA_ERR_ARG, "%s: NULL ranges or count < 0", fn);
    if (count > 0x7fffffffLL / kParamDistRows)
        return set_error(DPWA_ERR_ARG, "%s: more than %lld ranges", fn, 0x7fffffffLL / kParamDistRows);
    if (payload) {
        if (dtype == DPWA_MIXED) {
            if (!layout) return set_error(DPWA_ERR_ARG, "%s: a DPWA_MIXED payload needs its layout", fn);
            if (const char *why = layout_problem(*layout, -1)) return set_error(DPWA_ERR_ARG, "%s: %s", fn, why);
        } else if (dtype_size(dtype) == 0 || dtype == DPWA_F64 || n < 0) {
            return set_error(DPWA_ERR_ARG, "%s: unknown dtype %d or n < 0", fn, dtype);
        }
    }
    int64_t prev_end = 0;
    for (int64_t t = 0; t < count; ++t) {
        const dpwa_param_range &r = ranges[t];
        const long long i = (long long)t, off = (long long)r.byte_offset, len = (long long)r.byte_length;
        if (!is_float_dtype(r.dtype))
            return set_error(DPWA_ERR_ARG, "%s: range %lld: dtype %d is not DPWA_F32, DPWA_BF16 or DPWA_F16", fn, i, r.dtype);
        if (r.reserved != 0) return set_error(DPWA_ERR_ARG, "%s: range %lld: reserved must be 0", fn, i);
        if (r.byte_offset < 0 || r.byte_offset % DPWA_PARAM_ALIGN)
            return set_error(DPWA_ERR_ARG, "%s: range %lld: byte_offset %lld is not a non-negative multiple of %d", fn, i,
                             off, DPWA_PARAM_ALIGN);
        if (r.byte_length < 0 || r.byte_length % (int64_t)dtype_size(r.dtype))
            return set_error(DPWA_ERR_ARG, "%s: range %lld: byte_length %lld is not a non-negative multiple of the "
                                           "element size %d", fn, i, len, (int)dtype_size(r.dtype));
        if (r.byte_length > INT64_MAX - r.byte_offset)
            return set_error(DPWA_ERR_ARG, "%s: range %lld: byte_offset + byte_length overflows", fn, i);
        if (r.byte_offset < prev_end)
            return set_error(DPWA_ERR_ARG, "%s: range %lld: ranges must be ascending and non-overlapping (it begins at "
                                           "%lld, the one before ends at %lld)", fn, i, off, (long long)prev_end);
        prev_end = r.byte_offset + r.byte_length;
        if (!payload) continue;
        if (dtype != DPWA_MIXED) {
            if (r.dtype != dtype)
                return set_error(DPWA_ERR_ARG, "%s: range %lld: dtype %d in a payload of dtype %d", fn, i, r.dtype, dtype);
            if (prev_end > n * (int64_t)dtype_size(dtype))
                return set_error(DPWA_ERR_ARG, "%s: range %lld: it ends at byte %lld, outside the payload of %lld bytes",
                                 fn, i, (long long)prev_end, (long long)(n * (int64_t)dtype_size(dtype)));
            continue;
        }
        bool inside = false;
        for (int k = 0; k < layout->count; ++k) {
            const dpwa_segment &g = layout->seg[k];
            if (g.dtype == r.dtype && r.byte_offset >= g.byte_offset && prev_end <= g.byte_offset + g.byte_length)
                inside = true;
        }
        if (!inside)
            return set_error(DPWA_ERR_ARG, "%s: range %lld: bytes [%lld, %lld) do not lie wholly inside the segment of "
                                           "dtype %d", fn, i, off, (long long)prev_end, r.dtype);
    }
    return DPWA_OK;
}

// The device table of valid ranges, and the accumulator rows they need in all.
int64_t param_table(const dpwa_param_range *ranges, int64_t count, std::vector<ParamEntry> *out)
{
    constexpr int64_t span = 1024;   // the pass's one-wave span
    int64_t rows = 0;
    if (out) out->assign((size_t)count, ParamEntry{});
    for (int64_t t = 0; t < count; ++t) {
        const int64_t begin = ranges[t].byte_offset, end = begin + ranges[t].byte_length;
        const int64_t spans = end > begin ? (end + span - 1) / span - begin / span : 0;
        const int64_t r = std::min<int64_t>(spans, kParamDistRows);
        if (out) (*out)[(size_t)t] = ParamEntry{begin, end, ranges[t].dtype, (int32_t)rows, (int32_t)r, 0};
        rows += r;
    }
    return rows;
}

void param_sizes(const dpwa_param_range *ranges, int64_t count, dpwa_param_sizes &z)
{
    z.table_bytes = std::max<int64_t>(count, 1) * (int64_t)sizeof(ParamEntry);
    z.workspace_bytes = std::max<int64_t>(param_table(ranges, count, nullptr), 1) * DPWA_DISTANCE_ACC_STRIDE;
    z.record_bytes = (int64_t)sizeof(dpwa_param_distance_head) + count * (int64_t)sizeof(dpwa_param_pair);
    z.max_rows = kParamDistRows;
    z.reserved = 0;
}

}  // namespace dpwa

using namespace dpwa;

extern "C" {

static_assert(sizeof(dpwa_distance) == 32, "dpwa_distance must be 32 bytes");
static_assert(kDistanceWorkspaceBytes % DPWA_DISTANCE_ACC_STRIDE == 0 && kDistanceWorkspaceBytes <= (1 << 20),
              "distance workspace");

int dpwa_distance_workspace(int64_t *bytes)
{
    if (!bytes) return set_error(DPWA_ERR_ARG, "dpwa_distance_workspace: NULL argument");
    *bytes = kDistanceWorkspaceBytes;
    return DPWA_OK;
}

// The workspace and the record of a stateless distance entry: non-null, 16-B / 8-B aligned.
static bool distance_buffers_ok(const void *workspace, const dpwa_distance *out_dev)
{
    return workspace && out_dev && aligned16(workspace) && ((uintptr_t)out_dev & 7) == 0;
}

int dpwa_measure_distance(int32_t dtype, const void *param, const void *peer_payload, int64_t n, void *workspace,
                          dpwa_distance *out_dev, dpwa_stream_t stream)
{
    if (n < 0 || (n > 0 && (!param || !peer_payload)) || !distance_buffers_ok(workspace, out_dev))
        return set_error(DPWA_ERR_ARG, "dpwa_measure_distance: bad arguments (NULL or misaligned pointer, n < 0)");
    if (dtype == DPWA_MIXED)
        return set_error(DPWA_ERR_ARG, "dpwa_measure_distance: a DPWA_MIXED payload needs its layout "
                                       "(dpwa_measure_distance_mixed)");
    if (!is_float_dtype(dtype))
        return set_error(DPWA_ERR_ARG, "dpwa_measure_distance: unknown dtype %d", dtype);
    const size_t es = dtype_size(dtype);
    if (((uintptr_t)param | (uintptr_t)peer_payload) & (es - 1))
        return set_error(DPWA_ERR_ARG, "dpwa_measure_distance: an operand is not aligned to its element size");
    HIP_TRY(launch_distance(Elems{dtype, n, nullptr}, param, peer_payload, (double *)workspace, (hipStream_t)stream));
    HIP_TRY(launch_distance_finish((double *)workspace, out_dev, nullptr, n, (hipStream_t)stream));
    return DPWA_OK;
}

int dpwa_measure_distance_mixed(const dpwa_layout *layout, const void *param, const void *peer_payload,
                                void *workspace, dpwa_distance *out_dev, dpwa_stream_t stream)
{
    if (!layout || !param || !peer_payload || !distance_buffers_ok(workspace, out_dev))
        return set_error(DPWA_ERR_ARG, "dpwa_measure_distance_mixed: bad arguments (NULL or misaligned pointer)");
    if (const char *why = layout_problem(*layout, -1)) return set_error(DPWA_ERR_ARG, "dpwa_measure_distance_mixed: %s", why);
    if (!aligned16(param, peer_payload))
        return set_error(DPWA_ERR_ARG, "dpwa_measure_distance_mixed: a segmented payload is 16-byte aligned");
    const Elems e{DPWA_MIXED, layout_bytes(*layout), layout};
    HIP_TRY(launch_distance(e, param, peer_payload, (double *)workspace, (hipStream_t)stream));
    HIP_TRY(launch_distance_finish((double *)workspace, out_dev, nullptr, e.elements(), (hipStream_t)stream));
    return DPWA_OK;
}

// The stateless non-finite check (the pass a learner runs before its average: learner.cpp finite_pass).
int dpwa_check_finite(int32_t dtype, const void *peer_payload, int64_t n, uint32_t *veto_dev, uint32_t stamp,
                      dpwa_stream_t stream, void *start_event, void *stop_event)
{
    if (n < 0 || (n > 0 && !peer_payload) || !veto_dev || ((uintptr_t)veto_dev & 3) || stamp == 0 ||
        (!start_event) != (!stop_event))
        return set_error(DPWA_ERR_ARG, "dpwa_check_finite: bad arguments (NULL or misaligned pointer, n < 0, stamp 0)");
    if (dtype == DPWA_MIXED)
        return set_error(DPWA_ERR_ARG, "dpwa_check_finite: a DPWA_MIXED payload needs its layout (dpwa_check_finite_mixed)");
    if (!is_float_dtype(dtype)) return set_error(DPWA_ERR_ARG, "dpwa_check_finite: unknown dtype %d", dtype);
    if ((uintptr_t)peer_payload & (dtype_size(dtype) - 1))
        return set_error(DPWA_ERR_ARG, "dpwa_check_finite: the payload is not aligned to its element size");
    const CallerTiming timing(start_event, stop_event);
    HIP_TRY(launch_peer_finite(Elems{dtype, n, nullptr}, peer_payload, veto_dev, stamp, (hipStream_t)stream, timing));
    return DPWA_OK;
}

int dpwa_check_finite_mixed(const dpwa_layout *layout, const void *peer_payload, uint32_t *veto_dev, uint32_t stamp,
                            dpwa_stream_t stream, void *start_event, void *stop_event)
{
    if (!layout || !peer_payload || !veto_dev || ((uintptr_t)veto_dev & 3) || stamp == 0 || (!start_event) != (!stop_event))
        return set_error(DPWA_ERR_ARG, "dpwa_check_finite_mixed: bad arguments (NULL or misaligned pointer, stamp 0)");
    if (const char *why = layout_problem(*layout, -1)) return set_error(DPWA_ERR_ARG, "dpwa_check_finite_mixed: %s", why);
    if (!aligned16(peer_payload))
        return set_error(DPWA_ERR_ARG, "dpwa_check_finite_mixed: a segmented payload is 16-byte aligned");
    const CallerTiming timing(start_event, stop_event);
    HIP_TRY(launch_peer_finite(Elems{DPWA_MIXED, layout_bytes(*layout), layout}, peer_payload, veto_dev, stamp,
                               (hipStream_t)stream, timing));
    return DPWA_OK;
}

int dpwa_average_tracked(int32_t dtype, void *param, const void *peer_slot, int64_t n, const dpwa_interp *cfg,
                         double *clock_dev, double loss, dpwa_coef *coef_dev, void *snap_payload, void *workspace,
                         dpwa_distance *out_dev, dpwa_stream_t stream, void *start_event, void *stop_event)
{
    if (!cfg || !clock_dev || !coef_dev || !peer_slot || n < 0 || (n > 0 && !param) || (!start_event) != (!stop_event) ||
        !distance_buffers_ok(workspace, out_dev))
        return set_error(DPWA_ERR_ARG, "dpwa_average_tracked: bad arguments (NULL or misaligned pointer, n < 0)");
    if (dtype == DPWA_MIXED)
        return set_error(DPWA_ERR_ARG, "dpwa_average_tracked: segmented (DPWA_MIXED) payloads have no tracked kernel "
                                       "(dpwa_measure_distance_mixed, then dpwa_average_mixed)");
    if (!is_float_dtype(dtype))
        return set_error(DPWA_ERR_ARG, "dpwa_average_tracked: unknown dtype %d", dtype);
    if (int rc = check_method(cfg, "dpwa_average_tracked")) return rc;
    const FusedArgs fa = stateless_args(cfg, clock_dev, peer_slot, loss, coef_dev);
    const CallerTiming timing(start_event, stop_event);
    hipStream_t s = (hipStream_t)stream;
    const char *peer = (const char *)peer_slot + DPWA_SLOT_PAYLOAD_OFFSET;
    if (aligned16(param, peer, snap_payload)) {
        HIP_TRY(launch_average_tracked(dtype, param, peer, n, fa, snap_payload, false, (double *)workspace, s, timing));
    } else {   // the stand-alone pass, then dpwa_average's own (unaligned) kernel
        HIP_TRY(launch_distance(Elems{dtype, n, nullptr}, param, peer, (double *)workspace, s));
        HIP_TRY(launch_average(Elems{dtype, n, nullptr}, param, peer, fa, snap_payload, s, timing));
    }
    HIP_TRY(launch_distance_finish((double *)workspace, out_dev, coef_dev, n, s));
    return DPWA_OK;
}

int dpwa_distance_finish(void *workspace, dpwa_distance *out_dev, const dpwa_coef *coef_dev, int64_t n,
                         dpwa_stream_t stream, void *start_event, void *stop_event)
{
    if (n < 0 || (!start_event) != (!stop_event) || !distance_buffers_ok(workspace, out_dev))
        return set_error(DPWA_ERR_ARG, "dpwa_distance_finish: bad arguments (NULL or misaligned pointer, n < 0)");
    HIP_TRY(launch_distance_finish((double *)workspace, out_dev, coef_dev, n, (hipStream_t)stream,
                                   CallerTiming(start_event, stop_event)));
    return DPWA_OK;
}

// ---------------------------------------------------------------- per-parameter distance
static_assert(sizeof(dpwa_param_range) == 24 && sizeof(dpwa_param_pair) == 16 && sizeof(dpwa_param_distance_head) == 16,
              "per-parameter distance records");

int dpwa_param_ranges_check(const dpwa_param_range *ranges, int64_t count, int32_t dtype, int64_t n,
                            const dpwa_layout *layout)
{
    return param_ranges_problem("dpwa_param_ranges_check", ranges, count, true, dtype, n, layout);
}

int dpwa_param_distance_sizes(const dpwa_param_range *ranges, int64_t count, dpwa_param_sizes *sizes)
{
    if (!sizes) return set_error(DPWA_ERR_ARG, "dpwa_param_distance_sizes: NULL argument");
    if (int rc = param_ranges_problem("dpwa_param_distance_sizes", ranges, count, false, 0, 0, nullptr)) return rc;
    param_sizes(ranges, count, *sizes);
    return DPWA_OK;
}

int dpwa_param_distance_table(const dpwa_param_range *ranges, int64_t count, void *table_dev)
{
    if (count < 1 || !table_dev || !aligned16(table_dev))
        return set_error(DPWA_ERR_ARG, "dpwa_param_distance_table: count < 1, or a NULL or misaligned table");
    if (int rc = param_ranges_problem("dpwa_param_distance_table", ranges, count, false, 0, 0, nullptr)) return rc;
    std::vector<ParamEntry> table;
    param_table(ranges, count, &table);
    HIP_TRY(hipMemcpy(table_dev, table.data(), table.size() * sizeof(ParamEntry), hipMemcpyHostToDevice));
    return DPWA_OK;
}

static bool param_buffers_ok(const void *table_dev, int64_t count, const void *workspace, const void *out_dev)
{
    return count >= 1 && table_dev && workspace && out_dev &&
           aligned16(table_dev, workspace) && ((uintptr_t)out_dev & 7) == 0;
}

int dpwa_measure_param_distance(const void *table_dev, int64_t count, const void *param, const void *peer_payload,
                                int64_t payload_bytes, void *workspace, dpwa_param_distance_head *out_dev,
                                dpwa_stream_t stream, void *start_event, void *stop_event)
{
    if (!param_buffers_ok(table_dev, count, workspace, out_dev) || payload_bytes < 0 || (!start_event) != (!stop_event) ||
        (payload_bytes > 0 && (!param || !peer_payload)))
        return set_error(DPWA_ERR_ARG, "dpwa_measure_param_distance: bad arguments (NULL or misaligned pointer, "
                                       "count < 1, payload_bytes < 0)");
    if (!aligned16(param, peer_payload))
        return set_error(DPWA_ERR_ARG, "dpwa_measure_param_distance: the parameters and the peer payload are 16-byte "
                                       "aligned");
    const CallerTiming timing(start_event, stop_event);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_param_distance(param, peer_payload, payload_bytes, (const ParamEntry *)table_dev, count,
                                  (double *)workspace, s, timing));
    HIP_TRY(launch_param_distance_finish((double *)workspace, (const ParamEntry *)table_dev, count, out_dev, nullptr, s));
    return DPWA_OK;
}

int dpwa_param_distance_finish(const void *table_dev, int64_t count, void *workspace,
                               dpwa_param_distance_head *out_dev, const dpwa_coef *coef_dev, dpwa_stream_t stream,
                               void *start_event, void *stop_event)
{
    if (!param_buffers_ok(table_dev, count, workspace, out_dev) || (!start_event) != (!stop_event))
        return set_error(DPWA_ERR_ARG, "dpwa_param_distance_finish: bad arguments (NULL or misaligned pointer, "
                                       "count < 1)");
    HIP_TRY(launch_param_distance_finish((double *)workspace, (const ParamEntry *)table_dev, count, out_dev, coef_dev,
                                         (hipStream_t)stream, CallerTiming(start_event, stop_event)));
    return DPWA_OK;
}

}  // extern "C"
