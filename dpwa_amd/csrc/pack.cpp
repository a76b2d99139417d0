// pack.cpp -- packed snapshots without a learner: the stateless entry points of include/dpwa_hip.h
// (dpwa_pack_bytes, dpwa_pack, dpwa_pack_if, dpwa_unpack, dpwa_average_packed, dpwa_average_pack, and the
// stochastically rounding dpwa_pack_stochastic and dpwa_average_pack_stochastic).  A learner's
// images, packed at a publish or by the average ahead of it and pulled in place of the payload
// (DPWA_PULL_PACKED), are in learner.cpp, beside the slots they mirror.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

using namespace dpwa;

extern "C" {

// What all three check first: the rule broken, or null.  Host only.
static const char *pack_problem(int32_t dtype, int64_t n)
{
    if (dtype == DPWA_MIXED) return "a DPWA_MIXED payload has no packed form (one element type per image)";
    if (!is_float_dtype(dtype)) return "unknown dtype";
    if (n < 0 || n > INT64_MAX / 4) return "n < 0 or too large";
    return nullptr;
}

int dpwa_pack_bytes(int32_t dtype, int64_t n, int64_t *bytes)
{
    if (!bytes) return set_error(DPWA_ERR_ARG, "dpwa_pack_bytes: NULL argument");
    if (const char *why = pack_problem(dtype, n)) return set_error(DPWA_ERR_ARG, "dpwa_pack_bytes: %s", why);
    *bytes = pack_image_bytes(dtype, n);
    return DPWA_OK;
}

// dpwa_pack and dpwa_pack_stochastic: one set of refusals, one launcher, two rounding policies.
static int pack_entry(const char *fn, int32_t dtype, const void *payload, int64_t n, void *image, PackRounding rounding,
                      dpwa_stream_t stream, void *start_event, void *stop_event)
{
    if (const char *why = pack_problem(dtype, n)) return set_error(DPWA_ERR_ARG, "%s: %s", fn, why);
    if (!payload || !image || (!start_event) != (!stop_event))
        return set_error(DPWA_ERR_ARG, "%s: a NULL pointer, or one event without the other", fn);
    if (!aligned16(payload, image))
        return set_error(DPWA_ERR_ARG, "%s: the payload or the image is not 16-byte aligned (there is no unaligned form)", fn);
    HIP_TRY(launch_pack(dtype, payload, n, image, (hipStream_t)stream, CallerTiming(start_event, stop_event), rounding));
    return DPWA_OK;
}

int dpwa_pack(int32_t dtype, const void *payload, int64_t n, void *image, dpwa_stream_t stream, void *start_event,
              void *stop_event)
{
    return pack_entry("dpwa_pack", dtype, payload, n, image, PackRounding{}, stream, start_event, stop_event);
}

int dpwa_pack_stochastic(int32_t dtype, const void *payload, int64_t n, void *image, uint64_t nonce,
                         dpwa_stream_t stream, void *start_event, void *stop_event)
{
    return pack_entry("dpwa_pack_stochastic", dtype, payload, n, image, PackRounding{true, nonce}, stream, start_event,
                      stop_event);
}

int dpwa_unpack(int32_t dtype, const void *image, int64_t n, void *payload_out, int max_blocks, dpwa_stream_t stream,
                void *start_event, void *stop_event)
{
    if (const char *why = pack_problem(dtype, n)) return set_error(DPWA_ERR_ARG, "dpwa_unpack: %s", why);
    if (!payload_out || !image || (!start_event) != (!stop_event) || max_blocks < 1)
        return set_error(DPWA_ERR_ARG, "dpwa_unpack: a NULL pointer, one event without the other, or max_blocks < 1");
    if (!aligned16(payload_out, image))
        return set_error(DPWA_ERR_ARG, "dpwa_unpack: the image or the payload is not 16-byte aligned (there is no unaligned form)");
    HIP_TRY(launch_pull_unpack(dtype, payload_out, n, image, nullptr, nullptr, max_blocks, false, (hipStream_t)stream,
                               CallerTiming(start_event, stop_event)));
    return DPWA_OK;
}

// dpwa_average with the peer's payload still packed: dpwa_unpack into a buffer and dpwa_average from it, in one
// launch and without the buffer (k_lerp_packed).
int dpwa_average_packed(int32_t dtype, void *param, const void *header, const void *image, int64_t n,
                        const dpwa_interp *cfg, double *clock_dev, double loss, dpwa_coef *coef_dev, void *snap_payload,
                        dpwa_stream_t stream, void *start_event, void *stop_event)
{
    if (const char *why = pack_problem(dtype, n)) return set_error(DPWA_ERR_ARG, "dpwa_average_packed: %s", why);
    if (!cfg || !clock_dev || !coef_dev || !header || !image || (n > 0 && !param) || (!start_event) != (!stop_event))
        return set_error(DPWA_ERR_ARG, "dpwa_average_packed: a NULL pointer, or one event without the other");
    if (int rc = check_method(cfg, "dpwa_average_packed")) return rc;
    if (!aligned16(param, image, snap_payload))
        return set_error(DPWA_ERR_ARG, "dpwa_average_packed: the parameters, the image or the snapshot payload is not "
                                       "16-byte aligned (there is no unaligned form)");
    const FusedArgs fa = stateless_args(cfg, clock_dev, header, loss, coef_dev);
    HIP_TRY(launch_average_packed(dtype, param, n, image, fa, snap_payload, (hipStream_t)stream,
                                  CallerTiming(start_event, stop_event)));
    return DPWA_OK;
}

// dpwa_average (peer_payload) or dpwa_average_packed (peer_image) writing through to snap_payload, and dpwa_pack of
// that snapshot into image_out, in one launch (k_lerp_emit).
static int average_pack_entry(const char *fn, int32_t dtype, void *param, const void *header, const void *peer_payload,
                              const void *peer_image, int64_t n, const dpwa_interp *cfg, double *clock_dev, double loss,
                              dpwa_coef *coef_dev, void *snap_payload, void *image_out, PackRounding rounding,
                              dpwa_stream_t stream, void *start_event, void *stop_event)
{
    if (const char *why = pack_problem(dtype, n)) return set_error(DPWA_ERR_ARG, "%s: %s", fn, why);
    if (!cfg || !clock_dev || !coef_dev || !header || !param || !snap_payload || !image_out ||
        (!start_event) != (!stop_event))
        return set_error(DPWA_ERR_ARG, "%s: a NULL pointer, or one event without the other", fn);
    if ((!peer_payload) == (!peer_image))
        return set_error(DPWA_ERR_ARG, "%s: exactly one of peer_payload and peer_image", fn);
    if (snap_payload == param) return set_error(DPWA_ERR_ARG, "%s: snap_payload is the parameters", fn);
    if (int rc = check_method(cfg, fn)) return rc;
    if (!aligned16(param, peer_payload, peer_image) || !aligned16(snap_payload, image_out))
        return set_error(DPWA_ERR_ARG, "%s: the parameters, the peer's payload or image, the snapshot payload "
                                       "or the image is not 16-byte aligned (there is no unaligned form)", fn);
    const FusedArgs fa = stateless_args(cfg, clock_dev, header, loss, coef_dev);
    HIP_TRY(launch_average_emit(dtype, param, n, peer_payload, peer_image, fa, snap_payload, image_out,
                                (hipStream_t)stream, CallerTiming(start_event, stop_event), rounding));
    return DPWA_OK;
}

int dpwa_average_pack(int32_t dtype, void *param, const void *header, const void *peer_payload, const void *peer_image,
                      int64_t n, const dpwa_interp *cfg, double *clock_dev, double loss, dpwa_coef *coef_dev,
                      void *snap_payload, void *image_out, dpwa_stream_t stream, void *start_event, void *stop_event)
{
    return average_pack_entry("dpwa_average_pack", dtype, param, header, peer_payload, peer_image, n, cfg, clock_dev, loss,
                              coef_dev, snap_payload, image_out, PackRounding{}, stream, start_event, stop_event);
}

int dpwa_average_pack_stochastic(int32_t dtype, void *param, const void *header, const void *peer_payload,
                                 const void *peer_image, int64_t n, const dpwa_interp *cfg, double *clock_dev,
                                 double loss, dpwa_coef *coef_dev, void *snap_payload, void *image_out,
                                 dpwa_stream_t stream, void *start_event, void *stop_event, uint64_t nonce)
{
    return average_pack_entry("dpwa_average_pack_stochastic", dtype, param, header, peer_payload, peer_image, n, cfg,
                              clock_dev, loss, coef_dev, snap_payload, image_out, PackRounding{true, nonce}, stream,
                              start_event, stop_event);
}

// dpwa_pack behind a device-side condition (k_pack_if): the form a learner's reuse guard runs.
int dpwa_pack_if(int32_t dtype, const void *payload, int64_t n, void *image, const int32_t *dirty_dev, int32_t gen,
                 dpwa_stream_t stream, void *start_event, void *stop_event)
{
    if (const char *why = pack_problem(dtype, n)) return set_error(DPWA_ERR_ARG, "dpwa_pack_if: %s", why);
    if (!payload || !image || !dirty_dev || (!start_event) != (!stop_event))
        return set_error(DPWA_ERR_ARG, "dpwa_pack_if: a NULL pointer, or one event without the other");
    if (!aligned16(payload, image))
        return set_error(DPWA_ERR_ARG, "dpwa_pack_if: the payload or the image is not 16-byte aligned (there is no unaligned form)");
    HIP_TRY(launch_pack_if(dtype, payload, n, image, dirty_dev, gen, (hipStream_t)stream,
                           CallerTiming(start_event, stop_event)));
    return DPWA_OK;
}

}  // extern "C"
