/*
 * dpwa_hip.h -- C ABI of libdpwa_hip.so, the MI355X-native pairwise-averaging hot path.
 *
 * The reference (zenghanfu/dpwa) is pure Python; its hot path is the adapter/connection
 * seam below, which this library replaces.  Every entry point names the reference
 * interface it stands in for.  A maintainer binds it with ctypes;
 * dpwa_amd/_lib.py is that binding.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Device pointers are HIP device addresses on the
 *    learner's GPU; `dpwa_stream_t` is a hipStream_t (NULL = the legacy default stream).
 *  - Every function returns DPWA_OK (0) or a negative DPWA_ERR_*; the message of the
 *    last failure on the calling thread is available from dpwa_last_error().
 *  - The library never allocates or frees caller memory.  Learner-owned snapshot and
 *    staging buffers are allocated at dpwa_learner_create() with hipMalloc.
 *  - No host synchronisation happens inside publish / fetch / average: the factor is
 *    computed on the device from the (clock, loss) state and handed to the lerp through
 *    device memory (dpwa_coef), so a whole round can be enqueued without a sync.
 *  - There is no CPU fallback: without a HIP device the compute entry points fail.
 */
#ifndef DPWA_HIP_H
#define DPWA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 11: DPWA_F16 -- float16 parameters through every averaging form, dpwa_lerp_f16{,_host}.
 * Still 11, by additions only (every ABI-11 caller runs unchanged): DPWA_MIXED -- segmented payloads
 * (dpwa_layout): dpwa_average_mixed, dpwa_layout_digest, dpwa_learner_set_layout,
 * dpwa_node_set_layout; the IPC handle carries the layout digest in bytes that were zero.
 * Still 11, by additions only: the distance to the peer (dpwa_distance) -- dpwa_distance_workspace,
 * dpwa_measure_distance, dpwa_measure_distance_mixed, dpwa_average_tracked, dpwa_distance_finish,
 * dpwa_learner_set_distance, dpwa_learner_distance.
 * Still 11, by additions only: the distance to the peer for every parameter tensor (dpwa_param_range)
 * -- dpwa_param_ranges_check, dpwa_param_distance_sizes, dpwa_param_distance_table,
 * dpwa_measure_param_distance, dpwa_param_distance_finish, dpwa_learner_set_param_distance,
 * dpwa_learner_param_distance, dpwa_learner_param_distance_rounds.
 * Still 11, by additions only: skipping a round whose peer snapshot is not finite
 * (DPWA_STATUS_PEER_NONFINITE, a new value of dpwa_coef.status) -- dpwa_check_finite,
 * dpwa_check_finite_mixed, dpwa_learner_set_finite_check, dpwa_learner_finite_skips,
 * dpwa_node_set_finite_check.
 * Still 11, by additions only: the consensus of a group (dpwa_consensus_record) --
 * dpwa_consensus_workspace, dpwa_consensus, dpwa_consensus_mixed, dpwa_learner_consensus. */
#define DPWA_ABI_VERSION 11

#define DPWA_OK 0
#define DPWA_ERR_ARG (-1)     /* bad argument (API misuse)                          */
#define DPWA_ERR_HIP (-2)     /* a HIP runtime call failed                          */
#define DPWA_ERR_STATE (-3)   /* call out of order (e.g. average without a fetch)   */
#define DPWA_ERR_NOMEM (-4)

/* element types of the flat parameter buffer */
#define DPWA_F32 0            /* the reference's only type: TYPE_CONVERSION, pytorch.py:11-14 */
#define DPWA_BF16 1           /* extension: torch-eager bf16 rounding, no reference path      */
#define DPWA_F64 2            /* loss scalars only (dpwa_learner_set_loss_dtype)              */
#define DPWA_F16 3            /* extension: torch-eager fp16 rounding, no reference path       */
#define DPWA_MIXED 4          /* extension: a segmented payload of the three types above; its element is
                                 one byte (n = payload bytes) and a dpwa_layout says which bytes hold what */

/* interpolation methods: INTERPOLATION_METHODS, dpwa/dpwa.py:11-15 */
#define DPWA_INTERP_CONSTANT 0   /* interpolation.py:8-15  factor = value                       */
#define DPWA_INTERP_CLOCK 1      /* interpolation.py:18-24 factor = peer_clock/(clock+peer_clock) */
#define DPWA_INTERP_LOSS 2       /* interpolation.py:27-33 factor = loss/(loss+peer_loss)         */

/* status written into dpwa_coef.status by the factor kernel */
#define DPWA_STATUS_OK 0
#define DPWA_STATUS_ZERO_DIVISION 1   /* the reference raises ZeroDivisionError (dpwa.py:143) */
#define DPWA_STATUS_PEER_NONFINITE 2  /* no error: the round was skipped because the peer's snapshot held a NaN
                                         or an inf (dpwa_learner_set_finite_check); never the sticky status */

typedef void *dpwa_stream_t;

/* The published `state` of one learner (dpwa.py:115 `{'clock', 'loss'}`), stored as the
 * first 256 bytes of every snapshot slot so that state and parameters travel together
 * exactly as RxThread sends them together (conn.py:110). */
/* A snapshot slot is [dpwa_header | zero pad | payload]: the payload starts 4 KiB into the
 * slot, so every 1-KiB wave span of the averaging kernel lies inside one aligned 1-KiB block
 * (a payload right behind the 256-B header made each span straddle two: 0.7 % slower at
 * 11.17M fp32 and 2 % at 100M, tools/skew_tune.hip). */
#define DPWA_SLOT_PAYLOAD_OFFSET 4096
typedef struct dpwa_header {
    double clock;        /* publisher's clock after `clock += 1` (dpwa.py:112)           */
    double loss;         /* loss given to update_send (dpwa.py:115)                      */
    uint64_t version;    /* publishes so far; 0 = never published (have_state, conn.py:60) */
    int64_t n;           /* payload elements                                              */
    int32_t dtype;       /* DPWA_F32 / BF16 / F16 / MIXED: what a peer checks first      */
    int32_t reserved0;
    uint8_t pad[216];
} dpwa_header;

/* Averaging coefficients, produced on the device by the factor kernel (dpwa.py:143-150)
 * and consumed by the lerp (pytorch.py:68). */
typedef struct dpwa_coef {
    double factor;       /* interpolation factor after divergence scaling (dpwa.py:143-147) */
    double new_clock;    /* factor*peer_clock + (1-factor)*clock (dpwa.py:150)              */
    float a;             /* f32(factor)        -- torch casts the scalar to fp32            */
    float b;             /* f32(1.0 - factor)  -- `1 - factor` is a Python double           */
    int32_t status;      /* DPWA_STATUS_*; non-zero makes the lerp a no-op                  */
    int32_t reserved;
} dpwa_coef;

/* Interpolation configuration (DpwaConfiguration.get_interpolation / get_divergence_threshold,
 * dpwa.py:40-51). */
typedef struct dpwa_interp {
    int32_t method;               /* DPWA_INTERP_*                                 */
    int32_t reserved;
    double value;                 /* constant value (ConstantInterpolation)        */
    double divergence_threshold;  /* 0 disables (README.md:62)                     */
} dpwa_interp;

/* The layout of a DPWA_MIXED payload (a model that mixes parameter dtypes): 1..3 segments, one per
 * element type, each a whole number of 4 KiB blocks -- so no 16-byte word, no 1-KiB wave span and no
 * relay stripe (4 KiB multiples) ever holds two types.  A valid layout has segment 0 at byte 0, every
 * segment beginning where the one before ends (ascending, no overlap, no hole), byte_offset and
 * byte_length positive multiples of DPWA_LAYOUT_ALIGN (the offset may be 0), every dtype one of
 * DPWA_F32 / DPWA_BF16 / DPWA_F16 and none repeated.  Bytes of a segment no parameter occupies are
 * zero and average to zero. */
#define DPWA_LAYOUT_MAX_SEGMENTS 3
#define DPWA_LAYOUT_ALIGN 4096
typedef struct dpwa_segment {
    int32_t dtype;        /* DPWA_F32 / DPWA_BF16 / DPWA_F16 */
    int32_t reserved;
    int64_t byte_offset;  /* from the payload's first byte */
    int64_t byte_length;
} dpwa_segment;
typedef struct dpwa_layout {
    int32_t count;        /* segments in use, 1..DPWA_LAYOUT_MAX_SEGMENTS */
    int32_t reserved;
    dpwa_segment seg[DPWA_LAYOUT_MAX_SEGMENTS];
} dpwa_layout;

const char *dpwa_last_error(void);
int dpwa_abi_version(void);

/* Validates `layout` (DPWA_ERR_ARG with a message naming the rule it breaks; total_bytes >= 0: it
 * must also cover exactly that many bytes) and returns its 32-bit digest, what two peers compare
 * before they average each other's bytes: FNV-1a (offset basis 2166136261, prime 16777619) over, for
 * each segment in order, the little-endian bytes of dtype (4), byte_offset (8) and byte_length (8);
 * a result of 0 is replaced by 1, so 0 always means "no layout".  No device is needed.
 * dpwa_amd/flat.py layout_digest mirrors it. */
int dpwa_layout_digest(const dpwa_layout *layout, int64_t total_bytes, uint32_t *digest);

/* roctx ranges on the round (the reference's LOGGER.debug sites dpwa.py:119,152-153,
 * conn.py:242-243,296).  On only when DPWA_ROCTX=1 is set when the library loads: then
 * dpwa.update_send / dpwa.publish / dpwa.fetch_loop / dpwa.update_wait_average / dpwa.average
 * (and the learner's publish) are pushed as ranges that `rocprofv3 --marker-trace` records.
 * dpwa_trace_push/pop let the layer above add its own (no-ops when off).  ABI version 8. */
int dpwa_trace_enabled(void);
int dpwa_trace_push(const char *name);
int dpwa_trace_pop(void);

/* Last words (bench.py's held result line): registers `line` (len bytes, at most 16 KiB; len 0
 * clears it) to be written to `fd` with write(2) if the process is ended by SIGTERM, SIGINT,
 * SIGHUP, SIGABRT, SIGSEGV, SIGBUS, SIGFPE or SIGILL; the handler then restores the previous
 * handler and re-raises.  The first call installs the handlers.  dpwa_last_words_flush writes
 * the registered line now; the line is written at most once, by the flush or by a signal,
 * whichever claims it first (*wrote = 1 when the flush did).  ABI version 10. */
int dpwa_last_words_set(int fd, const char *line, int64_t len);
int dpwa_last_words_flush(int *wrote);
int dpwa_last_words_written(int *written);

/* ------------------------------------------------------------------------------------
 * Stateless kernels (the fused replacements of the ATen mul/mul/add behind pytorch.py:68)
 * ------------------------------------------------------------------------------------ */

/* param[i] = f32(f32(a*peer[i]) + f32(b*param[i])) with (a, b) read from coef_dev on the
 * device (no host sync).  Replaces the per-tensor loop dpwa/adapters/pytorch.py:66-68 with
 * one launch over the flat buffer.  In place; param and peer may not overlap. */
int dpwa_lerp_f32(float *param, const float *peer, int64_t n, const dpwa_coef *coef_dev,
                  dpwa_stream_t stream);
/* bf16 form: bf16(bf16(a*peer) + bf16(b*param)), RNE (torch-eager bf16). */
int dpwa_lerp_bf16(uint16_t *param, const uint16_t *peer, int64_t n, const dpwa_coef *coef_dev,
                   dpwa_stream_t stream);
/* fp16 form: f16(f16(a*peer) + f16(b*param)), RNE, subnormals kept (torch-eager float16).  bf16 and
 * fp16 elements have the same size: the dtype code is all that tells them apart.  ABI version 11. */
int dpwa_lerp_f16(uint16_t *param, const uint16_t *peer, int64_t n, const dpwa_coef *coef_dev,
                  dpwa_stream_t stream);
/* Same kernels with the factor given by the host, as pytorch.py:68 receives it. */
int dpwa_lerp_f32_host(float *param, const float *peer, int64_t n, double factor, dpwa_stream_t stream);
int dpwa_lerp_bf16_host(uint16_t *param, const uint16_t *peer, int64_t n, double factor,
                        dpwa_stream_t stream);
int dpwa_lerp_f16_host(uint16_t *param, const uint16_t *peer, int64_t n, double factor,
                       dpwa_stream_t stream);

/* The fused average of dpwa_learner_average without a learner (the product kernel over
 * caller-owned buffers): reads clock_dev[0] and the 256-B dpwa_header at `peer_slot`, lerps the
 * n elements at peer_slot + DPWA_SLOT_PAYLOAD_OFFSET into `param` in place, writes clock_dev[1] = new clock and
 * *coef_dev.  snap_payload (NULL or n elements): the write-through form, which also stores the
 * result there (dpwa_learner_average_through).  start_event/stop_event (hipEvent_t, both or neither): the kernel is launched with
 * hipExtLaunchKernelGGL so they record its own begin and end (measurement). */
int dpwa_average(int32_t dtype, void *param, const void *peer_slot, int64_t n, const dpwa_interp *cfg,
                 double *clock_dev, double loss, dpwa_coef *coef_dev, void *snap_payload, dpwa_stream_t stream,
                 void *start_event, void *stop_event);

/* dpwa_average for a DPWA_MIXED payload: `layout` in place of (dtype, n).  param, the payload at
 * peer_slot + DPWA_SLOT_PAYLOAD_OFFSET and snap_payload (NULL or as large) are 16-B aligned buffers of
 * the layout's total bytes; every segment is averaged with its own type's rounding (exactly what
 * dpwa_average computes on that segment alone), the new clock and *coef_dev are written once.
 * DPWA_ERR_ARG for an invalid layout or an unaligned pointer.  Events as dpwa_average. */
int dpwa_average_mixed(const dpwa_layout *layout, void *param, const void *peer_slot, const dpwa_interp *cfg,
                       double *clock_dev, double loss, dpwa_coef *coef_dev, void *snap_payload, dpwa_stream_t stream,
                       void *start_event, void *stop_event);

/* The distance to the peer (extension, opt-in; no reference interface): how far the parameters p
 * were from the snapshot q they were averaged with, both read BEFORE the average, over the n elements:
 *   dist2 = sum (double(q_i) - double(p_i))^2      norm2 = sum double(p_i)^2
 * every element widened exactly to fp64, every difference, product and sum in fp64; subnormals count,
 * a NaN anywhere gives NaN, no finite input overflows; padding bytes of a DPWA_MIXED layout are zeros
 * and add 0.  `clock` is the clock the round committed (which round the sums belong to; 0 from the
 * stateless dpwa_measure_distance); `n` the elements summed over (a DPWA_MIXED payload: the element
 * slots of its segments, padding included).  A round that does not average (no fetch, or the
 * ZeroDivision no-op) leaves the record untouched.  The sums are added across workgroups with hardware
 * fp64 atomic adds, whose order is not fixed: the record is this library's one output that is NOT
 * bit-exact from run to run -- it is reproducible to (n - 1) * 2^-53 relative (every term is >= 0).
 *
 * workspace: dpwa_distance_workspace() bytes of ordinary device memory (hipMalloc), 16-B aligned, zero
 * before the first use; every entry below leaves it zero again, so one workspace serves any number of
 * rounds of one stream (not two streams at once).  Its size does not depend on n: it holds
 * bytes / DPWA_DISTANCE_ACC_STRIDE accumulators, and the 1-KiB span s of the operands adds into
 * accumulator s modulo that count.
 *   dpwa_measure_distance        the stand-alone pass: reads n elements of `param` and of `peer_payload`
 *                                (any element alignment), stores nothing to either, writes *out_dev.
 *   dpwa_measure_distance_mixed  the same for a DPWA_MIXED payload (16-B aligned buffers of the layout's bytes).
 *   dpwa_average_tracked         dpwa_average whose kernel also forms the sums from the operands it holds
 *                                in registers anyway (no extra bytes): the averaged parameters, the
 *                                snapshot, the clock and *coef_dev are exactly dpwa_average's.  16-B
 *                                aligned operands run the tracked kernel; others the stand-alone pass
 *                                followed by dpwa_average's kernel.  The events time the averaging kernel.
 *   dpwa_distance_finish         the finishing step alone (what the entries above end with): sums the
 *                                accumulators into *out_dev and zeroes them; coef_dev non-NULL: the record
 *                                is written only when its status is DPWA_STATUS_OK, with its new_clock.
 *                                Events as dpwa_average (measurement).
 * DPWA_ERR_ARG (no device touched) for NULL pointers, n < 0, an unknown dtype, DPWA_MIXED without its
 * layout, an invalid layout or a misaligned workspace / record. */
#define DPWA_DISTANCE_ACC_STRIDE 128
typedef struct dpwa_distance {
    double dist2;
    double norm2;
    double clock;
    int64_t n;
} dpwa_distance;
int dpwa_distance_workspace(int64_t *bytes);
int dpwa_measure_distance(int32_t dtype, const void *param, const void *peer_payload, int64_t n, void *workspace,
                          dpwa_distance *out_dev, dpwa_stream_t stream);
int dpwa_measure_distance_mixed(const dpwa_layout *layout, const void *param, const void *peer_payload,
                                void *workspace, dpwa_distance *out_dev, dpwa_stream_t stream);
int dpwa_average_tracked(int32_t dtype, void *param, const void *peer_slot, int64_t n, const dpwa_interp *cfg,
                         double *clock_dev, double loss, dpwa_coef *coef_dev, void *snap_payload, void *workspace,
                         dpwa_distance *out_dev, dpwa_stream_t stream, void *start_event, void *stop_event);
int dpwa_distance_finish(void *workspace, dpwa_distance *out_dev, const dpwa_coef *coef_dev, int64_t n,
                         dpwa_stream_t stream, void *start_event, void *stop_event);

/* The non-finite check of a peer payload (extension; stateless, for tests and tools -- a learner runs it
 * itself, dpwa_learner_set_finite_check).  One read of the n elements at `peer_payload`; an element is
 * non-finite when its exponent field is all ones (fp32 0x7f800000, bf16 0x7f80, fp16 0x7c00; a test
 * on bit patterns, so NaNs of either kind and +-inf, never a subnormal or the largest finite value).
 * When there is one, `stamp` (non-zero) is stored into the 32-bit word *veto_dev (device memory,
 * 4-byte aligned); otherwise the word is left as it was, so a caller that passes a fresh stamp every
 * time never has to clear it.  dtype DPWA_F32 / BF16 / F16, the payload aligned to its element;
 * dpwa_check_finite_mixed: a DPWA_MIXED payload (16-B aligned, the layout's bytes; each segment by its
 * own type, padding is zeros).  Events as dpwa_average.  DPWA_ERR_ARG, no device touched, for NULL
 * or misaligned pointers, n < 0, stamp 0, an unknown dtype or an invalid layout. */
int dpwa_check_finite(int32_t dtype, const void *peer_payload, int64_t n, uint32_t *veto_dev, uint32_t stamp,
                      dpwa_stream_t stream, void *start_event, void *stop_event);
int dpwa_check_finite_mixed(const dpwa_layout *layout, const void *peer_payload, uint32_t *veto_dev, uint32_t stamp,
                            dpwa_stream_t stream, void *start_event, void *stop_event);

/* The consensus of a group (extension, opt-in, read-only; no reference interface): the element-wise
 * mean of `count` (1..DPWA_CONSENSUS_MAX) payloads of one dtype and n -- the model a gossip run
 * evaluates and saves -- and the group's consensus distance, in ONE pass that reads every payload once
 * ((count + 1) * n * s bytes with the store, no temporaries).  For every element j, the members in the
 * order given:
 *   s = ((x_0[j] + x_1[j]) + ...) + x_{count-1}[j]   each operand widened exactly to fp64, fp64 adds
 *   m = s * r                                        r = the fp64 1.0 / count, formed once on the host
 *   out[j] = f32(m), round to nearest even, subnormals kept; a bf16 / fp16 payload then rounds that fp32
 *            value to nearest even once more (two roundings, as documented, not one from fp64)
 *   norm2 = sum m^2      member_spread2[i] = sum (x_i[j] - m)^2      spread2 = sum_i member_spread2[i]
 * all in fp64 against the fp64 m (not the stored mean).  The consensus distance is sqrt(spread2 / count).
 * The means are bit-exact; the sums are added across workgroups as dpwa_distance's are, so they are
 * reproducible to the same summation bound and not bit-exact from run to run.
 *   out NULL                        measure only: nothing is stored to any payload
 *   workspace and record_dev NULL   the mean only (both or neither)
 * workspace: dpwa_consensus_workspace() bytes (= dpwa_distance_workspace()), 16-B aligned, zero before the
 * first use, left zero by every call.  record_dev: 8-B aligned device memory, written whole.  `version`
 * in the record is 0 from the stateless entries.  Payloads and out are 16-B aligned (there is no unaligned
 * form); out may not overlap a payload.  dpwa_consensus_mixed: a DPWA_MIXED payload (`layout` in place of
 * dtype and n; every segment with its own type's rounding; padding bytes are zeros in every member, their
 * mean is zero and they add 0; record n = the element slots of the segments).  Events as dpwa_average
 * (they time the pass, not the finishing step).  DPWA_ERR_ARG, nothing queued: a count outside
 * 1..DPWA_CONSENSUS_MAX, a NULL or misaligned pointer, out overlapping a payload, n < 0, an unknown dtype,
 * an invalid layout, neither out nor a record, a workspace without a record or the reverse. */
#define DPWA_CONSENSUS_MAX 8
typedef struct dpwa_consensus_record {
    double norm2;
    double spread2;
    double member_spread2[DPWA_CONSENSUS_MAX];   /* in the order of the payloads; 0 beyond `members` */
    int64_t n;
    int32_t members;
    int32_t reserved;
    uint64_t version;
    uint64_t pad[3];
} dpwa_consensus_record;
int dpwa_consensus_workspace(int64_t *bytes);
int dpwa_consensus(int32_t dtype, const void *const *payloads, int count, int64_t n, void *out, void *workspace,
                   dpwa_consensus_record *record_dev, dpwa_stream_t stream, void *start_event, void *stop_event);
int dpwa_consensus_mixed(const dpwa_layout *layout, const void *const *payloads, int count, void *out, void *workspace,
                         dpwa_consensus_record *record_dev, dpwa_stream_t stream, void *start_event, void *stop_event);

/* The per-parameter distance (extension, opt-in): the two sums above for every parameter tensor t of
 * the model, over that tensor's own elements only -- dist2_t = sum (double(q_i) - double(p_i))^2 and
 * norm2_t = sum double(p_i)^2 with dpwa_distance's arithmetic.  Where the tensors lie in the payload
 * is a list of dpwa_param_range:
 *   - ascending and non-overlapping: byte_offset[t] >= byte_offset[t-1] + byte_length[t-1];
 *   - byte_offset a multiple of DPWA_PARAM_ALIGN (256); byte_length a multiple of the element size,
 *     0 allowed (an empty tensor reports (0, 0));
 *   - dtype DPWA_F32, DPWA_BF16 or DPWA_F16; reserved 0;
 *   - every range inside the payload -- of a single-dtype payload of n elements, with that dtype; of a
 *     DPWA_MIXED payload, wholly inside the segment of its dtype.
 * Bytes of no range (the gaps between tensors, a segment's padding) are NOT read into any sum: unlike
 * the whole-model record this one does not rely on them being zero, and a NaN there shows in no tensor.
 * Each dist2_t / norm2_t is reproducible to (n_t - 1) * 2^-53 relative, like the whole-model record.
 *
 * The record is a dpwa_param_distance_head followed by `count` dpwa_param_pair, in the ranges' order;
 * `clock` as dpwa_distance's.  The table (the ranges as the kernels read them) and the workspace are
 * caller-owned device memory of the sizes dpwa_param_distance_sizes gives, 16-B aligned; the workspace
 * zero before the first use (every entry below leaves it zero again; one stream at a time).  Tensor t
 * owns min(the 1-KiB spans of the payload it touches, max_rows) accumulators of DPWA_DISTANCE_ACC_STRIDE
 * bytes each, and its span s adds into accumulator s modulo that count.
 *   dpwa_param_ranges_check      the rules above against a payload: (dtype, n) for a single dtype, or
 *                                DPWA_MIXED with its layout.  Needs no device.
 *   dpwa_param_distance_sizes    the bytes of table, workspace and record for the ranges (checks the
 *                                rules that need no payload).  Needs no device.
 *   dpwa_param_distance_table    writes the table to `table_dev` (a blocking copy).
 *   dpwa_measure_param_distance  the pass over `payload_bytes` of `param` and `peer_payload` (16-B aligned,
 *                                any form of payload the table was made for), then the finishing step:
 *                                writes the whole record, clock 0.  The events time the pass.  The table is
 *                                opaque device memory and is not checked against payload_bytes here: make
 *                                it from ranges that dpwa_param_ranges_check accepts for this payload.
 *                                Nothing is read beyond payload_bytes whatever the table says; elements of
 *                                a range that ends beyond it count as zeros.
 *   dpwa_param_distance_finish   the finishing step alone: one workgroup per tensor sums its accumulators
 *                                in a fixed order and zeroes them; the record is written only when
 *                                coef_dev is NULL or its status is DPWA_STATUS_OK (clock: its new_clock).
 *                                The events time it.
 * DPWA_ERR_ARG (no device touched) with a message naming the broken rule, for NULL or misaligned
 * pointers, count < 1 (count < 0 for the check and the sizes), payload_bytes < 0. */
#define DPWA_PARAM_ALIGN 256
typedef struct dpwa_param_range {
    int64_t byte_offset;
    int64_t byte_length;
    int32_t dtype;
    int32_t reserved;
} dpwa_param_range;
typedef struct dpwa_param_pair {
    double dist2;
    double norm2;
} dpwa_param_pair;
typedef struct dpwa_param_distance_head {
    double clock;
    int64_t count;
    /* dpwa_param_pair pair[count] follows */
} dpwa_param_distance_head;
typedef struct dpwa_param_sizes {
    int64_t table_bytes;
    int64_t workspace_bytes;
    int64_t record_bytes;
    int32_t max_rows;   /* accumulators of the largest tensors (the modulus above) */
    int32_t reserved;
} dpwa_param_sizes;
int dpwa_param_ranges_check(const dpwa_param_range *ranges, int64_t count, int32_t dtype, int64_t n,
                            const dpwa_layout *layout);
int dpwa_param_distance_sizes(const dpwa_param_range *ranges, int64_t count, dpwa_param_sizes *sizes);
int dpwa_param_distance_table(const dpwa_param_range *ranges, int64_t count, void *table_dev);
int dpwa_measure_param_distance(const void *table_dev, int64_t count, const void *param, const void *peer_payload,
                                int64_t payload_bytes, void *workspace, dpwa_param_distance_head *out_dev,
                                dpwa_stream_t stream, void *start_event, void *stop_event);
int dpwa_param_distance_finish(const void *table_dev, int64_t count, void *workspace,
                               dpwa_param_distance_head *out_dev, const dpwa_coef *coef_dev, dpwa_stream_t stream,
                               void *start_event, void *stop_event);

/* dpwa_average over several independent (param, peer slot) pairs in ONE dispatch -- the averages
 * of co-resident learners of one round (pytorch.py:66-68 once per learner).  Each descriptor is
 * one dpwa_average call: its own clock_dev (reads [0], writes [1]), coefficient block and loss;
 * all share `cfg` and `dtype`, and either all or none write through (snap_payload).  Every
 * pointer 16-B aligned; 1..8 descriptors.  Events as dpwa_average (the whole dispatch).
 * DPWA_MIXED is refused (DPWA_ERR_ARG): segmented payloads are not batched. */
typedef struct dpwa_average_desc {
    void *param;
    const void *peer_slot;   /* [dpwa_header | pad | payload] */
    int64_t n;
    double *clock_dev;
    double loss;
    dpwa_coef *coef_dev;
    void *snap_payload;      /* NULL, or n elements: the write-through destination */
} dpwa_average_desc;
int dpwa_average_many(int32_t dtype, const dpwa_average_desc *descs, int count, const dpwa_interp *cfg,
                      dpwa_stream_t stream, void *start_event, void *stop_event);
/* The same in the resident form (dpwa_learner_set_resident below): each `param` is read only and the
 * result goes to its snap_payload (required for n > 0) -- 3*n*s bytes per descriptor.  One
 * descriptor runs the single-learner kernel, several the batched one.  Equal-size descriptors whose
 * reads overlap (a `param` is another descriptor's peer payload, or two share a peer: co-resident
 * learners that picked each other, e.g. a mutual pair) run one fused pass that reads each distinct
 * buffer once, up to 8 of them; beyond that the repeated reads are dispatched to hit L2. */
int dpwa_average_many_resident(int32_t dtype, const dpwa_average_desc *descs, int count, const dpwa_interp *cfg,
                               dpwa_stream_t stream, void *start_event, void *stop_event);

/* Factor + clock on the device (dpwa.py:139-155 + interpolation.py): reads *clock_dev and the
 * peer's header, writes *coef_dev and, unless the status is an error, *clock_dev = new_clock.
 * `loss` is used when loss_dev is NULL, else *loss_dev (a device float64). */
int dpwa_factor(const dpwa_interp *cfg, double *clock_dev, const dpwa_header *peer_header_dev, double loss,
                const double *loss_dev, dpwa_coef *coef_dev, dpwa_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Learner runtime: one per gossip node.  Owns two snapshot slots (double-buffered
 * RxThread.set_current_state, conn.py:73-79), a staging buffer (the fetched
 * TxThread.peer_payload, conn.py:298), the device clock and the coefficient block.
 * ------------------------------------------------------------------------------------ */
typedef struct dpwa_learner dpwa_learner;

int dpwa_learner_create(dpwa_learner **out, int device, int64_t n, int32_t dtype, const dpwa_interp *cfg);
/* A learner created as DPWA_MIXED (n = payload bytes) is given its layout here, before it is
 * attached to peers and before its first average: DPWA_ERR_ARG for a learner of another dtype, a
 * layout that is invalid or does not cover exactly n bytes; DPWA_ERR_STATE for a second, different
 * layout.  Without one, publishes and pulls work (they move bytes) and every average, factor-then-lerp
 * included, is DPWA_ERR_STATE.  Peers must hold the same layout: attach_local and the IPC attach
 * compare its digest next to n and dtype.  Mixed learners are never batched
 * (dpwa_learner_average_many gives each its own launch) and refuse the relay's fused second phase
 * (dpwa_learner_relay_phase2 with fuse != 0). */
int dpwa_learner_set_layout(dpwa_learner *l, const dpwa_layout *layout);

/* Measurement only (bench.py `roofline.mix_ceiling`; no reference interface): the averaging
 * kernels' access mix with nothing else in it -- every 1-KiB span of `nr` (1-2) source buffers
 * loaded and one sum of them stored into `nw` (1-2) destinations, `nbytes` (a multiple of 16)
 * each, with the product kernel's launch shape and cache policy.  nr = 2, nw = 2 is the
 * write-through average's mix (read parameters and snapshot, write parameters and next
 * snapshot).  start/stop: optional dispatch begin/end events. */
int dpwa_stream_mix(void *const *dst, int nw, const void *const *src, int nr, int64_t nbytes, dpwa_stream_t stream,
                    void *start_event, void *stop_event);
int dpwa_learner_destroy(dpwa_learner *l);

/* update_send's publish half (dpwa.py:111-116 + pytorch.py:49-53): clock += 1 on the device,
 * copy the n-element flat buffer into the next snapshot slot with header {clock, loss,
 * version}.  Stream-ordered after prior work on `stream`. */
int dpwa_learner_publish(dpwa_learner *l, const void *flat, double loss, const double *loss_dev,
                         dpwa_stream_t stream);
/* Number of publishes so far (host counter, no sync). */
int dpwa_learner_version(const dpwa_learner *l, uint64_t *version);

/* Peers.  `peer_id` is the caller's index of that peer (e.g. its node index).
 * attach_local: the peer learner lives in this process (any device); peer == l is the
 * self-peer (a YAML node at the learner's own host:port: its own published snapshot).
 * ipc_handle / attach_ipc: the peer lives in another process; ipc_handle describes the
 * snapshot allocation (handle_len = DPWA_IPC_HANDLE_BYTES) and, for an ordinary allocation,
 * carries its hipIpcGetMemHandle.  Allocations of 1.5 GiB and more (or any size with
 * DPWA_VMM=1) are hipMemCreate chunks instead -- hipIpcOpenMemHandle does not return for
 * allocations above ~2 GiB on this ROCm stack -- and are shared as POSIX fds:
 * export_fds (which = 0: snapshot slots, 1: relay buffer) yields one fd per chunk, *n_fds = 0
 * for an ordinary allocation; the caller passes them to the peer process (e.g. SCM_RIGHTS over
 * a Unix socket) and closes its copies; the peer maps them with attach_fds (the fds stay the
 * caller's). */
#define DPWA_IPC_HANDLE_BYTES 128
int dpwa_learner_attach_local(dpwa_learner *l, int peer_id, dpwa_learner *peer);
int dpwa_learner_ipc_handle(dpwa_learner *l, void *handle_out, int64_t handle_len);
int dpwa_learner_attach_ipc(dpwa_learner *l, int peer_id, const void *handle, int64_t handle_len);
int dpwa_learner_export_fds(dpwa_learner *l, int which, int *fds, int max_fds, int *n_fds, int64_t *chunk_bytes);
int dpwa_learner_attach_fds(dpwa_learner *l, int peer_id, const void *handle, int64_t handle_len, const int *fds,
                            int n_fds, int64_t chunk_bytes);

/* The fetch (TxThread request -> reply, conn.py:297-298): pull peer `peer_id`'s snapshot of
 * publish number `peer_version` (1-based) into this learner's staging buffer on the
 * learner's side stream, after all work already enqueued on `stream`.  flags:
 * DPWA_FETCH_ZERO_COPY -- for a peer on the same device no bytes move: the average reads the
 * peer's slot in place; DPWA_FETCH_PUBLISHED -- an IPC peer's snapshot whose publish is
 * already complete (the gossip board advertised it): the pull is not ordered after `stream`
 * and alternates between two staging buffers, waiting only for the average that last read
 * the one it fills.  Slot reuse is protected for local peers by events; for IPC peers by the
 * caller's lock-step barrier or the board's read marks. */
#define DPWA_FETCH_ZERO_COPY 1
#define DPWA_FETCH_PUBLISHED 2
/* DPWA_FETCH_RESCUE: the fetch re-selected after a timed-out pull (conn.py:304-309 reconnects and
 * picks again): it copies into a rescue lane -- a buffer and a stream of the greatest priority of
 * its own -- so the stalled pull ahead of it on the side stream cannot hold it up.  A lane whose
 * pull has not landed stays taken and the next re-selected pull takes another (lanes made at first
 * use, up to 8, see rescue_free); DPWA_ERR_STATE when no lane is free. */
#define DPWA_FETCH_RESCUE 4
int dpwa_learner_fetch(dpwa_learner *l, int peer_id, uint64_t peer_version, int flags,
                       dpwa_stream_t stream);
/* The fetch timeout of the device path (the reference's socket timeout, conn.py:249 with
 * timeout_ms from the YAML, and its handling at conn.py:304-309).  fetch_state polls the copying
 * fetch in flight without blocking: DPWA_FETCH_LANDED (landed, or nothing to wait for),
 * DPWA_FETCH_IN_FLIGHT, or DPWA_FETCH_TIMED_OUT (still in flight timeout_ms after the request went
 * out).  The reference's socket timeout bounds only the wait for the reply (conn.py:249), so a pull
 * ordered after the caller's stream (a local peer's snapshot) is timed from when that stream
 * reached update_send -- a device backlog the caller queued before update_send is not the peer's
 * delay: while the stream has not reached it the pull is in flight, after it the time since is read
 * on the device's clock (an event on a probe stream of its own, timestamps compared); a backlog of
 * over 60 s, or a probe that cannot run, falls back to the host's issue time.  Board pulls wait
 * for nothing of the caller's and are timed from the issue.  Judged pulls are LocalGroup copying
 * pulls and board pulls.  rescue_free: *free_out = 1 when a rescue lane is free (its pull landed) or one
 * could be made now (it is made here: up to 8 lanes, each one snapshot, while 1 GiB stays free on
 * the device; a failed allocation caps the count where it is, *free_out = 0, no error).
 * rescue_lanes: lanes made so far and the current cap; set_rescue_cap lowers (or raises, up to 8)
 * the cap -- not below the lanes already made.  fetch_stream: the stream the fetch in flight moves
 * its bytes on (side stream or a rescue lane's). */
#define DPWA_FETCH_LANDED 0
#define DPWA_FETCH_IN_FLIGHT 1
#define DPWA_FETCH_TIMED_OUT 2
int dpwa_learner_fetch_state(dpwa_learner *l, int64_t timeout_ms, int *state);
int dpwa_learner_rescue_free(dpwa_learner *l, int *free_out);
int dpwa_learner_rescue_lanes(dpwa_learner *l, int *lanes, int *cap);
int dpwa_learner_set_rescue_cap(dpwa_learner *l, int cap);
int dpwa_learner_fetch_stream(dpwa_learner *l, dpwa_stream_t *stream);

/* update_wait's averaging (dpwa.py:133-155 + pytorch.py:64-68) as ONE kernel: make `stream`
 * wait for the fetch, then every workgroup evaluates the factor (fp64, from the device clock
 * and the peer's header) while its loads are in flight and lerps its part of the n-element
 * flat buffer in place; workgroup 0 writes the new clock and the dpwa_coef. */
int dpwa_learner_average(dpwa_learner *l, void *flat, double loss, const double *loss_dev,
                         dpwa_stream_t stream);

/* Write-through form: the averaged parameters are also stored into the slot of the NEXT
 * publish (4*n*s bytes instead of 3*n*s here, and that publish then moves no payload). */
int dpwa_learner_average_through(dpwa_learner *l, void *flat, double loss, const double *loss_dev,
                                 dpwa_stream_t stream);
/* The averages of `count` learners of one device (each with a fetch in flight) as few
 * dispatches as possible: every learner's dpwa_learner_average(_through) (write_through[i]),
 * same results and bookkeeping, but compatible ones (same dtype and form, 16-B aligned,
 * contiguous source) share one launch of up to 8.  loss_dev may be NULL (all host losses). */
int dpwa_learner_average_many(dpwa_learner *const *learners, void *const *flats, const double *loss,
                              const double *const *loss_dev, const int *write_through, int count,
                              dpwa_stream_t stream);
/* Distance tracking (dpwa_distance above; off by default, and off every launch is the untracked one).
 * set_distance(on != 0) allocates the workspace and the record once, here -- never inside a round --
 * and from then on every round of this learner that averages writes the record:
 *   single dtype, 16-B aligned, contiguous peer snapshot     the tracked kernel (no extra bytes), in the
 *     (average / average_through / resident)                 plain, write-through and resident forms
 *   DPWA_MIXED; unaligned parameters; the split              the stand-alone pass enqueued on the same
 *     factor -> lerp form; an average inside                 stream BEFORE the unchanged average (the
 *     dpwa_learner_average_many                              in-place forms overwrite what it reads):
 *                                                            2*n*s more bytes read per round
 *   the relay's fused second phase                           refused: dpwa_learner_relay_phase2 with
 *                                                            fuse != 0 on a tracking learner is
 *                                                            DPWA_ERR_STATE, and so is set_distance(on)
 *                                                            while a fused second phase is pending
 * A round that does not average leaves the record as it was.  dpwa_learner_distance: the record's
 * device address (borrowed, valid until dpwa_learner_destroy; DPWA_ERR_STATE before the first
 * set_distance(on)); read it in order with the stream that averaged. */
int dpwa_learner_set_distance(dpwa_learner *l, int on);
int dpwa_learner_distance(dpwa_learner *l, const dpwa_distance **dev);
/* The per-parameter distance of a learner (dpwa_param_range above; off by default, and off every launch
 * is the launch it was).  set_param_distance(ranges, count, every) checks the ranges against the
 * learner's n / dtype / layout (DPWA_ERR_ARG; a DPWA_MIXED learner needs its layout first:
 * DPWA_ERR_STATE), allocates the table, the workspace and the record once, here, and from then on the
 * every-th, 2*every-th, ... round of this learner that launches an average also runs the pass
 * (dpwa_measure_param_distance's) BEFORE that average on the same stream and the finishing step after
 * it, whatever the form: average / average_through / resident (it reads the published slot) /
 * DPWA_MIXED / the split factor -> lerp / an average inside dpwa_learner_average_many.  2*n*s more
 * bytes read on a measured round; other rounds launch nothing new and leave the record.  The
 * whole-model record (set_distance) is independent of it.  count = 0 switches it off (ranges may be
 * NULL); every >= 1.  The same two rules as set_distance hold for the relay's fused second phase.
 * While it is on, parameters that are not 16-byte aligned are refused by the average (DPWA_ERR_ARG,
 * nothing queued).  A round that does not average (the ZeroDivision no-op) leaves the record as it
 * was.  dpwa_learner_param_distance: the record's device address and its tensor count (borrowed, valid
 * until the next set_param_distance with count > 0 or dpwa_learner_destroy; DPWA_ERR_STATE before the
 * first). */
int dpwa_learner_set_param_distance(dpwa_learner *l, const dpwa_param_range *ranges, int64_t count, int every);
int dpwa_learner_param_distance(dpwa_learner *l, const dpwa_param_distance_head **dev, int64_t *count);
/* Host counters since the last set_param_distance with count > 0 (no device touched, no sync): the
 * rounds of this learner that launched an average, and those of them on which the pass and its
 * finishing step were launched.  A measured round that turned out a ZeroDivision no-op counts here
 * and writes no record: the record's `count` stays 0 until a round has written it. */
int dpwa_learner_param_distance_rounds(dpwa_learner *l, int64_t *averaged, int64_t *measured);
/* Skipping a round whose peer snapshot is not finite (off by default, and off every launch is the
 * launch it was and every result bit-equal).  A gossip network spreads a NaN or an inf as it spreads
 * everything else: a * q + b * p with a non-finite q is non-finite, and after O(log G) rounds so is
 * every replica.  With set_finite_check(on != 0) -- nothing is allocated, here or in a round -- every
 * round of this learner that would average first reads the fetched peer snapshot once more (n*s
 * bytes, one launch: dpwa_check_finite's pass) on the average's stream, behind the fetch and before
 * the average and any distance pass.  If an element of it is NaN or +-inf the round is the no-op
 * round of a ZeroDivision -- parameters untouched, a write-through or resident snapshot receives the
 * unchanged parameters, clock unchanged, the distance records left alone -- but it is no error:
 * dpwa_coef.status is DPWA_STATUS_PEER_NONFINITE, the sticky status word stays 0, and the round is
 * counted (finite_skips: the count since dpwa_learner_create; it waits for the device).  A ZeroDivision
 * round stays one, whatever the peer holds.  Where it runs: dpwa_learner_average / average_through
 * (resident and DPWA_MIXED included), once per checking learner before a dispatch of
 * dpwa_learner_average_many, and before the factor in dpwa_learner_factor, so that dpwa_learner_lerp
 * skips through the coefficients it reads anyway.  A caller that does the arithmetic itself after
 * dpwa_learner_factor gets factor 0, and 0 * NaN is NaN: use dpwa_learner_lerp.  The learner's own
 * parameters are not looked at: a replica that is itself non-finite is not healed, its peers stop
 * taking from it.  The pass of a split round is the factor's, so the snapshot it read must be the one the
 * lerp averages: on a checking learner dpwa_learner_fetch while a factor is computed and not yet consumed
 * is DPWA_ERR_STATE (nothing moves; lerp or cancel first), and so is set_finite_check(on) then; with the
 * check off a second fetch keeps the factor, as before.
 * The relay's fused second phase reads no contiguous snapshot: dpwa_learner_relay_phase2
 * with fuse != 0 on a checking learner is DPWA_ERR_STATE, and so is set_finite_check(on) while a fused
 * second phase is pending.  dpwa_node_set_finite_check: the same on a bound node's learner. */
int dpwa_learner_set_finite_check(dpwa_learner *l, int on);
int dpwa_learner_finite_skips(dpwa_learner *l, uint64_t *count);
/* The consensus of a group of learners (dpwa_consensus above) over the published snapshots of publish
 * number `version`: the slot (version - 1) % 2 of `l` and of the named attached peers, in the order
 * given; peer_id -1 stands for `l` itself.  Peers may be local learners of l's device or IPC / fd-mapped
 * ones.  out (NULL: measure only): the mean, device memory of the payload's bytes, 16-B aligned, no slot.
 * record_dev (NULL: the mean only): written whole, with `version`.  The accumulator rows belong to the
 * learner: allocated and zeroed by the first call that measures, never inside a later one.  Read-only: no
 * parameter, slot, clock, fetch or distance record of any learner changes, and a learner that never calls
 * it launches what it launched before.
 * Ordering: the launch follows the local members' publishes through their publish marks, and this learner
 * is registered as a reader of their slots exactly as a zero-copy fetch registers it, so the publish or
 * write-through average that rewrites a slot waits for the read.  Mapped members are not ordered here: in
 * a lock-step group the round's barrier has ordered every rank's publish `version`, and a launch on the
 * round's stream precedes the barrier in front of any rank's publish version + 2, which is what rewrites
 * the slot; the pass is preceded by a system-scope acquire.
 * DPWA_ERR_ARG: a count outside 1..DPWA_CONSENSUS_MAX, an unknown peer, a peer whose n, dtype or layout
 * digest differs, a local peer on another device, the same slot named twice (a self-peer and -1), neither
 * out nor a record, out misaligned or overlapping a member's slot.  DPWA_ERR_STATE: `l` or a local peer
 * whose current version is not `version`, version 0, a DPWA_MIXED learner without its layout, a learner
 * with a fused relay phase pending (no contiguous snapshot exists). */
int dpwa_learner_consensus(dpwa_learner *l, const int32_t *peer_ids, int count, uint64_t version, void *out,
                           dpwa_consensus_record *record_dev, dpwa_stream_t stream);

/* always != 0: a write-through average never writes the next publish's header ahead; that
 * publish then writes it with the loss given to it (a snapshot served over the wire bridge
 * carries the reference's {'clock', 'loss'} state, conn.py:110). */
int dpwa_learner_set_header_publish(dpwa_learner *l, int always);
/* Publish that reuses a write-through snapshot when the last average wrote `flat` through
 * (the caller asserts `flat` is unchanged since): header only; otherwise a full publish. */
int dpwa_learner_publish_reuse(dpwa_learner *l, const void *flat, double loss, const double *loss_dev,
                               dpwa_stream_t stream);
/* on != 0: a reusing publish (above) first compares 4096 16-B words spread over `flat` with
 * the written-through snapshot on the device, and copies the payload from `flat` when any
 * differs -- a write the caller's bookkeeping missed (pytorch.py:49-53 then holds anyway: the
 * snapshot is the parameters at update_send).  Two small launches, no host sync.
 * reuse_guard_hits: how many publishes found a difference (synchronises the device).
 * On a resident learner (below) the same flag is the window guard: every publish runs one small
 * kernel that compares the payload published last time with those words saved when it was
 * published -- a write while peers could read it (update_send .. update_wait, through
 * `param.data`, which the adapter's version counters miss) -- and saves the new payload's.  A
 * written window is reported by the first publish that finds it counted (never waiting for a
 * check): DPWA_ERR_STATE, nothing published; the publish after proceeds.  window_hits: windows
 * found written so far, checking the last one now (synchronises its stream). */
int dpwa_learner_set_reuse_guard(dpwa_learner *l, int on);
int dpwa_learner_reuse_guard_hits(dpwa_learner *l, uint32_t *hits);
int dpwa_learner_window_hits(dpwa_learner *l, uint32_t *hits);

/* Resident parameters (extension; replaces the snapshot copy of pytorch.py:49-53 and
 * RxThread.set_current_state, conn.py:73-79, with no copy at all).  The learner's parameters live
 * in its own two snapshot slots and move between them: a publish writes only the header of the
 * slot they are in, and the average reads them there -- the published snapshot, which it leaves
 * untouched -- and stores the result into the other slot, the slot of the next publish.  A round
 * then moves 3*n*s bytes, the averaging's own (write-through: 4*n*s; publish + in-place average:
 * 5*n*s), with the same results.
 *   set_resident      before the first publish: copy `init` (n elements) into slot 0.
 *   resident_params   where the parameters are now (*params NULL and *slot -1 when not resident):
 *                     a device pointer valid for the learner's life, which changes at every
 *                     average -- re-read it after each one.
 *   relocate          a round without an average: the parameters leave the published slot by one
 *                     copy into the next publish's slot (no-op when they are there).
 * Contract: the parameters ARE the served snapshot between a publish and the next average or
 * relocate, so they must not be written in that window.  The reference's own loop DOES write
 * there (README.md:18-29, examples/pytorch-cifar/main.py:130-145: update_send, the training
 * step, update_wait) and must use the write-through or full form; a resident learner needs the
 * reordered loop update_send, update_wait, step (the same gossip with each step applied after
 * the round's average instead of before it).  The Python layer records the parameters' version
 * counters at update_send and raises at update_wait when any moved (DpwaConnection,
 * DpwaPyTorchAdapter).  A publish is given the resident pointer; the split factor/lerp form is
 * refused. */
int dpwa_learner_set_resident(dpwa_learner *l, const void *init, dpwa_stream_t stream);
int dpwa_learner_resident_params(dpwa_learner *l, void **params, int *slot);
int dpwa_learner_relocate(dpwa_learner *l, dpwa_stream_t stream);

/* Split form of dpwa_learner_average for the DpwaConnection / adapter seam:
 * factor only (update_wait's return value), then lerp with the learner's coefficients.
 * A factor computed while a write-through average's snapshot still awaits its publish moves the clock
 * that the header written ahead was made from: the reusing publish then writes the header anew from the
 * live clock (one small kernel), as after dpwa_learner_write_clock. */
int dpwa_learner_factor(dpwa_learner *l, double loss, const double *loss_dev, dpwa_stream_t stream);
int dpwa_learner_lerp(dpwa_learner *l, void *flat, dpwa_stream_t stream);

/* Wire bridge.  read_snapshot: synchronous copy of the latest published
 * snapshot to host memory (header 256 B + up to payload_bytes), from any host thread --
 * RxThread's reply (conn.py:108-110); *version_out = 0 when nothing was published.
 * fetch_host: stage a snapshot received in host memory (a reference node's reply,
 * conn.py:298) as the fetch to average with; payload_bytes must equal n*sizeof(dtype).  The
 * copy waits only for the last reader of the staging buffer (not for `stream`'s queued work);
 * the host buffer may be reused on return (a page-locked one is DMA'd, and waited for). */
int dpwa_learner_read_snapshot(dpwa_learner *l, void *header_out, void *payload_out, int64_t payload_bytes,
                               uint64_t *version_out);
int dpwa_learner_fetch_host(dpwa_learner *l, const void *header, const void *payload, int64_t payload_bytes,
                            dpwa_stream_t stream);

/* Relay transport: a lock-step round's pulls spread over every xGMI link.  Each snapshot is
 * cut into `world` stripes; phase 1 (after the caller's collective that shares every rank's
 * pick, so that all publishes of the round are complete) pulls stripe `rank` of every
 * snapshot some rank needs into this rank's relay buffer; phase 2 (after a second
 * barrier) gathers this rank's peer's stripes from all ranks into staging and makes it the
 * fetch in flight (my_pick = rank averaged with, -1 none).  Both phases run on the learner's
 * side stream; picks_dev holds `world` int32 on this learner's device.
 * relay_wait makes `stream` wait for the previous round's relay work (call before the next
 * round's collective, so a slot or relay buffer is rewritten only after every reader).
 * phase2 with fuse != 0 gathers nothing yet: the next dpwa_learner_average(_through) reads the
 * peer's stripes where phase 1 left them (one kernel instead of the gather + the average; the
 * average's stream then carries the round's last reads of other ranks' relay buffers); any
 * other use of the fetch (the split factor/lerp, copy_fetched, wait_fetch) gathers first. */
int dpwa_learner_relay_enable(dpwa_learner *l, int world, int rank);
int dpwa_learner_relay_handle(dpwa_learner *l, void *handle_out, int64_t handle_len);
int dpwa_learner_relay_attach(dpwa_learner *l, int rank, int peer_id, const void *relay_handle,
                              int64_t handle_len);
int dpwa_learner_relay_attach_fds(dpwa_learner *l, int rank, int peer_id, const void *relay_handle,
                                  int64_t handle_len, const int *fds, int n_fds, int64_t chunk_bytes);
int dpwa_learner_relay_wait(dpwa_learner *l, dpwa_stream_t stream);
int dpwa_learner_relay_phase1(dpwa_learner *l, const int32_t *picks_dev, uint64_t version, int blocks,
                              dpwa_stream_t stream);
int dpwa_learner_relay_phase2(dpwa_learner *l, const int32_t *picks_dev, int my_pick, uint64_t version,
                              int blocks, int fuse);
/* Kernel timing for measurement.  time_averages allocates `capacity` begin/end event pairs
 * (0 frees them; synchronises the device).  After arm_timing, the next averaging launch
 * (average / average_through, 16-B aligned parameters) goes through hipExtLaunchKernelGGL
 * with the next free pair, so it is timed as a profiler times it, without the dispatch gaps
 * of an event pair recorded around the launch; the next publish disarms it (a round without an
 * average times nothing).  A batched dispatch (average_many) is timed with the pair of its first
 * armed learner, in call order.  read_average_times waits for and returns the recorded
 * durations (µs, launch order) and frees the pairs for reuse. */
int dpwa_learner_time_averages(dpwa_learner *l, int capacity);
int dpwa_learner_arm_timing(dpwa_learner *l);
int dpwa_learner_read_average_times(dpwa_learner *l, float *us_out, int max, int *count);
/* Bench: time the next `capacity` copying fetches (pull start to landed, on the side
 * stream; the relay is not timed) and read them back in order, in microseconds. */
int dpwa_learner_time_fetches(dpwa_learner *l, int capacity);
int dpwa_learner_read_fetch_times(dpwa_learner *l, float *us_out, int max, int *count);
/* The learner's side stream (fetches and relay phases run on it). */
int dpwa_learner_side_stream(dpwa_learner *l, dpwa_stream_t *stream);

/* Makes `stream` wait for the pull of the fetch in flight, if it copies (TxThread.fetch_wait,
 * conn.py:326-329); average/factor do this themselves -- this only lets a caller order the
 * wait before its own timing event. */
int dpwa_learner_wait_fetch(dpwa_learner *l, dpwa_stream_t stream);

/* How a copying fetch (any non-zero-copy fetch) moves its bytes: DPWA_PULL_COPY_ENGINE
 * (hipMemcpyAsync on the side stream, the default) or DPWA_PULL_KERNEL (a copy kernel of at
 * most max_blocks workgroups reading the IPC-mapped peer slot over xGMI). */
/* What a device loss pointer (`loss_dev` of publish / factor / average) points at: a float64
 * (DPWA_F64, the default) or a float32 (DPWA_F32: e.g. a training loss tensor passed as is,
 * widened exactly on the device as Python's float() widens it). */
int dpwa_learner_set_loss_dtype(dpwa_learner *l, int32_t dtype);

#define DPWA_PULL_COPY_ENGINE 0
#define DPWA_PULL_KERNEL 1
int dpwa_learner_set_pull(dpwa_learner *l, int mode, int max_blocks);

/* Reference-style seam (dpwa.py:156 returns (payload, factor) and pytorch.py:68 does the
 * arithmetic itself): copy_factor enqueues a copy of the last factor (float64) to dst_dev on
 * `stream`; copy_fetched enqueues, after the pull has landed, a copy of the payload of the fetch
 * in flight (between update_wait and the lerp) to dst_dev (n elements). */
int dpwa_learner_copy_factor(dpwa_learner *l, double *dst_dev, dpwa_stream_t stream);
int dpwa_learner_copy_fetched(dpwa_learner *l, void *dst_dev, dpwa_stream_t stream);

/* Abandons a fetch whose factor was computed but whose lerp will never be issued (the
 * caller of update_wait chose not to average); the snapshot it read may then be reused. */
int dpwa_learner_cancel(dpwa_learner *l);

/* Device pointers of the learner's blocks.  The clock is double-buffered: *clock_dev is the
 * live one and stays valid until the next factor/average.  status_word: the pinned host
 * word behind dpwa_learner_poll_status (host address), for callers that poll it directly. */
int dpwa_learner_status_word(dpwa_learner *l, int32_t **status_word);
int dpwa_learner_pointers(dpwa_learner *l, double **clock_dev, dpwa_coef **coef_dev,
                          dpwa_header **staging_header_dev, void **staging_payload_dev);
/* Synchronous reads for inspection (these DO synchronise with the learner's device). */
int dpwa_learner_read_clock(dpwa_learner *l, double *clock);
int dpwa_learner_write_clock(dpwa_learner *l, double clock);
int dpwa_learner_read_coef(dpwa_learner *l, dpwa_coef *coef);
/* Non-blocking status check: *done = 1 when the last factor computation has completed;
 * *status = the first non-OK DPWA_STATUS_* any factor computation reported since the last
 * poll (a sticky pinned host word, cleared by this call), else DPWA_STATUS_OK. */
int dpwa_learner_poll_status(dpwa_learner *l, int *done, int32_t *status);

/* ------------------------------------------------------------------------------------
 * Host scheduler: TxThread's peer choice and flow control (conn.py:178-317) plus the
 * Bernoulli fetch gate (dpwa.py:101-102), over a CPython-exact MT19937 so that a learner
 * seeded like `random.seed(seed)` draws the reference's exact sequence.
 * ------------------------------------------------------------------------------------ */
typedef struct dpwa_sched dpwa_sched;

/* outcomes reported back for a picked peer (conn.py:245-313) */
#define DPWA_CONNECT_OK 0        /* lazy connect succeeded                       conn.py:247-251 */
#define DPWA_CONNECT_REFUSED 1   /* ConnectionRefusedError: score -= 100, round ends  conn.py:253-256 */
#define DPWA_CONNECT_ERROR 2     /* other error: peer removed, round ends        conn.py:257-260 */
#define DPWA_REPLY_PAYLOAD 3     /* reply with data: score += 10, round ends      conn.py:301-302 */
#define DPWA_REPLY_EMPTY 4       /* peer had no state: score += 10, pick again    conn.py:301-302 */
#define DPWA_REPLY_TIMEOUT 5     /* socket.timeout: score -= 100, reconnect, again conn.py:304-309 */
#define DPWA_REPLY_ERROR 6       /* other error: peer removed, pick again         conn.py:311-313 */

/* static peer status for dpwa_sched_fetch (what the transport knows about each peer) */
#define DPWA_PEER_READY 0        /* up and has published                          */
#define DPWA_PEER_NO_STATE 1     /* up, nothing published yet -> empty reply       */
#define DPWA_PEER_DOWN 2         /* not up: refused when not connected, error if it was */
#define DPWA_PEER_SLOW 3         /* times out                                     */
#define DPWA_PEER_DEAD 4         /* unrecoverable: removed                        */

/* seed_key: 32-bit little-endian words of abs(seed) as CPython's random.seed(int) splits
 * it (key_len 0 means seed 0); key_len < 0 seeds from OS entropy (random.seed(None)). */
int dpwa_sched_create(dpwa_sched **out, int n_peers, const uint32_t *seed_key, int key_len,
                      double fetch_probability);
int dpwa_sched_destroy(dpwa_sched *s);
/* dpwa.py:101-102 / 118: *fetching = random() < fetch_probability */
int dpwa_sched_bernoulli(dpwa_sched *s, int *fetching);
/* conn.py:224-240: score each live peer + randint(10,1000) in insertion order, argmax,
 * tie-break randint(0, k-1).  *peer = -1 when no peers remain. *connected tells whether
 * the caller must report a CONNECT_* outcome before the REPLY_* one. */
int dpwa_sched_pick(dpwa_sched *s, int *peer, int *connected);
/* Applies an outcome for the picked peer; *round_done / *got_data say how the fetch loop
 * (conn.py:286-313) continues. */
int dpwa_sched_report(dpwa_sched *s, int peer, int outcome, int *round_done, int *got_data);
/* The whole fetch loop for one queue item (conn.py:277-315) against a static per-peer
 * status array; stops after max_attempts picks (the reference would spin forever when
 * every peer times out).  *peer_out = the peer that delivered data, or -1. */
int dpwa_sched_fetch(dpwa_sched *s, const int32_t *peer_status, int max_attempts, int *peer_out,
                     int *attempts_out);
/* flow_control_score of a peer (conn.py:190); -1 once removed */
int dpwa_sched_score(const dpwa_sched *s, int peer, int *score);
/* DpwaConnection.remove_peer (dpwa.py:98-99 -> conn.py:215-222): drop a peer for good. */
int dpwa_sched_remove(dpwa_sched *s, int peer);
/* DpwaConnection.add_peer (dpwa.py:95-96 -> conn.py:208-213): a fresh record for the peer
 * (score 1000, not connected); a removed peer is inserted again at the end of the pick order. */
int dpwa_sched_add(dpwa_sched *s, int peer);
int dpwa_sched_n_live(const dpwa_sched *s, int *n_live);
/* raw CPython-equivalent draws, for tests: random.random(), random.randint(a, b) */
/* Gossip-state checkpoint (SURVEY §5 checkpoint/resume; the reference keeps none across a
 * restart, dpwa.py:59): the scheduler's generator (CPython getstate() order), every peer's
 * flow-control score and connected/live flags, and TxThread's peer order, as 32-bit words.
 * get_state with words == NULL returns the size in *n_words; set_state validates the whole state
 * (format, peer count, score bounds, order) before changing anything.  ABI version 9. */
int dpwa_sched_get_state(const dpwa_sched *s, uint32_t *words, int max_words, int *n_words);
int dpwa_sched_set_state(dpwa_sched *s, const uint32_t *words, int n_words);
int dpwa_sched_random(dpwa_sched *s, double *out);
int dpwa_sched_randint(dpwa_sched *s, int64_t a, int64_t b, int64_t *out);

/* ------------------------------------------------------------------------------------
 * Node: DpwaConnection's per-round logic (dpwa/dpwa.py:54-156) in native code -- the
 * scheduler, the learner (bound at the first publish) and a peer table.  One call per
 * half-round keeps the host cost of a gossip round to a few microseconds.
 * ------------------------------------------------------------------------------------ */
typedef struct dpwa_node dpwa_node;

#define DPWA_NODE_PEER_UNSET 0    /* not reachable: a fetch is refused (conn.py:253-256)      */
#define DPWA_NODE_PEER_LOCAL 1    /* another node of this process (any device)                */
#define DPWA_NODE_PEER_REMOTE 2   /* IPC-attached learner of another process, lock-step rounds */

/* flags of the node calls */
#define DPWA_FLAG_EAGER 1            /* update_send/gate: start a granted fetch now (DistGroup)    */
#define DPWA_FLAG_ZERO_COPY 2        /* read a same-device local peer's slot in place              */
#define DPWA_FLAG_REUSE_SNAPSHOT 4   /* publish: flat unchanged since a write-through average      */
#define DPWA_FLAG_WRITE_THROUGH 8    /* update_wait_average: also write the next snapshot          */
#define DPWA_FLAG_PICK_ONLY 16       /* gate (EAGER): pick the peer, the caller moves the bytes    */

/* DpwaConnection.__init__ (dpwa.py:54-93) minus the model: scheduler seeded as
 * dpwa_sched_create, the interpolation config for the learner bound later. */
int dpwa_node_create(dpwa_node **out, int n_peers, const uint32_t *seed_key, int key_len,
                     double fetch_probability, const dpwa_interp *cfg);
int dpwa_node_destroy(dpwa_node *n);
/* Creates the node's learner for an n-element flat buffer of `dtype` on `device`. */
int dpwa_node_bind(dpwa_node *n, int device, int64_t numel, int32_t dtype);
/* dpwa_learner_set_layout for the node's learner (bound as DPWA_MIXED), before its peers attach. */
int dpwa_node_set_layout(dpwa_node *n, const dpwa_layout *layout);
/* Borrowed handles of the node's learner (NULL before bind) and scheduler. */
int dpwa_node_handles(dpwa_node *n, dpwa_learner **learner, dpwa_sched **sched);
/* How peer `peer` (scheduler index) is reached: DPWA_NODE_PEER_*; `local` for LOCAL (may be n
 * itself: a node entry at this node's own host:port, whose RxThread the reference dials like any
 * peer's -- the self-peer of configs[1]). */
int dpwa_node_set_peer(dpwa_node *n, int peer, int kind, dpwa_node *local);
/* Fault injection: force a DPWA_PEER_* status for a peer, -1 clears. */
int dpwa_node_set_fault(dpwa_node *n, int peer, int status);
/* Free-running rounds (extension of DPWA_NODE_PEER_REMOTE): the node's REMOTE peers are
 * read through `board` (see below) instead of lock-step.  peer_ranks[k] = board rank of
 * scheduler peer k; publish_timeout_ms bounds a publish's wait for readers (-1 forever).
 * board NULL returns the node to lock-step.  The node does not own the board. */
typedef struct dpwa_board dpwa_board;
int dpwa_node_set_board(dpwa_node *n, dpwa_board *board, const int32_t *peer_ranks, int publish_timeout_ms);
/* The YAML's timeout_ms (DpwaConfiguration.get_timeoutms, dpwa.py:90 -> conn.py:249) on the
 * device path (< 0 disables).  A copying pull from a local peer or through the gossip board is
 * judged when update_wait polls it (never a host wait in the normal path): landed, or out less
 * than timeout_ms (dpwa_learner_fetch_state) -> the reply with data (score +10, conn.py:301-302;
 * a pull still in flight is then waited for on the device); still in flight after timeout_ms -> a
 * socket timeout (score -100, reconnect, conn.py:304-309) and the loop picks again, the
 * re-selected pull going to a rescue lane (DPWA_FETCH_RESCUE) and being polled on the host up to
 * timeout_ms like the reference's blocking receive; a rescue pull that times out too is followed
 * by the next pick on another lane, until data, no peer or every peer removed, as TxThread
 * (conn.py:286-313).  With every lane (up to 8) still pulling, the next request waits for one to
 * land before it goes out; only a learner whose own transport stays stuck for
 * $DPWA_RESCUE_WAIT_MS (default 60000) gives that request up as a timeout and ends the round
 * without data.  Lock-step (DistGroup) pulls wait for the round's barrier, i.e. for the slowest
 * learner, not for the peer, and are not judged. */
int dpwa_node_set_timeout(dpwa_node *n, int timeout_ms);

/* update_send (dpwa.py:104-123): publish, then the Bernoulli gate; with DPWA_FLAG_EAGER a
 * granted fetch starts now (peer choice + pull on the side stream), else at update_wait.
 * Split form: publish, then (after a caller-side barrier) gate. */
int dpwa_node_update_send(dpwa_node *n, const void *flat, double loss, const double *loss_dev, int flags,
                          dpwa_stream_t stream, int *fetching);
int dpwa_node_publish(dpwa_node *n, const void *flat, double loss, const double *loss_dev, int flags,
                      dpwa_stream_t stream);
int dpwa_node_gate(dpwa_node *n, int flags, dpwa_stream_t stream, int *fetching);
/* Starts the fetch a non-eager gate granted (TxThread.run, conn.py:277-315), now instead of at
 * update_wait: a group of co-resident learners calls it once every learner of the round has
 * published, so the pull overlaps the training step (no-op when nothing is pending). */
int dpwa_node_start_fetch(dpwa_node *n, int flags, dpwa_stream_t stream);
/* update_wait (dpwa.py:125-156): *peer = the peer averaged with, or -1 for (None, 0).
 * _average fuses the adapter's lerp (pytorch.py:66-68) into the same kernel; the split
 * form computes the factor only and dpwa_node_lerp applies it. */
int dpwa_node_update_wait(dpwa_node *n, double loss, const double *loss_dev, int flags,
                          dpwa_stream_t stream, int *peer);
int dpwa_node_lerp(dpwa_node *n, void *flat, dpwa_stream_t stream);
int dpwa_node_update_wait_average(dpwa_node *n, void *flat, double loss, const double *loss_dev,
                                  int flags, dpwa_stream_t stream, int *peer);
/* update_wait_average of `count` nodes of this process whose learners share a device, in node
 * order (each node's fetch is resolved in turn, as `count` calls would), with their averages
 * enqueued as one batched dispatch (dpwa_learner_average_many).  peers[i] as *peer above. */
int dpwa_node_update_wait_average_many(dpwa_node *const *nodes, void *const *flats, const double *loss,
                                       const double *const *loss_dev, int count, int flags,
                                       dpwa_stream_t stream, int *peers);
/* Resident parameters for the node's learner (dpwa_learner_set_resident; bound, before the first
 * publish).  A resident node's update_wait_average always averages in the resident form (flat =
 * dpwa_learner_resident_params before the call) and relocates the parameters in a round without
 * an average; its split update_wait is refused. */
int dpwa_node_set_resident(dpwa_node *n, const void *init, dpwa_stream_t stream);
/* dpwa_learner_set_finite_check on the node's learner (DPWA_ERR_STATE before dpwa_node_bind).  The
 * scheduler is not told of a skipped round: the fetch outcome was reported before the device looked. */
int dpwa_node_set_finite_check(dpwa_node *n, int on);
/* State of the current/last round: fetching flag, fetched peer (-1: none), its publish
 * number, and the picks the last fetch took. */
int dpwa_node_info(const dpwa_node *n, int *fetching, int *fetch_peer, uint64_t *fetch_version,
                   int *last_attempts);

/* ------------------------------------------------------------------------------------
 * Gossip board: free-running rounds across the processes of one node (extension).
 * Replaces the reference's always-on RxThread server (conn.py:51-172) and its publish Lock
 * (conn.py:76-79, 109-110) with a POSIX shared-memory block: the newest complete publish
 * of every rank (written by its stream after the publish), per (publisher, reader) the
 * version being pulled, and liveness (a closed entry or a dead pid is a refused
 * connection, conn.py:253-256).  No collective runs per round.
 * ------------------------------------------------------------------------------------ */
/* name: "/..." (shm_open); create != 0 on exactly one rank, before the others open. */
int dpwa_board_open(dpwa_board **out, const char *name, int world, int rank, int create);
int dpwa_board_unlink(const char *name);
/* marks this rank closed (peers see a refused connection) and unmaps */
int dpwa_board_close(dpwa_board *b);
/* hipHostRegister the block for stream writes from `device` (needed before a device
 * advertise/release) */
int dpwa_board_register(dpwa_board *b, int device);
/* DPWA_PEER_DOWN / NO_STATE / READY for rank r */
int dpwa_board_status(dpwa_board *b, int r, int32_t *status);
/* raw view of rank r: its newest complete publish, our read mark on it, liveness */
int dpwa_board_read(dpwa_board *b, int r, uint64_t *version, uint64_t *reading_by_me, int32_t *alive);
/* reader: a version of r that r will not overwrite until released (0 = never published) */
int dpwa_board_acquire(dpwa_board *b, int r, uint64_t *version);
/* reader: clear the read mark on r after the work on `stream` (host != 0: now) */
int dpwa_board_release(dpwa_board *b, int r, dpwa_stream_t stream, int host);
/* publisher: wait until publish `next` may rewrite its slot (timeout_ms < 0: forever) */
int dpwa_board_publish_wait(dpwa_board *b, uint64_t next, int timeout_ms);
/* publisher: announce publish `version` after the work on `stream` (host != 0: now) */
int dpwa_board_advertise(dpwa_board *b, uint64_t version, dpwa_stream_t stream, int host);

#ifdef __cplusplus
}
#endif

#endif /* DPWA_HIP_H */
