// kernels.hip -- CDNA4 (gfx950) kernels of the pairwise-averaging hot path.
//
//  * lerp:    the averaging statement of dpwa/adapters/pytorch.py:68,
//             param = f32(f32(a*peer) + f32(b*param)), as ONE streaming pass over the flat
//             parameter buffer (the reference runs three ATen kernels and allocates three
//             temporaries per tensor).  Pure HBM streaming (0.25 flop/byte): no LDS
//             staging, no MFMA.  Shape chosen by measurement (tools/lerp_tune.hip): one
//             16-byte item per lane and an exact grid -- many short-lived one-wave
//             workgroups keep the most loads in flight per CU (tools/block_sweep.sh);
//             grid-stride loops with more items per lane or a capped grid were 5-20%
//             slower on gfx950.
//             Separate roundings are required for bit parity with the reference (an FMA
//             changes up to ~30% of results near cancellation), so contraction is
//             switched off for this whole file.
//  * fused average: the same pass with the factor of dpwa/dpwa.py:139-155 computed in
//             the kernel: every workgroup evaluates it in fp64 while its loads are in flight
//             (one-wave workgroups keep the uniform (a, b) in registers; wider ones have wave 0
//             share them through LDS); block 0
//             also writes the new clock (into the other half of a double-buffered clock,
//             so no workgroup ever reads a clock another one is writing) and dpwa_coef.
//  * mixed:   the same pass over the segmented payload of a model that mixes float32, bfloat16
//             and float16 parameters (k_lerp_mixed): each one-wave span rounds as its segment's type.
//  * distance: opt-in -- the round's distance to the peer, sum (q - p)^2 and sum p^2 in fp64, formed
//             by a tracked form of the fused average from the operands it holds anyway
//             (k_lerp_tracked), or by a stand-alone pass (k_distance*), added across workgroups with
//             the hardware fp64 add and finished by k_distance_finish.
//             Opt-in too: the same sums for every parameter tensor over its own elements, by a
//             stand-alone pass that looks each span's tensors up in a device table
//             (k_param_distance) and one finishing workgroup per tensor (k_param_distance_finish).
//  * non-finite peer check: opt-in -- one read of the fetched peer snapshot before the average
//             (k_peer_finite*), a test on the exponent bits; a lane that finds a NaN or an inf
//             stores the round's stamp into the learner's veto word, and the factor of a round
//             whose stamp it finds there is the no-op's, with a status of its own.
//  * factor:  the same fp64 math as a one-thread kernel for the split API.
//  * publish: update_send's snapshot (dpwa.py:111-116, pytorch.py:49-53) -- clock += 1 on
//             the device and one copy of the flat buffer into a snapshot slot behind its
//             header.
//  * launches: the host half picks a kernel instantiation through with_ops (dtype) and Choice
//             (workgroup size, cache policy -- "the policy table" says what each averaging form
//             launches for a requested policy: the one policy.hpp chooses from the bytes of the
//             launch, or DPWA_LERP_POLICY's) and starts it with launch().
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "kernels.hpp"
#include "policy.hpp"

#include <hip/hip_ext.h>

namespace dpwa {

constexpr int kBlock = 256;   // 4 waves of 64

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));

static inline int64_t blocks_for(int64_t items)
{
    int64_t g = (items + kBlock - 1) / kBlock;
    return g < 1 ? 1 : g;
}

// ---------------------------------------------------------------- host helpers
// One launch.  With `timing` the dispatch itself is timed (the kernel's begin/end, as a profiler
// sees it).  The arguments are converted to the kernel's parameter types.
template <class... Params, class... Args>
static hipError_t launch(void (*kernel)(Params...), dim3 grid, dim3 block, hipStream_t s, const LaunchTiming *timing,
                         const Args &...args)
{
    if (timing)
        hipExtLaunchKernelGGL(kernel, grid, block, 0, s, timing->start, timing->stop, 0, (Params)args...);
    else
        hipLaunchKernelGGL(kernel, grid, block, 0, s, (Params)args...);
    return hipGetLastError();
}

// A run-time integer as a template argument: with(v, f) calls f(std::integral_constant<int, V>{})
// for the listed V equal to v, or for FALLBACK.  Only the listed values and FALLBACK are
// instantiated.
template <int FALLBACK, int... Vs> struct Choice {
    static constexpr int launched(int v) { return ((v == Vs) || ...) ? v : FALLBACK; }
    template <class F> static hipError_t with(int v, F &&f)
    {
        hipError_t r = hipSuccess;
        const bool listed = ((v == Vs && (r = f(std::integral_constant<int, Vs>{}), true)) || ...);
        return listed ? r : f(std::integral_constant<int, FALLBACK>{});
    }
};

// A tuning knob: environment variable `name`, where parse(text) is its value, or kNoValue for a
// text that is not accepted; unset or not accepted, the knob is `dflt`.  Every knob reads its
// variable once (a static at its call site).
constexpr int kNoValue = INT_MIN;

template <class Parse> static int env_knob(const char *name, int dflt, Parse parse)
{
    const char *e = getenv(name);
    const int v = e ? parse(e) : kNoValue;
    return v == kNoValue ? dflt : v;
}

static int one_of(int v, std::initializer_list<int> accepted)
{
    return std::find(accepted.begin(), accepted.end(), v) != accepted.end() ? v : kNoValue;
}

// ---------------------------------------------------------------- element ops
__device__ __forceinline__ float lerp1(float a, float b, float peer, float param)
{
    float x = a * peer;     // f32(a*t)          pytorch.py:68 `factor * t`
    float y = b * param;    // f32(b*p)          pytorch.py:68 `(1 - factor) * param.data`
    return x + y;           // f32(x + y)        contraction is off for this file
}

__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// Two f32 -> packed bf16, round-to-nearest-even (v_cvt_pk_bf16_f32 on gfx950).
__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi)
{
    float2v v = {lo, hi};
    bf16x2v r = __builtin_convertvector(v, bf16x2v);
    return __builtin_bit_cast(uint32_t, r);
}

// bf16(bf16(a*q) + bf16(b*p)) for the two bf16 held in each 32-bit word (torch-eager form).
__device__ __forceinline__ uint32_t lerp_bf16x2(float a, float b, uint32_t q, uint32_t p)
{
    uint32_t x = pk_bf16(a * bf_lo(q), a * bf_hi(q));
    uint32_t y = pk_bf16(b * bf_lo(p), b * bf_hi(p));
    return pk_bf16(bf_lo(x) + bf_lo(y), bf_hi(x) + bf_hi(y));
}

// Two f32 -> packed f16, round-to-nearest-even (v_cvt_pk_f16_f32; never the pkrtz form, which
// rounds toward zero).  fp16 subnormals are kept: the kernels run with the default
// float_denorm_mode_16_64 = 3 and no flush-to-zero build flag.
__device__ __forceinline__ uint32_t pk_f16(float lo, float hi)
{
    float2v v = {lo, hi};
    f16x2v r = __builtin_convertvector(v, f16x2v);
    return __builtin_bit_cast(uint32_t, r);
}

__device__ __forceinline__ float2v unpk_f16(uint32_t w)
{
    return __builtin_convertvector(__builtin_bit_cast(f16x2v, w), float2v);
}

// f16(f16(a*q) + f16(b*p)) for the two fp16 held in each 32-bit word (torch-eager form on
// torch.float16: each product is an fp32 product rounded to fp16, then the fp16 sum).  The fp32
// sum of two fp16 values is exact, so rounding it once to fp16 is the fp16 addition.
__device__ __forceinline__ uint32_t lerp_f16x2(float a, float b, uint32_t q, uint32_t p)
{
    const float2v qf = unpk_f16(q), pf = unpk_f16(p);
    const float2v x = unpk_f16(pk_f16(a * qf.x, a * qf.y));
    const float2v y = unpk_f16(pk_f16(b * pf.x, b * pf.y));
    return pk_f16(x.x + y.x, x.y + y.y);
}

// One element, for the ragged tail and the unaligned kernel.  Left alone, the compiler selects
// f16(a * f32(q)) as v_fma_mixlo_f16 with a +0.0 addend, and (-0.0) + (+0.0) is +0.0 where torch
// keeps the product's -0.0 (0.0 * q for a negative q, or q = -0.0); the empty asm keeps the fp32
// product a value of its own, so it is rounded by v_cvt_f16_f32 as in the packed form.
__device__ __forceinline__ uint16_t lerp_f16x1(float a, float b, uint16_t q, uint16_t p)
{
    float x = a * (float)__builtin_bit_cast(_Float16, q);
    float y = b * (float)__builtin_bit_cast(_Float16, p);
    asm("" : "+v"(x));
    asm("" : "+v"(y));
    const _Float16 xh = (_Float16)x, yh = (_Float16)y;
    return __builtin_bit_cast(uint16_t, (_Float16)((float)xh + (float)yh));
}

struct OpsF32 {
    using V = f32x4;
    using S = float;
    static constexpr int PER = 4;
    static constexpr bool TAIL = true;   // n counts elements; those past the last whole V are the ragged tail
    __device__ static __forceinline__ V lerp(float a, float b, V q, V p)
    {
        V x = a * q;
        V y = b * p;
        return x + y;
    }
    __device__ static __forceinline__ S lerp_s(float a, float b, S q, S p) { return lerp1(a, b, q, p); }
};

struct OpsBF16 {
    using V = u32x4;
    using S = uint16_t;
    static constexpr int PER = 8;
    static constexpr bool TAIL = true;
    __device__ static __forceinline__ V lerp(float a, float b, V q, V p)
    {
        V r;
        r.x = lerp_bf16x2(a, b, q.x, p.x);
        r.y = lerp_bf16x2(a, b, q.y, p.y);
        r.z = lerp_bf16x2(a, b, q.z, p.z);
        r.w = lerp_bf16x2(a, b, q.w, p.w);
        return r;
    }
    __device__ static __forceinline__ S lerp_s(float a, float b, S q, S p)
    {
        return (S)(lerp_bf16x2(a, b, (uint32_t)q, (uint32_t)p) & 0xffffu);
    }
};

struct OpsF16 {
    using V = u32x4;
    using S = uint16_t;
    static constexpr int PER = 8;
    static constexpr bool TAIL = true;
    __device__ static __forceinline__ V lerp(float a, float b, V q, V p)
    {
        V r;
        r.x = lerp_f16x2(a, b, q.x, p.x);
        r.y = lerp_f16x2(a, b, q.y, p.y);
        r.z = lerp_f16x2(a, b, q.z, p.z);
        r.w = lerp_f16x2(a, b, q.w, p.w);
        return r;
    }
    __device__ static __forceinline__ S lerp_s(float a, float b, S q, S p)
    {
        return lerp_f16x1(a, b, q, p);
    }
};

// A run-time dtype as an element-op type: f(OpsF32{}) and so on.
template <class F> static hipError_t with_ops(int32_t dtype, F &&f)
{
    switch (dtype) {
    case DPWA_F32: return f(OpsF32{});
    case DPWA_BF16: return f(OpsBF16{});
    case DPWA_F16: return f(OpsF16{});
    default: return hipErrorInvalidValue;
    }
}

// The loss given to update_send / update_wait: a host double, or read on the device from a
// float64 or float32 scalar (a loss tensor, so the host never synchronises).
__device__ __forceinline__ double read_loss(const double *d, int32_t f32, double h)
{
    if (!d) return h;
    return f32 ? (double)*reinterpret_cast<const float *>(d) : *d;
}

// ---------------------------------------------------------------- factor math
// dpwa.py:139-155 in IEEE double with every operation separately rounded, exactly as
// CPython evaluates it.  Python raises ZeroDivisionError on x/0.0; here that is status 1,
// the clock is left unchanged and the lerp becomes a no-op.
__device__ __forceinline__ dpwa_coef factor_math(const dpwa_interp &cfg, double c, double pc, double pl, double loss)
{
    int32_t status = DPWA_STATUS_OK;
    double f = 0.0;
    if (cfg.method == DPWA_INTERP_CONSTANT) {          // interpolation.py:13-15
        f = cfg.value;
    } else if (cfg.method == DPWA_INTERP_CLOCK) {      // interpolation.py:22-24
        const double den = c + pc;
        if (den == 0.0) status = DPWA_STATUS_ZERO_DIVISION;
        else f = pc / den;
    } else {                                           // interpolation.py:31-33
        const double den = loss + pl;
        if (den == 0.0) status = DPWA_STATUS_ZERO_DIVISION;
        else f = loss / den;
    }
    if (status == DPWA_STATUS_OK && loss < cfg.divergence_threshold) {   // dpwa.py:146-147
        if (cfg.divergence_threshold == 0.0) status = DPWA_STATUS_ZERO_DIVISION;
        else f = f * (loss / cfg.divergence_threshold);
    }
    dpwa_coef out;
    out.status = status;
    out.reserved = 0;
    if (status == DPWA_STATUS_OK) {
        out.factor = f;
        out.new_clock = f * pc + (1.0 - f) * c;        // dpwa.py:150
        out.a = (float)f;                              // torch: Python float -> fp32 scalar
        out.b = (float)(1.0 - f);                      // `1 - factor` in double, then fp32
    } else {
        out.factor = 0.0;
        out.new_clock = c;
        out.a = 0.0f;
        out.b = 1.0f;
    }
    return out;
}

__device__ __forceinline__ void factor_commit(const FusedArgs &fa, const dpwa_coef &c)
{
    *fa.clock_out = c.new_clock;                       // dpwa.py:155 (unchanged on error)
    *fa.coef_out = c;
    // sticky, and an error only: a round skipped for a non-finite peer must not make the next call raise
    if (fa.status_mirror && c.status == DPWA_STATUS_ZERO_DIVISION) *fa.status_mirror = c.status;
    if (c.status == DPWA_STATUS_PEER_NONFINITE) *fa.skips = *fa.skips + 1;   // (this lane alone writes it)
    if (fa.next_header) {                              // the next publish's state, written ahead
        const double next = c.new_clock + 1.0;         // dpwa.py:112 of that publish
        *fa.clock_next = next;
        dpwa_header *h = fa.next_header;
        h->clock = next;
        h->loss = __builtin_nan("");
        h->version = fa.next_version;
        h->n = fa.n;
        h->dtype = fa.dtype;
    }
}

// The fused-factor prologue: the (uniform) factor, evaluated by every lane that calls this;
// `commit` is true for the one lane of the grid that also writes it out.
// A learner that skips non-finite peers (fa.veto non-null; "non-finite peer check" below) has had
// k_peer_finite* look at the snapshot earlier on this stream: the veto word equals this round's
// stamp when it found a NaN or an inf.  Such a round is the no-op round with a status of its own,
// DPWA_STATUS_PEER_NONFINITE, which is no error; ZeroDivision keeps precedence.  The word is a
// uniform load from a kernel-argument pointer, issued before the factor math it overlaps with.
__device__ __forceinline__ dpwa_coef fused_factor(const FusedArgs &fa, bool commit)
{
    const bool vetoed = fa.veto && *fa.veto == fa.stamp;
    const double clock = *fa.clock_in;
    dpwa_coef c = factor_math(fa.cfg, clock, fa.hdr->clock, fa.hdr->loss, read_loss(fa.loss_d, fa.loss_f32, fa.loss_h));
    if (vetoed && c.status == DPWA_STATUS_OK) {
        c.status = DPWA_STATUS_PEER_NONFINITE;
        c.factor = 0.0;
        c.new_clock = clock;
        c.a = 0.0f;
        c.b = 1.0f;
    }
    if (commit) factor_commit(fa, c);
    return c;
}

__global__ void k_factor(FusedArgs fa)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    fused_factor(fa, true);
}

hipError_t launch_factor(const FusedArgs &fa, hipStream_t s)
{
    hipLaunchKernelGGL(k_factor, dim3(1), dim3(64), 0, s, fa);
    return hipGetLastError();
}

// ---------------------------------------------------------------- lerp kernels
enum CoefMode { COEF_HOST = 0, COEF_DEV = 1, COEF_FUSED = 2 };

struct LerpArgs {
    float a, b;                  // COEF_HOST
    const dpwa_coef *coef;       // COEF_DEV
    FusedArgs fused;             // COEF_FUSED
    void *snap;                  // DUAL: second destination (the next snapshot's payload)
};

// The MODE ladder: this launch's (a, b).  False: nothing to average -- COEF_DEV after a factor
// kernel that failed, COEF_FUSED in a no-op round.  The fused factor is evaluated in fp64 by
// every lane, which keeps the uniform (a, b) in registers (no LDS hand-off, no barrier), or with
// LDS (workgroups of more than one wave) by wave 0, which shares them through LDS; callers
// issue their loads first, so that they are in flight meanwhile.  Lane 0 of the workgroup for
// which `first_wg` holds commits the factor.
template <int MODE, bool LDS = false>
__device__ __forceinline__ bool lerp_coef(const LerpArgs &args, bool first_wg, float &a, float &b)
{
    if (MODE == COEF_HOST) {
        a = args.a;
        b = args.b;
        return true;
    } else if (MODE == COEF_DEV) {
        if (args.coef->status != DPWA_STATUS_OK) return false;
        a = args.coef->a;
        b = args.coef->b;
        return true;
    } else if (!LDS) {
        const dpwa_coef c = fused_factor(args.fused, first_wg && threadIdx.x == 0);
        a = c.a;
        b = c.b;
        return c.status == DPWA_STATUS_OK;
    } else {
        __shared__ float s_a, s_b;
        __shared__ int s_ok;
        if (threadIdx.x < 64) {
            const dpwa_coef c = fused_factor(args.fused, false);   // (lane 0's commit follows its hand-off)
            if (threadIdx.x == 0) {
                s_a = c.a;
                s_b = c.b;
                s_ok = c.status == DPWA_STATUS_OK;
                if (first_wg) factor_commit(args.fused, c);
            }
        }
        __syncthreads();
        a = s_a;
        b = s_b;
        return s_ok != 0;
    }
}

// ---------------------------------------------------------------- streaming buffer access
// Every workgroup covers one span (BLOCK lanes x 16 B) of each operand through its own
// buffer descriptor: 32-bit lane offsets whatever the buffer size (7B bf16 = 14 GB), and the
// hardware range check drops the lanes past the end (loads return 0, stores are discarded),
// so no lane branches.  Cache policy, chosen by measurement (tools/lerp_tune.hip,
// profiles/r01b_lerp_tune_*): loads `nt` (each byte is read once per round) and stores `sc1`;
// against plain loads/stores 11.2M fp32 went from 25.4 to 21.6 us cold and from 18.0 to
// 16.4 us Infinity-Cache warm, 100M fp32 from 198 to 189 us.
constexpr int kSpan = kBlock * 16;
// The averaging and publish kernels run one-wave (64-lane) workgroups: inside the gossip
// round (tools/block_sweep.sh, profiles/r01e_block_sweep_*.log) 64 beat 128/256/512 lanes
// cold at 11.2M fp32 (21.7 vs 22.5 us) and at 100M (179-183 vs 182-194 us), and the round
// with a 64-lane publish was the fastest or within noise of it at both sizes.
constexpr int kStreamBlock = 64;
constexpr int kAuxStream = 2;    // nt
constexpr int kAuxStore = 16;    // sc1

template <int SPAN = kSpan>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_rsrc(const void *base, int64_t off, int64_t total)
{
    const int64_t rem = total - off;
    const int num = rem <= 0 ? 0 : (rem < SPAN ? (int)rem : SPAN);
    return __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)base + off), 0, num, 0x00020000);
}

template <class V, int AUX = kAuxStream>
__device__ __forceinline__ V span_load(__amdgpu_buffer_rsrc_t r, int lane_off)
{
    return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(r, lane_off, 0, AUX));
}

template <class V, int AUX = kAuxStore>
__device__ __forceinline__ void span_store(__amdgpu_buffer_rsrc_t r, int lane_off, V v)
{
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, lane_off, 0, AUX);
}

// Cache policies of the averaging kernel (a bit set; cache-sized launches use 0, larger ones and
// the resident forms 8, see policy.hpp and lerp_policy()):
// the peer snapshot is always read `nt`; the parameters are read `nt` or, with bit 1, with the
// default policy; the result is stored `sc1`, with bit 2 `sc0 sc1`, with bit 4 `nt sc1`.
template <int POLICY> struct LerpPolicy {
    static constexpr int param_load = (POLICY & 1) ? 0 : kAuxStream;
    static constexpr int base_store = kAuxStore | ((POLICY & 2) ? 1 : 0) | ((POLICY & 4) ? kAuxStream : 0);
    // bit 16: only the next snapshot is stored `nt` (a co-resident peer reads it two averages
    // later; this learner's parameters, re-read by its next average one average later, keep
    // the Infinity Cache)
    static constexpr int snap_store = base_store | ((POLICY & 16) ? kAuxStream : 0);
    // bit 8: the parameters are stored `nt`, leaving the Infinity Cache to the snapshot a peer
    // reads next (the product policy)
    static constexpr int store = base_store | ((POLICY & 8) ? kAuxStream : 0);
};

// Where the peer's bytes are.  ContigSrc: one buffer (a staging buffer, or a peer's slot
// read in place).  StripeSrc: the relay's stripes, stripe s at src[s] (k_lerp_relay).
struct ContigSrc {
    const char *p;
    // byte offset of workgroup b's span: spans in order
    template <int SPAN>
    __device__ __forceinline__ int64_t span_of(uint32_t b) const { return (int64_t)b * SPAN; }
    // base such that base + byte_offset addresses the span starting at span_off
    __device__ __forceinline__ const char *span_base(int64_t) const { return p; }
    __device__ __forceinline__ const char *at(int64_t byte) const { return p + byte; }
};

struct StripeSrc {
    const char *src[kMaxRelayRanks];
    int64_t stripe;    // a multiple of every span (4 KiB multiple): no span straddles stripes
    int32_t parts;     // stripes (ranks)
    // Consecutive workgroups take consecutive stripes (b % parts), so the workgroups in flight
    // at any moment read from every stripe holder -- every xGMI link -- at once, not one
    // stripe (one link) after another.
    template <int SPAN>
    __device__ __forceinline__ int64_t span_of(uint32_t b) const
    {
        return (int64_t)(b % (uint32_t)parts) * stripe + (int64_t)(b / (uint32_t)parts) * SPAN;
    }
    __device__ __forceinline__ const char *span_base(int64_t span_off) const
    {
        const int64_t s = span_off / stripe;
        return src[s] - s * stripe;
    }
    __device__ __forceinline__ const char *at(int64_t byte) const
    {
        const int64_t s = byte / stripe;
        return src[s] + (byte - s * stripe);
    }
};

// ---------------------------------------------------------------- distance to the peer
// The opt-in measurement of a round (include/dpwa_hip.h dpwa_distance): dist2 = sum (q - p)^2 and
// norm2 = sum p^2 over the operands as they were before the average, every element widened
// exactly to fp64 and every difference, product and sum in fp64 (contraction is off: a separate
// multiply and add).  A lane sums its own elements in order, the wave sums its lanes with a
// fixed xor butterfly of shuffles (no LDS memory), and lanes 0 and 1 add the pair into one of
// kDistAccs accumulators with the hardware fp64 add, the accumulator chosen by the span's index
// so that the workgroups in flight do not meet on one address.  Each accumulator has a 128-byte
// row of its own (float atomics that all land in one row run an order of magnitude slower).
// k_distance_finish sums the accumulators in a fixed order; the order in which workgroups
// reached an accumulator is not fixed, so the record is the library's one output that is not
// bit-exact from run to run (it is within (n - 1) 2^-53 relative, all terms being >= 0).
constexpr int kDistAccs = 1024;
constexpr int kDistAccStride = 128 / (int)sizeof(double);   // doubles from one accumulator to the next
static_assert((size_t)kDistAccs * kDistAccStride * sizeof(double) == kDistanceWorkspaceBytes, "workspace size");

__device__ __forceinline__ void dist_term(double q, double p, double &d2, double &n2)
{
    const double d = q - p;
    d2 = d2 + d * d;
    n2 = n2 + p * p;
}

__device__ __forceinline__ void dist_add_bf16x2(uint32_t q, uint32_t p, double &d2, double &n2)
{
    dist_term((double)bf_lo(q), (double)bf_lo(p), d2, n2);
    dist_term((double)bf_hi(q), (double)bf_hi(p), d2, n2);
}

__device__ __forceinline__ void dist_add_f16x2(uint32_t q, uint32_t p, double &d2, double &n2)
{
    const f16x2v qh = __builtin_bit_cast(f16x2v, q), ph = __builtin_bit_cast(f16x2v, p);
    dist_term((double)qh.x, (double)ph.x, d2, n2);
    dist_term((double)qh.y, (double)ph.y, d2, n2);
}

// One lane's 16-byte item, its elements in order.
__device__ __forceinline__ void dist_add(OpsF32, f32x4 q, f32x4 p, double &d2, double &n2)
{
    dist_term((double)q.x, (double)p.x, d2, n2);
    dist_term((double)q.y, (double)p.y, d2, n2);
    dist_term((double)q.z, (double)p.z, d2, n2);
    dist_term((double)q.w, (double)p.w, d2, n2);
}

__device__ __forceinline__ void dist_add(OpsBF16, u32x4 q, u32x4 p, double &d2, double &n2)
{
    dist_add_bf16x2(q.x, p.x, d2, n2);
    dist_add_bf16x2(q.y, p.y, d2, n2);
    dist_add_bf16x2(q.z, p.z, d2, n2);
    dist_add_bf16x2(q.w, p.w, d2, n2);
}

__device__ __forceinline__ void dist_add(OpsF16, u32x4 q, u32x4 p, double &d2, double &n2)
{
    dist_add_f16x2(q.x, p.x, d2, n2);
    dist_add_f16x2(q.y, p.y, d2, n2);
    dist_add_f16x2(q.z, p.z, d2, n2);
    dist_add_f16x2(q.w, p.w, d2, n2);
}

// One element (the ragged tail, the unaligned kernel).
__device__ __forceinline__ void dist_add_s(OpsF32, float q, float p, double &d2, double &n2)
{
    dist_term((double)q, (double)p, d2, n2);
}

__device__ __forceinline__ void dist_add_s(OpsBF16, uint16_t q, uint16_t p, double &d2, double &n2)
{
    dist_term((double)bf_lo(q), (double)bf_lo(p), d2, n2);
}

__device__ __forceinline__ void dist_add_s(OpsF16, uint16_t q, uint16_t p, double &d2, double &n2)
{
    dist_term((double)__builtin_bit_cast(_Float16, q), (double)__builtin_bit_cast(_Float16, p), d2, n2);
}

// The sum over the wave's 64 lanes, the same in every lane: a xor butterfly, so the order of the
// additions is fixed.
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// The wave's pair into accumulator `index` mod kDistAccs: one atomic instruction, lane 0 adding
// dist2 and lane 1 norm2 (global_atomic_add_f64, no compare-and-swap loop; the accumulators are
// ordinary device memory).
__device__ __forceinline__ void dist_commit(double *acc, uint32_t index, double d2, double n2)
{
    d2 = wave_sum(d2);
    n2 = wave_sum(n2);
    const int lane = threadIdx.x & 63;
    if (lane < 2) unsafeAtomicAdd(acc + (size_t)(index % kDistAccs) * kDistAccStride + lane, lane ? n2 : d2);
}

// What lerp_span does about the distance: nothing (every averaging kernel but k_lerp_tracked), or
// the sums above into `acc`.
struct NoTrack {
    static constexpr bool ON = false;
};
struct DistTrack {
    static constexpr bool ON = true;
    double *acc;
};

// One 16-byte item per lane; items beyond n/PER (the ragged tail) go to block 0.
// DUAL also stores the result into args.snap (write-through snapshot: the next publish of
// these parameters then needs no copy).  OOP (with DUAL): the result is stored into args.snap
// ONLY -- the resident form, whose parameters live in the learner's own snapshot slots and move
// from the published slot to the next one at every average (2 reads + 1 write per element, the
// averaging's own bytes; learner.cpp "resident").  BLOCK lanes per workgroup (kStreamBlock).
// Track (DistTrack, one-wave workgroups only): a round that averages also adds its distance sums,
// formed from the q and p this lane loaded anyway; a no-op round adds nothing.
template <class Ops, int MODE, bool DUAL, int BLOCK, int POLICY, class Src, bool OOP = false, class Track = NoTrack>
__device__ __forceinline__ void lerp_span(uint32_t blk, typename Ops::V *__restrict__ param, const Src &src,
                                          int64_t n, const LerpArgs &args, const Ops &ops = Ops{},
                                          const Track &track = Track{})
{
    static_assert(!Track::ON || BLOCK == 64, "the tracked form runs one-wave workgroups");
    using V = typename Ops::V;
    using P = LerpPolicy<POLICY>;
    constexpr int SPAN = BLOCK * 16;
    const int64_t vbytes = Ops::TAIL ? n / Ops::PER * 16 : n;   // the whole 16-byte items
    const int64_t span_off = src.template span_of<SPAN>(blk);
    const int lane_off = threadIdx.x * 16;
    const __amdgpu_buffer_rsrc_t rq = span_rsrc<SPAN>(src.span_base(span_off), span_off, vbytes);
    const __amdgpu_buffer_rsrc_t rp = span_rsrc<SPAN>(param, span_off, vbytes);
    // issue this lane's loads before anything else
    const V q = span_load<V>(rq, lane_off);
    const V p = span_load<V, P::param_load>(rp, lane_off);
    float a, b;
    if (!lerp_coef<MODE, BLOCK != 64>(args, blk == 0, a, b)) {
        if (MODE == COEF_FUSED && DUAL) {   // no-op round; a write-through snapshot still gets the parameters
            span_store<V, P::snap_store>(span_rsrc<SPAN>(args.snap, span_off, vbytes), lane_off, p);
            if constexpr (Ops::TAIL) {
                const int64_t tail = n / Ops::PER * Ops::PER;
                if (blk == 0 && threadIdx.x < n - tail) {
                    const int64_t j = tail + threadIdx.x;
                    reinterpret_cast<typename Ops::S *>(args.snap)[j] = reinterpret_cast<typename Ops::S *>(param)[j];
                }
            }
        }
        return;
    }
    const V r = ops.lerp(a, b, q, p);
    if (!OOP) span_store<V, P::store>(rp, lane_off, r);
    if (DUAL) span_store<V, P::snap_store>(span_rsrc<SPAN>(args.snap, span_off, vbytes), lane_off, r);
    [[maybe_unused]] double d2 = 0.0, n2 = 0.0;
    if constexpr (Track::ON) dist_add(ops, q, p, d2, n2);
    if constexpr (Ops::TAIL) {
        using S = typename Ops::S;
        S *ps = reinterpret_cast<S *>(param);
        const int64_t tail = n / Ops::PER * Ops::PER;
        if (blk == 0 && threadIdx.x < n - tail) {
            const int64_t j = tail + threadIdx.x;
            const S qs = *reinterpret_cast<const S *>(src.at(j * (int64_t)sizeof(S))), pj = ps[j];
            const S t = Ops::lerp_s(a, b, qs, pj);
            if (!OOP) ps[j] = t;
            if (DUAL) reinterpret_cast<S *>(args.snap)[j] = t;
            if constexpr (Track::ON) dist_add_s(ops, qs, pj, d2, n2);
        }
    }
    if constexpr (Track::ON) dist_commit(track.acc, blk, d2, n2);
}

template <class Ops, int MODE, bool DUAL, int BLOCK = kBlock, int POLICY = 0, bool OOP = false>
__global__ __launch_bounds__(BLOCK) void k_lerp(typename Ops::V *__restrict__ param,
                                                const typename Ops::V *__restrict__ peer, int64_t n, LerpArgs args)
{
    lerp_span<Ops, MODE, DUAL, BLOCK, POLICY, ContigSrc, OOP>(blockIdx.x, param, ContigSrc{(const char *)peer}, n,
                                                              args);
}

// ---------------------------------------------------------------- segmented (DPWA_MIXED) payloads
// A model that mixes float32, bfloat16 and float16 parameters has a payload of up to three
// segments, one per type, each a whole number of 4-KiB blocks (dpwa_layout, include/dpwa_hip.h): a
// 1-KiB span lies inside one segment.  The table travels by value; unused entries begin at
// INT64_MAX, so the lookup is two compares whatever the count.
struct SegTable {
    int64_t begin[DPWA_LAYOUT_MAX_SEGMENTS];   // ascending, begin[0] = 0
    int32_t dtype[DPWA_LAYOUT_MAX_SEGMENTS];
};

// The type of the segment holding byte `off` (uniform: from kernel arguments and the span offset).
__device__ __forceinline__ int32_t seg_dtype(const SegTable &t, int64_t off)
{
    int32_t d = t.dtype[0];
#pragma unroll
    for (int k = 1; k < DPWA_LAYOUT_MAX_SEGMENTS; ++k)
        if (off >= t.begin[k]) d = t.dtype[k];
    return d;
}

// The element op of a segmented payload's span: OpsF32 / OpsBF16 / OpsF16 ::lerp, so each type
// rounds exactly as its own kernel, chosen under a uniform branch by the type of the segment the
// span lies in (looked up here, after the span's loads were issued).  No ragged tail: n counts
// the payload's bytes, a multiple of 4 KiB.
struct OpsMixed {
    using V = u32x4;
    static constexpr int PER = 16;
    static constexpr bool TAIL = false;
    const SegTable &segs;
    int64_t span_off;
    __device__ __forceinline__ V lerp(float a, float b, V q, V p) const
    {
        const int32_t dtype = seg_dtype(segs, span_off);
        if (dtype == DPWA_F32)
            return __builtin_bit_cast(V, OpsF32::lerp(a, b, __builtin_bit_cast(f32x4, q), __builtin_bit_cast(f32x4, p)));
        if (dtype == DPWA_BF16) return OpsBF16::lerp(a, b, q, p);
        return OpsF16::lerp(a, b, q, p);
    }
};

// The single-dtype span code (lerp_span: one 16-byte item per lane, loads first, the fp64 factor
// by every lane while they are in flight, the commit by one lane of the grid -- of global
// workgroup 0, not of the first workgroup of each segment -- and the no-op round) for a
// segmented payload: the span's element op is chosen by the span's byte offset (not by the
// workgroup index: right for any span order).  No unaligned form, and the grid is exact.
// One-wave workgroups.
template <int MODE, bool DUAL, int POLICY, bool OOP>
__global__ __launch_bounds__(kStreamBlock) void k_lerp_mixed(u32x4 *__restrict__ param,
                                                             const u32x4 *__restrict__ peer, int64_t total,
                                                             LerpArgs args, SegTable segs)
{
    const ContigSrc src{(const char *)peer};
    const OpsMixed ops{segs, src.span_of<kStreamBlock * 16>(blockIdx.x)};
    lerp_span<OpsMixed, MODE, DUAL, kStreamBlock, POLICY, ContigSrc, OOP>(blockIdx.x, param, src, total, args, ops);
}

// The tracked form of the single-learner fused average (k_lerp's span code with DistTrack, so the
// averaged bits are k_lerp's): plain, write-through (DUAL) and resident (OOP), one-wave
// workgroups, the cache policy k_lerp would take (by size; resident: kProductPolicy).  `acc`: the
// distance accumulators.
template <class Ops, bool DUAL, bool OOP, int POLICY>
__global__ __launch_bounds__(kStreamBlock) void k_lerp_tracked(typename Ops::V *__restrict__ param,
                                                               const typename Ops::V *__restrict__ peer, int64_t n,
                                                               LerpArgs args, double *__restrict__ acc)
{
    lerp_span<Ops, COEF_FUSED, DUAL, kStreamBlock, POLICY, ContigSrc, OOP, DistTrack>(
        blockIdx.x, param, ContigSrc{(const char *)peer}, n, args, Ops{}, DistTrack{acc});
}

// The stand-alone distance pass: the same sums with no store to either operand, for the averaging
// forms that have no tracked kernel (it runs before their average, on the same stream) and for
// dpwa_measure_distance.  The spans are the averaging kernel's; the loads take the default cache
// policy, since the average that follows reads the same bytes again.
template <class Ops>
__global__ __launch_bounds__(kStreamBlock) void k_distance(const typename Ops::V *__restrict__ param,
                                                           const typename Ops::V *__restrict__ peer, int64_t n,
                                                           double *__restrict__ acc)
{
    using V = typename Ops::V;
    using S = typename Ops::S;
    constexpr int SPAN = kStreamBlock * 16;
    const int64_t vbytes = n / Ops::PER * 16;
    const int64_t span_off = (int64_t)blockIdx.x * SPAN;
    const int lane_off = threadIdx.x * 16;
    const V q = span_load<V, 0>(span_rsrc<SPAN>(peer, span_off, vbytes), lane_off);
    const V p = span_load<V, 0>(span_rsrc<SPAN>(param, span_off, vbytes), lane_off);
    double d2 = 0.0, n2 = 0.0;
    dist_add(Ops{}, q, p, d2, n2);
    const int64_t tail = n / Ops::PER * Ops::PER;
    if (blockIdx.x == 0 && threadIdx.x < n - tail) {
        const int64_t j = tail + threadIdx.x;
        dist_add_s(Ops{}, reinterpret_cast<const S *>(peer)[j], reinterpret_cast<const S *>(param)[j], d2, n2);
    }
    dist_commit(acc, blockIdx.x, d2, n2);
}

// The same over a segmented payload: the span's type is its segment's (no ragged tail; padding
// bytes are zeros on both sides and add nothing).
__global__ __launch_bounds__(kStreamBlock) void k_distance_mixed(const u32x4 *__restrict__ param,
                                                                 const u32x4 *__restrict__ peer, int64_t total,
                                                                 SegTable segs, double *__restrict__ acc)
{
    constexpr int SPAN = kStreamBlock * 16;
    const int64_t span_off = (int64_t)blockIdx.x * SPAN;
    const int lane_off = threadIdx.x * 16;
    const u32x4 q = span_load<u32x4, 0>(span_rsrc<SPAN>(peer, span_off, total), lane_off);
    const u32x4 p = span_load<u32x4, 0>(span_rsrc<SPAN>(param, span_off, total), lane_off);
    const int32_t dtype = seg_dtype(segs, span_off);
    double d2 = 0.0, n2 = 0.0;
    if (dtype == DPWA_F32) dist_add(OpsF32{}, __builtin_bit_cast(f32x4, q), __builtin_bit_cast(f32x4, p), d2, n2);
    else if (dtype == DPWA_BF16) dist_add(OpsBF16{}, q, p, d2, n2);
    else dist_add(OpsF16{}, q, p, d2, n2);
    dist_commit(acc, blockIdx.x, d2, n2);
}

// Element-wise form for operands that are not 16-byte aligned: a grid-stride loop, each wave
// adding its pair into the accumulator of its index in the grid.
template <class Ops>
__global__ __launch_bounds__(kBlock) void k_distance_unaligned(const typename Ops::S *__restrict__ param,
                                                               const typename Ops::S *__restrict__ peer, int64_t n,
                                                               double *__restrict__ acc)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double d2 = 0.0, n2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        dist_add_s(Ops{}, peer[i], param[i], d2, n2);
    dist_commit(acc, blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), d2, n2);
}

// Finishing (one workgroup, after the pass on the same stream: the kernel boundary orders it
// behind every add): one lane per accumulator, so every load is in flight at once; the sums are
// taken in a fixed order -- the butterfly inside each wave, then the waves in order -- and the
// accumulators are left zero for the next round.  The record is written only when the round
// averaged (`coef` null, or its status OK); its clock is the one that round committed (0 without
// a coef).  The accumulators are read and zeroed with agent-scope accesses: the adds that fill
// them never pass through an L2.
constexpr int kDistFinishBlock = kDistAccs;
static_assert(kDistFinishBlock <= 1024 && kDistFinishBlock % 64 == 0, "one lane per accumulator");

__global__ __launch_bounds__(kDistFinishBlock) void k_distance_finish(double *__restrict__ acc,
                                                                      dpwa_distance *__restrict__ out,
                                                                      const dpwa_coef *__restrict__ coef, int64_t n)
{
    __shared__ double s_d2[kDistFinishBlock / 64], s_n2[kDistFinishBlock / 64];
    double *a = acc + (size_t)threadIdx.x * kDistAccStride;
    double d2 = __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double n2 = __hip_atomic_load(a + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a + 1, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    d2 = wave_sum(d2);
    n2 = wave_sum(n2);
    if ((threadIdx.x & 63) == 0) {
        s_d2[threadIdx.x >> 6] = d2;
        s_n2[threadIdx.x >> 6] = n2;
    }
    __syncthreads();
    if (threadIdx.x != 0 || (coef && coef->status != DPWA_STATUS_OK)) return;
    d2 = s_d2[0];
    n2 = s_n2[0];
#pragma unroll
    for (int w = 1; w < kDistFinishBlock / 64; ++w) {
        d2 = d2 + s_d2[w];
        n2 = n2 + s_n2[w];
    }
    out->dist2 = d2;
    out->norm2 = n2;
    out->clock = coef ? coef->new_clock : 0.0;
    out->n = n;
}

// ---------------------------------------------------------------- non-finite peer check
// Opt-in (dpwa_learner_set_finite_check): before a round averages, one pass reads the fetched peer
// snapshot and vetoes the round when any element of it is NaN or +-inf, so that one replica that
// overflowed does not spread through the gossip.  k_distance's shape: one-wave workgroups, one
// 16-byte item per lane, an exact grid of 1-KiB spans whose lanes past the end load zeros (finite),
// the ragged tail element by element in workgroup 0.
//
// The test is on bit patterns: an element is non-finite when its exponent field is all ones, both
// halves of every dword for the 16-bit types.  No float compare and no conversion, so signalling
// NaNs, subnormals and the largest finite values come out right whatever the denormal or NaN mode.
//
// No reduction, no atomics, nothing to zero: the launch carries a non-zero stamp (the learner's
// count of checked rounds), and a lane that sees a non-finite element stores it into the veto word
// with a plain vector store -- several lanes store the same value.  The word is never cleared; it
// vetoes a round only while it equals that round's stamp (fused_factor), which the kernel boundary
// behind this pass orders after every store.
//
// AUX: the cache policy of the loads.  The average that follows reads the same bytes again, so
// they take the default policy, at every size (finite_aux(): measured against `nt`).
__device__ __forceinline__ bool nonfinite_f32(uint32_t w) { return (w & 0x7f800000u) == 0x7f800000u; }
// the two 16-bit elements of a dword, exponent mask M (bf16 0x7f80, fp16 0x7c00)
template <uint32_t M> __device__ __forceinline__ bool nonfinite_16x2(uint32_t w)
{
    return (w & M) == M || (w & (M << 16)) == (M << 16);
}

__device__ __forceinline__ bool peer_bad(OpsF32, u32x4 q)
{
    return nonfinite_f32(q.x) || nonfinite_f32(q.y) || nonfinite_f32(q.z) || nonfinite_f32(q.w);
}
__device__ __forceinline__ bool peer_bad(OpsBF16, u32x4 q)
{
    return nonfinite_16x2<0x7f80u>(q.x) || nonfinite_16x2<0x7f80u>(q.y) || nonfinite_16x2<0x7f80u>(q.z) ||
           nonfinite_16x2<0x7f80u>(q.w);
}
__device__ __forceinline__ bool peer_bad(OpsF16, u32x4 q)
{
    return nonfinite_16x2<0x7c00u>(q.x) || nonfinite_16x2<0x7c00u>(q.y) || nonfinite_16x2<0x7c00u>(q.z) ||
           nonfinite_16x2<0x7c00u>(q.w);
}
// One element, as its bits (FiniteBits<Ops>::T: an unsigned integer of the element's size).
__device__ __forceinline__ bool peer_bad_s(OpsF32, uint32_t q) { return nonfinite_f32(q); }
__device__ __forceinline__ bool peer_bad_s(OpsBF16, uint16_t q) { return (q & 0x7f80u) == 0x7f80u; }
__device__ __forceinline__ bool peer_bad_s(OpsF16, uint16_t q) { return (q & 0x7c00u) == 0x7c00u; }
template <class Ops> struct FiniteBits {
    using T = std::conditional_t<sizeof(typename Ops::S) == 4, uint32_t, uint16_t>;
};

template <class Ops, int AUX>
__global__ __launch_bounds__(kStreamBlock) void k_peer_finite(const void *__restrict__ peer, int64_t n, uint32_t *veto,
                                                              uint32_t stamp)
{
    using B = typename FiniteBits<Ops>::T;
    constexpr int SPAN = kStreamBlock * 16;
    const int64_t vbytes = n / Ops::PER * 16;
    const int64_t span_off = (int64_t)blockIdx.x * SPAN;
    const u32x4 q = span_load<u32x4, AUX>(span_rsrc<SPAN>(peer, span_off, vbytes), threadIdx.x * 16);
    bool bad = peer_bad(Ops{}, q);
    const int64_t tail = n / Ops::PER * Ops::PER;
    if (blockIdx.x == 0 && threadIdx.x < n - tail) bad = bad || peer_bad_s(Ops{}, reinterpret_cast<const B *>(peer)[tail + threadIdx.x]);
    if (bad) *veto = stamp;
}

// The same over a segmented payload: the span's test is its segment's (seg_dtype from the span's
// byte offset, as k_lerp_mixed; no ragged tail; padding bytes are zeros, which are finite).
template <int AUX>
__global__ __launch_bounds__(kStreamBlock) void k_peer_finite_mixed(const u32x4 *__restrict__ peer, int64_t total,
                                                                    SegTable segs, uint32_t *veto, uint32_t stamp)
{
    constexpr int SPAN = kStreamBlock * 16;
    const int64_t span_off = (int64_t)blockIdx.x * SPAN;
    const u32x4 q = span_load<u32x4, AUX>(span_rsrc<SPAN>(peer, span_off, total), threadIdx.x * 16);
    const int32_t dtype = seg_dtype(segs, span_off);
    const bool bad = dtype == DPWA_F32 ? peer_bad(OpsF32{}, q) : dtype == DPWA_BF16 ? peer_bad(OpsBF16{}, q) : peer_bad(OpsF16{}, q);
    if (bad) *veto = stamp;
}

// Element-wise form for a single-dtype payload that is not 16-byte aligned: a grid-stride loop.
template <class Ops>
__global__ __launch_bounds__(kBlock) void k_peer_finite_unaligned(const typename FiniteBits<Ops>::T *__restrict__ peer,
                                                                  int64_t n, uint32_t *veto, uint32_t stamp)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) bad = bad || peer_bad_s(Ops{}, peer[i]);
    if (bad) *veto = stamp;
}

// ---------------------------------------------------------------- distance to the peer, per tensor
// The same two sums for every parameter tensor of the model over that tensor's own elements only
// (include/dpwa_hip.h "per-parameter distance"): a stand-alone pass beside k_distance, then one
// finishing workgroup per tensor.  A tensor starts on a 256-byte boundary of the payload only, so
// each 256-byte quarter of a 1-KiB span -- 16 lanes' items -- holds bytes of at most one tensor
// (and perhaps the gap behind it): a span holds at most four.  The tensors are a table in device
// memory sorted by byte_begin (a model has tens to thousands: too many for kernel arguments); the
// tensor of a quarter is the last entry that begins at or before it, found by a binary search on
// uniform values while the span's loads are in flight.  Bytes of no tensor (the 256-byte gaps, a
// segment's padding) are loaded with their item but never enter a sum: every element at or beyond
// its tensor's end is masked.
//
// Tensor t owns rows [first_row, first_row + rows), rows = min(spans it touches, kParamDistRows),
// each a 128-byte row as above; the tensor's span s (counted from the span holding its first
// byte) adds into row s mod rows, so that the workgroups in flight on one large tensor do not
// meet on one address, as in the whole-model pass.

// The last entry with begin <= off, or -1 (uniform in, uniform out).
__device__ __forceinline__ int param_lookup(const ParamEntry *__restrict__ table, int count, int64_t off)
{
    int lo = 0, hi = count;   // entries below lo begin at or before off, entries from hi on after it
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (table[mid].begin <= off) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// One element into the sums when `in` (it lies wholly before its tensor's end).
__device__ __forceinline__ void dist_term_if(bool in, double q, double p, double &d2, double &n2)
{
    const double d = q - p;
    const double a = d2 + d * d, b = n2 + p * p;
    d2 = in ? a : d2;
    n2 = in ? b : n2;
}

// A lane's 16-byte item at payload byte `at`, the elements whose bytes end at or before `end` only.
__device__ __forceinline__ void dist_add_until(int32_t dtype, u32x4 q, u32x4 p, int64_t at, int64_t end, double &d2,
                                               double &n2)
{
    const int64_t room = end - at;   // bytes of the tensor from this item on (<= 0: none)
    const uint32_t qw[4] = {q.x, q.y, q.z, q.w}, pw[4] = {p.x, p.y, p.z, p.w};
    if (dtype == DPWA_F32) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            dist_term_if(room >= 4 * (j + 1), (double)__uint_as_float(qw[j]), (double)__uint_as_float(pw[j]), d2, n2);
    } else if (dtype == DPWA_BF16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dist_term_if(room >= 4 * j + 2, (double)bf_lo(qw[j]), (double)bf_lo(pw[j]), d2, n2);
            dist_term_if(room >= 4 * j + 4, (double)bf_hi(qw[j]), (double)bf_hi(pw[j]), d2, n2);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f16x2v qh = __builtin_bit_cast(f16x2v, qw[j]), ph = __builtin_bit_cast(f16x2v, pw[j]);
            dist_term_if(room >= 4 * j + 2, (double)qh.x, (double)ph.x, d2, n2);
            dist_term_if(room >= 4 * j + 4, (double)qh.y, (double)ph.y, d2, n2);
        }
    }
}

// The sum over the 16 lanes of a quarter, the same in each of them: four xor steps.
__device__ __forceinline__ double quarter_sum(double v)
{
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// The row of tensor entry e that the payload span `span` adds into.
__device__ __forceinline__ double *param_row(double *acc, const ParamEntry &e, int64_t span)
{
    const uint32_t s = (uint32_t)(span - e.begin / (kStreamBlock * 16));   // the tensor's own span index (grid < 2^31)
    return acc + ((size_t)e.first_row + (size_t)(s % (uint32_t)e.rows)) * kDistAccStride;
}

// `total`: the payload's bytes; the vector loads cover its whole 16-byte items, and the bytes
// behind the last whole item (a single-dtype payload of n elements may end inside one) are read
// element by element by the lane whose item they would be.  One-wave workgroups, an exact grid of
// spans over the payload.  The loads take the default cache policy, as k_distance's.
__global__ __launch_bounds__(kStreamBlock) void k_param_distance(const u32x4 *__restrict__ param,
                                                                 const u32x4 *__restrict__ peer, int64_t total,
                                                                 const ParamEntry *__restrict__ table, int count,
                                                                 double *__restrict__ acc)
{
    constexpr int SPAN = kStreamBlock * 16;
    const int64_t vbytes = total / 16 * 16;
    const int64_t span_off = (int64_t)blockIdx.x * SPAN;
    const int lane = threadIdx.x;
    const int lane_off = lane * 16;
    u32x4 q = span_load<u32x4, 0>(span_rsrc<SPAN>(peer, span_off, vbytes), lane_off);
    u32x4 p = span_load<u32x4, 0>(span_rsrc<SPAN>(param, span_off, vbytes), lane_off);
    const int t0 = param_lookup(table, count, span_off);
    double d2 = 0.0, n2 = 0.0;
    if (t0 >= 0 && table[t0].end >= span_off + SPAN) {   // the span lies inside one tensor: k_distance's body
        const ParamEntry e = table[t0];
        if (e.dtype == DPWA_F32) dist_add(OpsF32{}, __builtin_bit_cast(f32x4, q), __builtin_bit_cast(f32x4, p), d2, n2);
        else if (e.dtype == DPWA_BF16) dist_add(OpsBF16{}, q, p, d2, n2);
        else dist_add(OpsF16{}, q, p, d2, n2);
        d2 = wave_sum(d2);
        n2 = wave_sum(n2);
        if (lane < 2) unsafeAtomicAdd(param_row(acc, e, blockIdx.x) + lane, lane ? n2 : d2);
        return;
    }
    const int64_t at = span_off + lane_off;
    if (at == vbytes && at < total) {   // the payload ends inside this lane's item: its bytes one by one
        const unsigned char *qb = (const unsigned char *)peer + at, *pb = (const unsigned char *)param + at;
        uint32_t qw[4] = {0, 0, 0, 0}, pw[4] = {0, 0, 0, 0};
        for (int b = 0; b < (int)(total - at); ++b) {
            qw[b >> 2] |= (uint32_t)qb[b] << (8 * (b & 3));
            pw[b >> 2] |= (uint32_t)pb[b] << (8 * (b & 3));
        }
        q = u32x4{qw[0], qw[1], qw[2], qw[3]};
        p = u32x4{pw[0], pw[1], pw[2], pw[3]};
    }
    // each quarter's tensor, then this lane's own by its quarter: the table is sorted, so a later
    // quarter's tensor is the one before it or one of the next few (a step or two forward, not another
    // search -- a search per quarter made the pass 82.6 us against 48.5 at 16,384 tensors).  The index
    // is the same in every lane, but the compiler emits these steps' loads as global_load_dwordx2 of
    // one address for the wave, not as scalar loads (readfirstlane on the index does not change that).
    int mine = -1, t = t0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        while (t + 1 < count && table[t + 1].begin <= span_off + k * 256) ++t;
        if ((lane >> 4) == k) mine = t;
    }
    ParamEntry e{};
    bool live = false;
    if (mine >= 0) {
        e = table[mine];
        live = e.end > span_off + (lane >> 4) * 256;   // else the quarter is all gap
    }
    if (live) dist_add_until(e.dtype, q, p, at, e.end, d2, n2);
    d2 = quarter_sum(d2);
    n2 = quarter_sum(n2);
    if (live && (lane & 15) < 2) unsafeAtomicAdd(param_row(acc, e, blockIdx.x) + (lane & 15), (lane & 15) ? n2 : d2);
}

// Finishing: one workgroup per tensor behind the pass (and behind the average, whose coefficients
// it reads) on the same stream.  kParamFinishBlock lanes, lane i taking rows i, i + kParamFinishBlock,
// ... of the tensor (all its loads in flight at once; most tensors of a model have a handful of rows,
// and a 1024-lane workgroup for each of 16,384 small tensors took 70 us); the sums in a fixed order
// -- a lane's rows in order, the butterfly inside each wave, then the waves in order -- and the rows
// left zero whatever the round did.  The tensor's pair -- and, by workgroup 0, the clock and the
// count -- is written only when the round averaged.  Agent-scope accesses, as k_distance_finish.
constexpr int kParamFinishBlock = 256;
static_assert(kParamDistRows % kParamFinishBlock == 0 && kParamFinishBlock % 64 == 0, "whole lanes' worth of rows");

__global__ __launch_bounds__(kParamFinishBlock) void k_param_distance_finish(double *__restrict__ acc,
                                                                            const ParamEntry *__restrict__ table,
                                                                            dpwa_param_distance_head *__restrict__ out,
                                                                            const dpwa_coef *__restrict__ coef,
                                                                            int64_t count)
{
    constexpr int PER = kParamDistRows / kParamFinishBlock;
    __shared__ double s_d2[kParamFinishBlock / 64], s_n2[kParamFinishBlock / 64];
    const ParamEntry e = table[blockIdx.x];
    double rd[PER], rn[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int row = (int)threadIdx.x + j * kParamFinishBlock;
        rd[j] = rn[j] = 0.0;
        if (row < e.rows) {
            double *a = acc + ((size_t)e.first_row + row) * kDistAccStride;
            rd[j] = __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            rn[j] = __hip_atomic_load(a + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a + 1, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    double d2 = rd[0], n2 = rn[0];
#pragma unroll
    for (int j = 1; j < PER; ++j) {
        d2 = d2 + rd[j];
        n2 = n2 + rn[j];
    }
    d2 = wave_sum(d2);
    n2 = wave_sum(n2);
    if ((threadIdx.x & 63) == 0) {
        s_d2[threadIdx.x >> 6] = d2;
        s_n2[threadIdx.x >> 6] = n2;
    }
    __syncthreads();
    if (threadIdx.x != 0 || (coef && coef->status != DPWA_STATUS_OK)) return;
    d2 = s_d2[0];
    n2 = s_n2[0];
#pragma unroll
    for (int w = 1; w < kParamFinishBlock / 64; ++w) {
        d2 = d2 + s_d2[w];
        n2 = n2 + s_n2[w];
    }
    dpwa_param_pair *pair = reinterpret_cast<dpwa_param_pair *>(out + 1) + blockIdx.x;   // the pairs follow the head
    pair->dist2 = d2;
    pair->norm2 = n2;
    if (blockIdx.x == 0) {
        out->clock = coef ? coef->new_clock : 0.0;
        out->count = count;
    }
}

// The relay's fused second phase: the fused average reads the peer's snapshot stripe by stripe
// where the relay left it (stripe s in rank s's relay buffer, the peer's own stripe in its slot,
// ours in local HBM) instead of gathering it into staging first.
template <class Ops, bool DUAL, int POLICY = 0, bool OOP = false>
__global__ __launch_bounds__(kStreamBlock) void k_lerp_relay(typename Ops::V *__restrict__ param, int64_t n,
                                                             LerpArgs args, StripeSrc src)
{
    lerp_span<Ops, COEF_FUSED, DUAL, kStreamBlock, POLICY, StripeSrc, OOP>(blockIdx.x, param, src, n, args);
}

// Several independent fused averages in ONE dispatch (co-resident learners of one round:
// LocalGroup).  Entry i owns the workgroups [begin[i], begin[i+1]); each workgroup runs the
// single-average span code for its entry, so the per-learner semantics (factor, clock commit by
// the entry's first workgroup, ragged tail) are those of k_lerp.  One launch instead of one per
// learner removes a ramp, a drain and a kernel boundary per extra learner.
template <class Ops, bool DUAL, int POLICY = 0, bool OOP = false>
__global__ __launch_bounds__(kStreamBlock) void k_lerp_batch(AvgBatch batch)
{
    int i = 0;
    uint32_t blk;
    if (batch.interleave == 2) {
        // XCD-grouped: workgroup b = (s / 8) * 8E + e * 8 + s % 8 takes span s of entry e, so every
        // entry's span s runs on XCD s % 8 (round-robin dispatch) within a few dispatch slots of the
        // others': entries that read the same buffer -- two resident learners that average with each
        // other both read both published slots -- fetch each span from HBM once, the later reads hit
        // that XCD's L2
        const uint32_t w = 8u * (uint32_t)batch.count;
        const uint32_t r = blockIdx.x % w;
        i = (int)(r >> 3);
        blk = (blockIdx.x / w) * 8u + (r & 7u);
        if (blk >= batch.spans) return;
    } else if (batch.interleave == 1) {
        // entries of equal size, their spans dealt round-robin: a span is read one round after
        // the span at the same position was written by the previous round's dispatch, whichever
        // entry wrote it, so every re-read is equally recent (Infinity Cache residency)
        i = (int)(blockIdx.x % (uint32_t)batch.count);
        blk = blockIdx.x / (uint32_t)batch.count;
    } else {
        // the entry of this workgroup: a short scalar scan over the uniform begin[] table
#pragma unroll
        for (int k = 1; k < kMaxAvgBatch; ++k)
            if (k < batch.count && blockIdx.x >= batch.begin[k]) i = k;
        blk = blockIdx.x - batch.begin[i];
    }
    const AvgEntry &e = batch.e[i];
    LerpArgs args{};
    args.fused = e.fa;
    args.snap = e.snap;
    lerp_span<Ops, COEF_FUSED, DUAL, kStreamBlock, POLICY, ContigSrc, OOP>(blk, (typename Ops::V *)e.param,
                                                                           ContigSrc{(const char *)e.peer}, e.n, args);
}

// A group of resident averages in one pass: co-resident learners whose reads overlap (a slot is
// one learner's parameters and another's peer snapshot, or two learners picked the same peer;
// the N=1 loop's two learners, each the other's only peer, are the mutual pair).  The dispatch's
// U distinct source buffers -- the entries' parameters, then peer snapshots that are no entry's
// parameters -- are loaded once per span by one workgroup, which stores every entry's average
// into its next slot: U loads and `count` stores per lane where the batched span code spends
// 2*count loads (the repeated ones served by L2 at best) over `count` workgroups, and one fp64
// factor evaluation per entry per workgroup as there.  Per entry exactly k_lerp_batch's span
// code: the factor and its commit by workgroup 0, the ZeroDivision no-op (the parameters stored
// unchanged), the ragged tail in workgroup 0.  Entries i < batch.count are src[i]'s averages.
template <class Ops, int POLICY, int U>
__device__ __forceinline__ void group_span(const AvgBatch &batch)
{
    using V = typename Ops::V;
    using S = typename Ops::S;
    using P = LerpPolicy<POLICY>;
    constexpr int SPAN = kStreamBlock * 16;
    const int G = batch.count;       // outputs (<= U), uniform
    const int64_t n = batch.e[0].n;
    const int64_t nv = n / Ops::PER;
    const uint32_t blk = blockIdx.x;
    const int64_t off = (int64_t)blk * SPAN;
    const int lane_off = threadIdx.x * 16;
    V v[U];
#pragma unroll
    for (int j = 0; j < U; ++j)   // all loads first
        v[j] = span_load<V, P::param_load>(span_rsrc<SPAN>(batch.src[j], off, nv * 16), lane_off);
    // per entry: its factor (and workgroup 0's commit), then its average -- one entry's factor
    // live at a time
    float fa_[U], fb_[U];
    bool ok_[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        if (i >= G) break;
        const dpwa_coef c = fused_factor(batch.e[i].fa, blk == 0 && threadIdx.x == 0);
        fa_[i] = c.a;
        fb_[i] = c.b;
        ok_[i] = c.status == DPWA_STATUS_OK;
        const int k = batch.peer_of[i];   // uniform: a select over registers, no indexed access
        V q = v[0];
#pragma unroll
        for (int j = 1; j < U; ++j)
            if (k == j) q = v[j];
        span_store<V, P::snap_store>(span_rsrc<SPAN>(batch.e[i].snap, off, nv * 16), lane_off,
                                     ok_[i] ? Ops::lerp(c.a, c.b, q, v[i]) : v[i]);
    }
    if (blk == 0 && threadIdx.x < n - nv * Ops::PER) {
        const int64_t j = nv * Ops::PER + threadIdx.x;
        S t[U];
#pragma unroll
        for (int m = 0; m < U; ++m) t[m] = reinterpret_cast<const S *>(batch.src[m])[j];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            if (i >= G) break;
            const int k = batch.peer_of[i];
            S q = t[0];
#pragma unroll
            for (int m = 1; m < U; ++m)
                if (k == m) q = t[m];
            reinterpret_cast<S *>(batch.e[i].snap)[j] = ok_[i] ? Ops::lerp_s(fa_[i], fb_[i], q, t[i]) : t[i];
        }
    }
}

// The mutual pair (two entries, two sources), the N=1 bench's kernel.
template <class Ops, int POLICY>
__global__ __launch_bounds__(kStreamBlock) void k_lerp_pair(AvgBatch batch)
{
    group_span<Ops, POLICY, 2>(batch);
}

// Groups of 3..8 source buffers.
template <class Ops, int POLICY, int U>
__global__ __launch_bounds__(kStreamBlock) void k_lerp_group(AvgBatch batch)
{
    group_span<Ops, POLICY, U>(batch);
}

// Element-wise path for pointers that are not 16-byte aligned (arbitrary views).
template <class Ops, int MODE, bool DUAL>
__global__ __launch_bounds__(kBlock) void k_lerp_unaligned(typename Ops::S *__restrict__ param,
                                                           const typename Ops::S *__restrict__ peer, int64_t n,
                                                           LerpArgs args)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    float a, b;
    if (!lerp_coef<MODE>(args, blockIdx.x == 0, a, b)) {   // every lane evaluates a fused factor
        if (MODE == COEF_FUSED && DUAL)
            for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
                reinterpret_cast<typename Ops::S *>(args.snap)[i] = param[i];
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const typename Ops::S r = Ops::lerp_s(a, b, peer[i], param[i]);
        param[i] = r;
        if (DUAL) reinterpret_cast<typename Ops::S *>(args.snap)[i] = r;
    }
}

static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// ---------------------------------------------------------------- tuning knobs
// Workgroup size of the averaging kernel; DPWA_LERP_BLOCK (64/128/256/512) forces another
// (tuning).
static int lerp_block()
{
    static const int block =
        env_knob("DPWA_LERP_BLOCK", kStreamBlock, [](const char *e) { return one_of(atoi(e), {64, 128, 256, 512}); });
    return block;
}

// The cache policy requested of a launch that averages `payload` bytes (policy.hpp: kFitPolicy
// while the parameters and two snapshot slots fit kCacheFitBytes, kProductPolicy above).  The
// single-learner and batched launches that are not resident, the tracked and the segmented
// launches ask with their bytes, and so does k_stream_mix, which is measured against them.
// DPWA_LERP_POLICY (0..31) forces one policy on every launch and DPWA_CACHE_FIT_BYTES moves the
// threshold (0: never fit) -- tuning and tests; what a requested value launches depends on the
// form, see the table below.
static int lerp_policy(int64_t payload)
{
    static const int forced = parse_lerp_policy(getenv("DPWA_LERP_POLICY"));
    static const int64_t fit_bytes = parse_cache_fit_bytes(getenv("DPWA_CACHE_FIT_BYTES"));
    return policy_for_bytes(forced, fit_bytes, payload);
}

// The resident, pair, group and relay kernels store into a slot that a peer reads next: the
// product policy whatever the size, unless DPWA_LERP_POLICY forces another.
static int lerp_policy() { return lerp_policy(INT64_MAX); }

// Span order of a batched dispatch of equal-size entries.  Dealt round-robin, every span is
// re-read by the next round's dispatch one round after it was written, which keeps the re-reads
// in the 256 MiB Infinity Cache while a round writes less than that; one entry after the other,
// half the re-reads come 1.5 rounds after their write.  Measured (profiles/r03_batch_order_ab.log,
// three interleaved pairs): round-robin +2.8 % at 11.17M fp32 (179 MB written per round), -4 %
// at 100M fp32 (1.6 GB: twice the concurrent streams, no cache to win).  DPWA_BATCH_ORDER=
// interleaved / contiguous forces one (1 / 0; -1: by size).  (kInfinityCacheBytes: policy.hpp)

static int batch_order()
{
    static const int order = env_knob("DPWA_BATCH_ORDER", -1, [](const char *e) {
        return strcmp(e, "contiguous") == 0 ? 0 : strcmp(e, "interleaved") == 0 ? 1 : kNoValue;
    });
    return order;
}

// (a switch that only "0" turns off)
static int off_when_0(const char *e) { return strcmp(e, "0") == 0 ? 0 : kNoValue; }

// XCD-grouped span order for resident batches whose entries share a read (k_lerp_batch);
// DPWA_BATCH_SHARE=0 turns it off (A/B runs).  tools/pair_tune.hip: two 11.17M fp32 resident
// learners averaging with each other, 36.8 -> 25-27 us per dispatch in the gossip loop, 41.3 ->
// 28.5 us cold (a fused one-workgroup form of both averages: 25.6 / 28.5).
static bool batch_share()
{
    static const bool on = env_knob("DPWA_BATCH_SHARE", 1, off_when_0) != 0;
    return on;
}

// A closed resident group runs as k_lerp_pair / k_lerp_group (one workgroup per span for all its
// averages); DPWA_PAIR_FUSED=0 keeps it on the XCD-grouped batch (A/B runs).
static bool pair_fused()
{
    static const bool on = env_knob("DPWA_PAIR_FUSED", 1, off_when_0) != 0;
    return on;
}

// ---------------------------------------------------------------- the policy table
// Which cache policy (LerpPolicy) each averaging form launches for a requested one
// (lerp_policy()): the listed values as themselves, every other value as the fallback, which
// comes first.  These are the instantiated kernels; the launchers below pick through these
// types, so the table is what runs.  Every table of a form that chooses by size lists both
// kFitPolicy and kProductPolicy.
using Lerp64Policies = Choice<0, 1, 2, 3, 4, 5, 8, 9, 10, 16>;   // k_lerp, 64 lanes, not resident
using LerpWidePolicies = Choice<0, 8>;                           // k_lerp, 128 / 256 / 512 lanes (tuning sizes)
// the resident kernels store only the next slot, so their store policy is the snapshot one: bit
// 16 makes it `nt`, bit 1 loads the parameters with the default policy
using ResidentPolicies = Choice<kProductPolicy, 0, 1, 2, 16, 17>;   // k_lerp and k_lerp_batch, resident (OOP)
using BatchPolicies = Choice<0, 1, 2, 8, 9, 10, 16>;                // k_lerp_batch, not resident
// the pair's two loads both take the parameter load's policy (each slot is one entry's parameters
// and the other's peer)
using PairF32Policies = Choice<kProductPolicy, 0, 1, 2, 16>;   // k_lerp_pair, float32
using Pair16Policies = Choice<kProductPolicy, 0>;              // k_lerp_pair, bfloat16 / float16
using GroupPolicies = Choice<kProductPolicy, 0>;               // k_lerp_group
using RelayPolicies = Choice<0, 8>;                            // k_lerp_relay
// k_lerp_tracked and k_lerp_mixed (not resident), k_stream_mix: the two policies the size chooses between
using BySizePolicies = Choice<kProductPolicy, kFitPolicy>;

template <class Policies, int... Ps> constexpr bool launches_as_itself() { return ((Policies::launched(Ps) == Ps) && ...); }
static_assert(launches_as_itself<Lerp64Policies, 1, 2, 3, 4, 5, 8, 9, 10, 16>() && Lerp64Policies::launched(6) == 0);
static_assert(launches_as_itself<LerpWidePolicies, 8>() && LerpWidePolicies::launched(1) == 0);
static_assert(launches_as_itself<ResidentPolicies, 0, 1, 2, 16, 17>() && ResidentPolicies::launched(9) == 8 &&
              ResidentPolicies::launched(8) == 8);
static_assert(launches_as_itself<BatchPolicies, 1, 2, 8, 9, 10, 16>() && BatchPolicies::launched(3) == 0);
static_assert(launches_as_itself<PairF32Policies, 0, 1, 2, 16>() && PairF32Policies::launched(17) == 8 &&
              PairF32Policies::launched(8) == 8);
static_assert(launches_as_itself<Pair16Policies, 0>() && Pair16Policies::launched(1) == 8 && Pair16Policies::launched(8) == 8);
static_assert(launches_as_itself<GroupPolicies, 0>() && GroupPolicies::launched(16) == 8 && GroupPolicies::launched(8) == 8);
static_assert(launches_as_itself<RelayPolicies, 8>() && RelayPolicies::launched(9) == 0);
static_assert(launches_as_itself<BySizePolicies, kFitPolicy, kProductPolicy>() && BySizePolicies::launched(16) == 8);
static_assert(launches_as_itself<Lerp64Policies, kFitPolicy, kProductPolicy>() &&
              launches_as_itself<BatchPolicies, kFitPolicy, kProductPolicy>());

// ---------------------------------------------------------------- averaging launches
// Workgroups of one 16-byte item per lane over n elements; the last span may be empty
// (range-checked).
template <class Ops> static int64_t span_grid(int64_t n, int block) { return (n / Ops::PER) / block + 1; }
// Workgroups of the grid-stride kernels for operands that are not 16-B aligned.
static dim3 unaligned_grid(int64_t n) { return dim3((uint32_t)std::min<int64_t>(blocks_for(n), 8192)); }

template <class Ops, int MODE, bool DUAL>
static hipError_t launch_mode(void *param, const void *peer, int64_t n, const LerpArgs &args, hipStream_t s,
                              const LaunchTiming *timing)
{
    if (!aligned16(param) || !aligned16(peer) || !aligned16(args.snap)) {
        // (callers time only the aligned product kernel; an unaligned launch is not timed)
        return launch(k_lerp_unaligned<Ops, MODE, DUAL>, unaligned_grid(n), dim3(kBlock), s, nullptr, param, peer, n, args);
    }
    return Choice<256, 64, 128, 512>::with(lerp_block(), [&](auto block) {
        constexpr int BLOCK = decltype(block)::value;
        using Policies = std::conditional_t<BLOCK == 64, Lerp64Policies, LerpWidePolicies>;
        return Policies::with(lerp_policy(n * (int64_t)sizeof(typename Ops::S)), [&](auto policy) {
            return launch(k_lerp<Ops, MODE, DUAL, BLOCK, decltype(policy)::value>, dim3((uint32_t)span_grid<Ops>(n, BLOCK)),
                          dim3(BLOCK), s, timing, param, peer, n, args);
        });
    });
}

// (a segmented payload's k_lerp_mixed launches, behind with_segments below)
static hipError_t launch_any_mixed(const Elems &e, int mode, bool oop, void *param, const void *peer, const LerpArgs &args,
                                   hipStream_t s, const LaunchTiming *t);

static hipError_t launch_any(const Elems &e, int mode, void *param, const void *peer, const LerpArgs &args, hipStream_t s,
                             const LaunchTiming *t = nullptr)
{
    if (e.segmented()) return launch_any_mixed(e, mode, false, param, peer, args, s, t);
    const int64_t n = e.n;
    if (n < 0) return hipErrorInvalidValue;
    if (n == 0 && mode != COEF_FUSED) return hipSuccess;
    return with_ops(e.dtype, [&](auto ops) {
        using Ops = decltype(ops);
        if (mode == COEF_HOST) return launch_mode<Ops, COEF_HOST, false>(param, peer, n, args, s, t);
        if (mode == COEF_DEV) return launch_mode<Ops, COEF_DEV, false>(param, peer, n, args, s, t);
        if (args.snap) return launch_mode<Ops, COEF_FUSED, true>(param, peer, n, args, s, t);
        return launch_mode<Ops, COEF_FUSED, false>(param, peer, n, args, s, t);
    });
}

hipError_t launch_lerp(const Elems &e, void *param, const void *peer, const dpwa_coef *coef, float a, float b,
                       hipStream_t s)
{
    LerpArgs args{};
    args.a = a;
    args.b = b;
    args.coef = coef;
    return launch_any(e, coef ? COEF_DEV : COEF_HOST, param, peer, args, s);
}

hipError_t launch_average(const Elems &e, void *param, const void *peer, const FusedArgs &fa, void *snap, hipStream_t s,
                          const LaunchTiming *timing, bool oop)
{
    LerpArgs args{};
    args.fused = fa;
    args.snap = snap;
    if (!oop) return launch_any(e, COEF_FUSED, param, peer, args, s, timing);
    if (e.segmented()) return launch_any_mixed(e, COEF_FUSED, true, param, peer, args, s, timing);
    // resident: 16-B aligned slot payloads only, one-wave workgroups
    const int64_t n = e.n;
    if (n < 0 || (!snap && n > 0) || !aligned16(param) || !aligned16(peer) || !aligned16(snap)) return hipErrorInvalidValue;
    return with_ops(e.dtype, [&](auto ops) {
        using Ops = decltype(ops);
        return ResidentPolicies::with(lerp_policy(), [&](auto policy) {
            return launch(k_lerp<Ops, COEF_FUSED, true, kStreamBlock, decltype(policy)::value, true>,
                          dim3((uint32_t)span_grid<Ops>(n, kStreamBlock)), dim3(kStreamBlock), s, timing, param, peer, n, args);
        });
    });
}

const char *layout_problem(const dpwa_layout &layout, int64_t total_bytes)
{
    if (layout.count < 1) return "no segment";
    if (layout.count > DPWA_LAYOUT_MAX_SEGMENTS) return "more than three segments";
    int64_t end = 0;
    for (int i = 0; i < layout.count; ++i) {
        const dpwa_segment &g = layout.seg[i];
        if (g.dtype != DPWA_F32 && g.dtype != DPWA_BF16 && g.dtype != DPWA_F16)
            return "a segment's dtype is not DPWA_F32, DPWA_BF16 or DPWA_F16";
        for (int j = 0; j < i; ++j)
            if (layout.seg[j].dtype == g.dtype) return "a dtype is repeated";
        if (g.byte_offset < 0 || g.byte_offset % DPWA_LAYOUT_ALIGN) return "a segment does not begin on a 4096-byte boundary";
        if (g.byte_length <= 0 || g.byte_length % DPWA_LAYOUT_ALIGN)
            return "a segment's length is not a positive multiple of 4096 bytes";
        if (g.byte_offset < end) return "segments overlap or are out of order";
        if (g.byte_offset > end) return i ? "a hole between two segments" : "the first segment does not begin at byte 0";
        if (g.byte_length > INT64_MAX - end) return "the segments' total overflows";
        end += g.byte_length;
    }
    if (total_bytes >= 0 && end != total_bytes) return "the segments do not cover the payload's bytes exactly";
    return nullptr;
}

// The launch of a segmented payload, one 1-KiB span per workgroup: run(total bytes, grid, the segments' table).
// Refused: `operands_bad` (the caller's null or misaligned pointers), no layout, an invalid one, too many spans.
template <class Run> static hipError_t with_segments(const Elems &e, bool operands_bad, Run &&run)
{
    if (operands_bad || !e.layout || layout_problem(*e.layout, -1)) return hipErrorInvalidValue;
    const dpwa_layout &layout = *e.layout;
    SegTable t;
    for (int i = 0; i < DPWA_LAYOUT_MAX_SEGMENTS; ++i) {
        t.begin[i] = i < layout.count ? layout.seg[i].byte_offset : INT64_MAX;
        t.dtype[i] = i < layout.count ? layout.seg[i].dtype : layout.seg[0].dtype;
    }
    const int64_t total = layout_bytes(layout);
    const int64_t g = total / (kStreamBlock * 16);   // exact: whole 4-KiB segments
    if (g > 0x7fffffffLL) return hipErrorInvalidValue;
    return run(total, dim3((uint32_t)g), t);
}
// (a segmented payload's operand: there, and 16-B aligned)
static bool absent_or_unaligned(const void *p) { return !p || !aligned16(p); }

template <int MODE, bool DUAL, bool OOP>
static hipError_t launch_mixed(const Elems &e, void *param, const void *peer, const LerpArgs &args, hipStream_t s,
                               const LaunchTiming *timing)
{
    const bool bad = absent_or_unaligned(param) || absent_or_unaligned(peer) || !aligned16(args.snap) || (DUAL && !args.snap);
    return with_segments(e, bad, [&](int64_t total, dim3 grid, const SegTable &t) {
        // (resident: the product policy, as the single-dtype resident kernels without the knob)
        return BySizePolicies::with(OOP ? kProductPolicy : lerp_policy(total), [&](auto policy) {
            constexpr int P = OOP ? kProductPolicy : decltype(policy)::value;
            return launch(k_lerp_mixed<MODE, DUAL, P, OOP>, grid, dim3(kStreamBlock), s, timing, param, peer, total, args, t);
        });
    });
}

static hipError_t launch_any_mixed(const Elems &e, int mode, bool oop, void *param, const void *peer, const LerpArgs &args,
                                   hipStream_t s, const LaunchTiming *t)
{
    if (mode == COEF_HOST) return hipErrorInvalidValue;   // (a segmented lerp reads its coefficients on the device)
    if (mode == COEF_DEV) return launch_mixed<COEF_DEV, false, false>(e, param, peer, args, s, t);
    if (oop) return launch_mixed<COEF_FUSED, true, true>(e, param, peer, args, s, t);
    if (args.snap) return launch_mixed<COEF_FUSED, true, false>(e, param, peer, args, s, t);
    return launch_mixed<COEF_FUSED, false, false>(e, param, peer, args, s, t);
}

// ---------------------------------------------------------------- distance launches
hipError_t launch_average_tracked(int32_t dtype, void *param, const void *peer, int64_t n, const FusedArgs &fa,
                                  void *snap, bool oop, double *acc, hipStream_t s, const LaunchTiming *timing)
{
    if (n < 0 || !acc || (oop && !snap && n > 0) || !aligned16(param) || !aligned16(peer) || !aligned16(snap))
        return hipErrorInvalidValue;
    LerpArgs args{};
    args.fused = fa;
    args.snap = snap;
    return with_ops(dtype, [&](auto ops) {
        using Ops = decltype(ops);
        using V = typename Ops::V;
        if (span_grid<Ops>(n, kStreamBlock) > 0x7fffffffLL) return hipErrorInvalidValue;
        const auto run = [&](void (*kernel)(V *, const V *, int64_t, LerpArgs, double *)) {
            return launch(kernel, dim3((uint32_t)span_grid<Ops>(n, kStreamBlock)), dim3(kStreamBlock), s, timing, param,
                          peer, n, args, acc);
        };
        if (oop) return run(k_lerp_tracked<Ops, true, true, kProductPolicy>);   // resident: no choice by size
        return BySizePolicies::with(lerp_policy(n * (int64_t)sizeof(typename Ops::S)), [&](auto policy) {
            constexpr int P = decltype(policy)::value;
            return snap ? run(k_lerp_tracked<Ops, true, false, P>) : run(k_lerp_tracked<Ops, false, false, P>);
        });
    });
}

hipError_t launch_distance(const Elems &e, const void *param, const void *peer, double *acc, hipStream_t s)
{
    if (!acc) return hipErrorInvalidValue;
    if (const int64_t n = e.n; !e.segmented()) {
        if (n <= 0) return n < 0 ? hipErrorInvalidValue : hipSuccess;
        return with_ops(e.dtype, [&](auto ops) {
            using Ops = decltype(ops);
            if (!aligned16(param) || !aligned16(peer))
                return launch(k_distance_unaligned<Ops>, unaligned_grid(n), dim3(kBlock), s, nullptr, param, peer, n, acc);
            if (span_grid<Ops>(n, kStreamBlock) > 0x7fffffffLL) return hipErrorInvalidValue;
            return launch(k_distance<Ops>, dim3((uint32_t)span_grid<Ops>(n, kStreamBlock)), dim3(kStreamBlock), s, nullptr,
                          param, peer, n, acc);
        });
    }
    const bool bad = absent_or_unaligned(param) || absent_or_unaligned(peer);
    return with_segments(e, bad, [&](int64_t total, dim3 grid, const SegTable &t) {
        return launch(k_distance_mixed, grid, dim3(kStreamBlock), s, nullptr, param, peer, total, t, acc);
    });
}

hipError_t launch_distance_finish(double *acc, dpwa_distance *out, const dpwa_coef *coef, int64_t n, hipStream_t s,
                                  const LaunchTiming *timing)
{
    if (!acc || !out) return hipErrorInvalidValue;
    return launch(k_distance_finish, dim3(1), dim3(kDistFinishBlock), s, timing, acc, out, coef, n);
}

hipError_t launch_param_distance(const void *param, const void *peer, int64_t total, const ParamEntry *table,
                                 int64_t count, double *acc, hipStream_t s, const LaunchTiming *timing)
{
    if (total < 0 || count < 1 || count > 0x7fffffffLL || !table || !acc || !aligned16(param) || !aligned16(peer))
        return hipErrorInvalidValue;
    const int64_t g = (total + kStreamBlock * 16 - 1) / (kStreamBlock * 16);
    if (g > 0x7fffffffLL) return hipErrorInvalidValue;
    if (g == 0) return hipSuccess;
    return launch(k_param_distance, dim3((uint32_t)g), dim3(kStreamBlock), s, timing, param, peer, total, table,
                  (int)count, acc);
}

hipError_t launch_param_distance_finish(double *acc, const ParamEntry *table, int64_t count,
                                        dpwa_param_distance_head *out, const dpwa_coef *coef, hipStream_t s,
                                        const LaunchTiming *timing)
{
    if (count < 1 || count > 0x7fffffffLL || !table || !acc || !out) return hipErrorInvalidValue;
    return launch(k_param_distance_finish, dim3((uint32_t)count), dim3(kParamFinishBlock), s, timing, acc, table, out, coef,
                  count);
}

// ---------------------------------------------------------------- non-finite peer check launches
// The load policy of the pass: the default one at every size.  The rule by size of policy.hpp (`nt`
// above kCacheFitBytes) was the starting point and lost on both sides of the threshold, pass +
// average together, fresh processes taking turns (profiles/finite_cost.json): 11,173,962 fp32
// 27.1-27.4 us against `nt` 27.4-27.5 (the pass itself 9.92 against 10.16); 100M fp32, the snapshot
// from HBM, 249.3-252.8 us against 262.6-272.7 -- the pass takes 83.2 us either way, the average
// behind it 166-169 us against 179-189: what the default loads leave in the Infinity Cache, it
// reads there.  DPWA_FINITE_LOADS=nt / default forces one (tools/finite_cost.py's A/B).
static int finite_aux()
{
    static const int aux = env_knob("DPWA_FINITE_LOADS", 0, [](const char *e) {
        return strcmp(e, "default") == 0 ? 0 : strcmp(e, "nt") == 0 ? kAuxStream : kNoValue;
    });
    return aux;
}
using FiniteLoads = Choice<0, kAuxStream>;

hipError_t launch_peer_finite(const Elems &e, const void *peer, uint32_t *veto, uint32_t stamp, hipStream_t s,
                              const LaunchTiming *timing)
{
    if (!veto || stamp == 0 || ((uintptr_t)veto & 3)) return hipErrorInvalidValue;
    if (const int64_t n = e.n; !e.segmented()) {
        if (n <= 0) return n < 0 ? hipErrorInvalidValue : hipSuccess;
        return with_ops(e.dtype, [&](auto ops) {
            using Ops = decltype(ops);
            if (!aligned16(peer))
                return launch(k_peer_finite_unaligned<Ops>, unaligned_grid(n), dim3(kBlock), s, timing, peer, n, veto, stamp);
            if (span_grid<Ops>(n, kStreamBlock) > 0x7fffffffLL) return hipErrorInvalidValue;
            return FiniteLoads::with(finite_aux(), [&](auto aux) {
                return launch(k_peer_finite<Ops, decltype(aux)::value>, dim3((uint32_t)span_grid<Ops>(n, kStreamBlock)),
                              dim3(kStreamBlock), s, timing, peer, n, veto, stamp);
            });
        });
    }
    return with_segments(e, absent_or_unaligned(peer), [&](int64_t total, dim3 grid, const SegTable &t) {
        return FiniteLoads::with(finite_aux(), [&](auto aux) {
            return launch(k_peer_finite_mixed<decltype(aux)::value>, grid, dim3(kStreamBlock), s, timing, peer, total, t, veto,
                          stamp);
        });
    });
}

// Some buffer is read by two entries (as parameters or as the peer snapshot).
static bool shares_a_read(const AvgBatch &x)
{
    for (int i = 0; i < x.count; ++i)
        for (int j = 0; j < x.count; ++j)
            if (i != j && (x.e[i].peer == x.e[j].param || (j > i && x.e[i].peer == x.e[j].peer)))
                return true;
    return false;
}

template <class Ops>
static hipError_t average_batch(bool dual, const AvgBatch &b, hipStream_t s, const LaunchTiming *timing, bool oop)
{
    AvgBatch x = b;
    for (int i = 0; i < x.count; ++i) {
        const AvgEntry &e = x.e[i];
        if (e.n < 0 || !aligned16(e.param) || !aligned16(e.peer) || (!dual && e.snap) || (dual && !e.snap && e.n > 0) ||
            !aligned16(e.snap))
            return hipErrorInvalidValue;
        if (span_grid<Ops>(e.n, kStreamBlock) > 0x7fffffffLL) return hipErrorInvalidValue;
    }
    int64_t total = 0;   // in 64 bits: up to 8 entries of up to 2^31 - 1 workgroups each
    for (int i = 0; i < x.count; ++i) {
        x.begin[i] = (uint32_t)total;
        total += span_grid<Ops>(x.e[i].n, kStreamBlock);
        if (total > 0x7fffffffLL) return hipErrorInvalidValue;
    }
    uint32_t g = (uint32_t)total;
    for (int i = x.count; i < kMaxAvgBatch; ++i) x.begin[i] = 0xffffffffu;
    // span order: see batch_order()
    bool same = true;
    size_t written = 0;
    for (int i = 0; i < x.count; ++i) {
        same = same && x.e[i].n == x.e[0].n;
        written += (size_t)x.e[i].n * sizeof(typename Ops::S) * (dual && !oop ? 2 : 1);
    }
    const int order = batch_order();
    x.interleave = same && x.count > 1 && (order == 1 || (order < 0 && written <= kInfinityCacheBytes)) ? 1 : 0;
    // resident entries of equal size that read a common buffer (a learner's published slot is its
    // own parameters and another's peer): XCD-grouped, whatever the size (nothing writes what they
    // read, so any order is safe)
    x.spans = (uint32_t)span_grid<Ops>(x.e[0].n, kStreamBlock);
    // a group: entries of equal size, distinct parameters, whose reads overlap; its sources are
    // the parameters, then the peers that are no entry's parameters (at most kMaxAvgBatch)
    bool grouped = oop && same && x.count > 1 && order < 0 && batch_share() && pair_fused();
    int nsrc = x.count;
    for (int i = 0; grouped && i < x.count; ++i) {
        x.src[i] = x.e[i].param;
        for (int j = 0; j < i; ++j)
            if (x.e[j].param == x.e[i].param) grouped = false;
    }
    for (int i = 0; grouped && i < x.count; ++i) {
        int k = -1;
        for (int j = 0; j < nsrc && k < 0; ++j)
            if (x.src[j] == x.e[i].peer) k = j;
        if (k < 0) {
            if (nsrc == kMaxAvgBatch) grouped = false;
            else {
                k = nsrc;
                x.src[nsrc++] = x.e[i].peer;
            }
        }
        x.peer_of[i] = (int8_t)k;
        grouped = grouped && k != i;
    }
    grouped = grouped && nsrc < 2 * x.count;   // some read is shared
    for (int j = nsrc; j < kMaxAvgBatch; ++j) x.src[j] = nullptr;
    const auto run = [&](void (*kernel)(AvgBatch), uint32_t grid) {
        return launch(kernel, dim3(grid), dim3(kStreamBlock), s, timing, x);
    };
    if (grouped && nsrc == 2 && x.count == 2) {   // the mutual pair: both averages in one workgroup per span
        using Policies = std::conditional_t<std::is_same_v<Ops, OpsF32>, PairF32Policies, Pair16Policies>;
        return Policies::with(lerp_policy(), [&](auto policy) { return run(k_lerp_pair<Ops, decltype(policy)::value>, x.spans); });
    }
    if (grouped) {   // 3..8 source buffers
        return GroupPolicies::with(lerp_policy(), [&](auto policy) {
            return Choice<8, 3, 4, 5, 6, 7>::with(nsrc, [&](auto u) {
                return run(k_lerp_group<Ops, decltype(policy)::value, decltype(u)::value>, x.spans);
            });
        });
    }
    if (oop && same && x.count > 1 && order < 0 && batch_share() && shares_a_read(x)) {
        const uint64_t gg = (uint64_t)(x.spans + 7) / 8 * 8 * (uint64_t)x.count;
        if (gg > 0x7fffffffu) return hipErrorInvalidValue;
        x.interleave = 2;
        g = (uint32_t)gg;
    }
    if (oop)
        return ResidentPolicies::with(lerp_policy(), [&](auto policy) {
            return run(k_lerp_batch<Ops, true, decltype(policy)::value, true>, g);
        });
    int64_t numel[kMaxAvgBatch];
    for (int i = 0; i < x.count; ++i) numel[i] = x.e[i].n;
    return BatchPolicies::with(lerp_policy(payload_bytes(numel, x.count, sizeof(typename Ops::S))), [&](auto policy) {
        constexpr int P = decltype(policy)::value;
        return dual ? run(k_lerp_batch<Ops, true, P, false>, g) : run(k_lerp_batch<Ops, false, P, false>, g);
    });
}

hipError_t launch_average_batch(int32_t dtype, bool dual, const AvgBatch &b, hipStream_t s,
                                 const LaunchTiming *timing, bool oop)
{
    if (b.count < 1 || b.count > kMaxAvgBatch || (oop && !dual)) return hipErrorInvalidValue;
    return with_ops(dtype, [&](auto ops) { return average_batch<decltype(ops)>(dual, b, s, timing, oop); });
}

__global__ void k_acquire_system();

hipError_t launch_average_relay(int32_t dtype, void *param, int64_t n, const FusedArgs &fa, void *snap,
                                const RelayArgs &a, int my_pick, hipStream_t s, const LaunchTiming *timing, bool oop)
{
    if (n < 0 || a.world < 1 || a.world > kMaxRelayRanks || my_pick < 0 || my_pick >= a.world ||
        my_pick == a.rank || a.stripe <= 0 || a.stripe % (kStreamBlock * 16) || !aligned16(param) ||
        (snap && !aligned16(snap)) || (oop && !snap))
        return hipErrorInvalidValue;
    const int j = my_pick;
    StripeSrc src;
    for (int r = 0; r < a.world; ++r)   // where stripe r of j's snapshot is (k_relay_phase2's sources)
        src.src[r] = r == j        ? a.slots[j] + a.slot_off + DPWA_SLOT_PAYLOAD_OFFSET + (int64_t)r * a.stripe
                     : r == a.rank ? a.relay_mine + (int64_t)j * a.stripe
                                   : a.relays[r] + (int64_t)j * a.stripe;
    for (int r = a.world; r < kMaxRelayRanks; ++r) src.src[r] = nullptr;
    src.stripe = a.stripe;
    src.parts = a.world;
    LerpArgs args{};
    args.fused = fa;
    args.snap = snap;
    hipLaunchKernelGGL(k_acquire_system, dim3(256), dim3(64), 0, s);   // remote lines in L2 are stale
    // every span of every stripe (the spans past the payload are range-checked away)
    const dim3 grid((uint32_t)((int64_t)src.parts * (src.stripe / (kStreamBlock * 16))));
    return with_ops(dtype, [&](auto ops) {
        using Ops = decltype(ops);
        return RelayPolicies::with(lerp_policy(), [&](auto policy) {
            constexpr int P = decltype(policy)::value;
            const auto run = [&](void (*kernel)(typename Ops::V *, int64_t, LerpArgs, StripeSrc)) {
                return launch(kernel, grid, dim3(kStreamBlock), s, timing, param, n, args, src);
            };
            return oop ? run(k_lerp_relay<Ops, true, P, true>) : snap ? run(k_lerp_relay<Ops, true, P>) : run(k_lerp_relay<Ops, false, P>);
        });
    });
}

// ---------------------------------------------------------------- publish
// This workgroup's span of a streaming copy: one 16-B item per lane with the streaming policy of
// the lerp (nt loads, sc1 stores); the bytes past the last whole item go to workgroup 0.
template <int BLOCK>
__device__ __forceinline__ void copy_span(char *__restrict__ dst, const char *__restrict__ src, int64_t nbytes)
{
    constexpr int SPAN = BLOCK * 16;
    const int64_t n16 = nbytes >> 4;
    const int64_t span_off = (int64_t)blockIdx.x * SPAN;
    const int lane_off = threadIdx.x * 16;
    span_store(span_rsrc<SPAN>(dst, span_off, n16 * 16), lane_off,
               span_load<u32x4>(span_rsrc<SPAN>(src, span_off, n16 * 16), lane_off));
    if (blockIdx.x == 0 && threadIdx.x < (nbytes & 15)) {
        const int64_t j = (n16 << 4) + threadIdx.x;
        dst[j] = src[j];
    }
}

template <bool VEC, int BLOCK = kBlock>
__global__ __launch_bounds__(BLOCK) void k_publish(char *__restrict__ slot, const char *__restrict__ flat,
                                                   int64_t nbytes, int64_t n, int32_t dtype,
                                                   double *__restrict__ clock, double loss_h,
                                                   const double *__restrict__ loss_d, int32_t loss_f32,
                                                   uint64_t version)
{
    char *payload = slot + DPWA_SLOT_PAYLOAD_OFFSET;
    if (VEC) {
        copy_span<BLOCK>(payload, flat, nbytes);
    } else {
        const int64_t stride = (int64_t)gridDim.x * kBlock;
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nbytes; i += stride) payload[i] = flat[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        dpwa_header *h = reinterpret_cast<dpwa_header *>(slot);
        const double c = *clock + 1.0;                 // dpwa.py:112  self.clock += 1
        *clock = c;
        h->clock = c;                                  // dpwa.py:115  state = {'clock', 'loss'}
        h->loss = read_loss(loss_d, loss_f32, loss_h);
        h->version = version;
        h->n = n;
        h->dtype = dtype;
    }
}

// Local streaming copy of a payload (a resident learner's relocation: the parameters leave the
// published slot for the next one), the publish's span shape without the header.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_copy_payload(char *__restrict__ dst, const char *__restrict__ src,
                                                        int64_t nbytes)
{
    copy_span<BLOCK>(dst, src, nbytes);
}

hipError_t launch_copy_payload(void *dst, const void *src, int64_t nbytes, hipStream_t s)
{
    if (nbytes <= 0) return hipSuccess;
    if (!aligned16(dst) || !aligned16(src))
        return hipMemcpyAsync(dst, src, (size_t)nbytes, hipMemcpyDeviceToDevice, s);
    const int64_t g = (nbytes >> 4) / kStreamBlock + 1;
    if (g > 0x7fffffffLL) return hipMemcpyAsync(dst, src, (size_t)nbytes, hipMemcpyDeviceToDevice, s);
    hipLaunchKernelGGL(k_copy_payload<kStreamBlock>, dim3((uint32_t)g), dim3(kStreamBlock), 0, s, (char *)dst,
                       (const char *)src, nbytes);
    return hipGetLastError();
}

// 16-byte words first, first + stride, ... below n16, four loads in flight per lane.
__device__ __forceinline__ void copy16(u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, int64_t n16,
                                       int64_t first, int64_t stride)
{
    int64_t i = first;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        u32x4 v0 = src[i], v1 = src[i + stride], v2 = src[i + 2 * stride], v3 = src[i + 3 * stride];
        dst[i] = v0;
        dst[i + stride] = v1;
        dst[i + 2 * stride] = v2;
        dst[i + 3 * stride] = v3;
    }
    for (; i < n16; i += stride) dst[i] = src[i];
}

// Pull: copy a peer's snapshot (header + payload, IPC-mapped in another GPU's HBM) into the
// local staging buffer.  The loads travel over the xGMI link to the owner; each lane keeps
// four 16-byte loads in flight and the grid is capped (grid-stride) so the pull occupies a
// bounded share of the CUs while the training step runs on the compute stream.
__global__ __launch_bounds__(kBlock) void k_pull(u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, int64_t n16)
{
    copy16(dst, src, n16, (int64_t)blockIdx.x * kBlock + threadIdx.x, (int64_t)gridDim.x * kBlock);
}

// Invalidates every XCD's L2 lines of other agents' memory (system-scope acquire from 256
// workgroups, dealt round-robin over the 8 XCDs) ahead of a kernel that reads peer memory.
__global__ __launch_bounds__(64) void k_acquire_system()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
}

hipError_t launch_pull(void *dst, const void *src, int64_t nbytes, int max_blocks, bool remote, hipStream_t s)
{
    if (((uintptr_t)dst | (uintptr_t)src | (uintptr_t)nbytes) & 15) return hipErrorInvalidValue;
    if (remote) hipLaunchKernelGGL(k_acquire_system, dim3(256), dim3(64), 0, s);
    const int64_t n16 = nbytes >> 4;
    int64_t g = (n16 + kBlock * 4 - 1) / (kBlock * 4);
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    hipLaunchKernelGGL(k_pull, dim3((uint32_t)g), dim3(kBlock), 0, s, (u32x4 *)dst, (const u32x4 *)src, n16);
    return hipGetLastError();
}

// ---------------------------------------------------------------- relay (multi-link pull)
// Lock-step round of G ranks where rank i averages with rank picks[i] (-1: none).  Each
// snapshot payload is cut into G stripes.  Phase 1 on rank r pulls stripe r of every
// snapshot some rank needs (its own peer's included) into its relay buffer (R_r[j] = stripe
// r of rank j); after a barrier, phase 2 on rank r gathers stripe s of its peer j's snapshot
// from rank s's relay buffer, from its own relay buffer for s == r (local HBM) and from j
// itself for s == j.  Every pair's xGMI link then carries at most one stripe per phase
// instead of one link carrying the whole snapshot.
// blockIdx.x selects the source (phase 1) or the stripe (phase 2) and blockIdx.y strides it:
// consecutive workgroups (the dispatch order) take different sources, so every link is busy
// from the start even when the grid exceeds what is resident at once.
__global__ void k_release_system();

// A relay copy: this workgroup's share (blockIdx.y of gridDim.y) of n16 words.
__device__ __forceinline__ void relay_copy(u32x4 *__restrict__ dst, const u32x4 *__restrict__ src, int64_t n16)
{
    copy16(dst, src, n16, (int64_t)blockIdx.y * kBlock + threadIdx.x, (int64_t)gridDim.y * kBlock);
}

__device__ __forceinline__ int64_t stripe_len(int s, int64_t stripe, int64_t payload)
{
    const int64_t beg = (int64_t)s * stripe;
    if (beg >= payload) return 0;
    return (payload - beg < stripe ? payload - beg : stripe);
}

__global__ __launch_bounds__(kBlock) void k_relay_phase1(RelayArgs a)
{
    const int j = blockIdx.x;
    if (j == a.rank) return;
    bool active = false;                                   // does any rank (me included) need j?
    for (int i = 0; i < a.world; ++i) active |= (a.picks[i] == j);
    if (!active) return;
    const int64_t len = stripe_len(a.rank, a.stripe, a.payload);
    const char *src = a.slots[j] + a.slot_off + DPWA_SLOT_PAYLOAD_OFFSET + (int64_t)a.rank * a.stripe;
    char *dst = a.relay_mine + (int64_t)j * a.stripe;
    relay_copy((u32x4 *)dst, (const u32x4 *)src, len >> 4);
}

__global__ __launch_bounds__(kBlock) void k_relay_phase2(RelayArgs a)
{
    const int j = a.picks[a.rank];
    if (j < 0) return;
    const int s = blockIdx.x;
    if (s == 0 && blockIdx.y == 0 && threadIdx.x < 16)     // the 256-B header, straight from j
        reinterpret_cast<u32x4 *>(a.staging)[threadIdx.x] =
            reinterpret_cast<const u32x4 *>(a.slots[j] + a.slot_off)[threadIdx.x];
    const int64_t len = stripe_len(s, a.stripe, a.payload);
    const char *src = s == j        ? a.slots[j] + a.slot_off + DPWA_SLOT_PAYLOAD_OFFSET + (int64_t)s * a.stripe
                      : s == a.rank ? a.relay_mine + (int64_t)j * a.stripe
                                    : a.relays[s] + (int64_t)j * a.stripe;
    relay_copy((u32x4 *)(a.staging + DPWA_SLOT_PAYLOAD_OFFSET + (int64_t)s * a.stripe), (const u32x4 *)src, len >> 4);
}

hipError_t launch_relay(int phase, const RelayArgs &a, int blocks_per_part, hipStream_t s)
{
    if (a.world < 1 || a.world > kMaxRelayRanks || (a.stripe & 15) || (a.payload & 15)) return hipErrorInvalidValue;
    dim3 grid((uint32_t)a.world, (uint32_t)blocks_per_part);
    hipLaunchKernelGGL(k_acquire_system, dim3(256), dim3(64), 0, s);   // both phases read peers
    if (phase == 1) {   // the relay buffer is read by other GPUs: write it back from the L2s
        hipLaunchKernelGGL(k_relay_phase1, grid, dim3(kBlock), 0, s, a);
        hipLaunchKernelGGL(k_release_system, dim3(256), dim3(64), 0, s);
    } else {
        hipLaunchKernelGGL(k_relay_phase2, grid, dim3(kBlock), 0, s, a);
    }
    return hipGetLastError();
}

// Writes back every XCD's L2 (system-scope release from 256 workgroups, which the
// dispatcher deals round-robin over the 8 XCDs) so a snapshot that another GPU will pull
// is in HBM, not only in this GPU's L2s.  Used only once the slots are IPC-exported.
__global__ __launch_bounds__(64) void k_release_system()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
}

hipError_t launch_release_system(hipStream_t s)
{
    hipLaunchKernelGGL(k_release_system, dim3(256), dim3(64), 0, s);
    return hipGetLastError();
}

// Workgroup size of the snapshot copy; DPWA_PUBLISH_BLOCK (64/128/256) forces another.
static int publish_block()
{
    static const int block =
        env_knob("DPWA_PUBLISH_BLOCK", kStreamBlock, [](const char *e) { return one_of(atoi(e), {64, 128, 256}); });
    return block;
}

hipError_t launch_publish(char *slot, const void *flat, int64_t nbytes, int64_t n, int32_t dtype, double *clock,
                          double loss, const double *loss_dev, bool loss_f32, uint64_t version, bool system_release,
                          hipStream_t s)
{
    const auto run = [&](auto kernel, int64_t grid, int block) {
        return launch(kernel, dim3((uint32_t)grid), dim3(block), s, nullptr, slot, flat, nbytes, n, dtype, clock, loss,
                      loss_dev, loss_f32, version);
    };
    hipError_t err = aligned16(flat) ? Choice<kBlock, 64, 128>::with(publish_block(), [&](auto block) {
        constexpr int BLOCK = decltype(block)::value;
        return run(k_publish<true, BLOCK>, (nbytes >> 4) / BLOCK + 1, BLOCK);
    })
                                     : run(k_publish<false>, std::min<int64_t>(blocks_for(nbytes), 8192), kBlock);
    if (system_release) {   // the last launch that failed is the error
        const hipError_t r = launch_release_system(s);
        if (r != hipSuccess) err = r;
    }
    return err;
}

// Header-only publish: the payload of `slot` was already written by a write-through
// average of exactly these parameters.
__global__ void k_publish_header(char *__restrict__ slot, int64_t n, int32_t dtype, double *__restrict__ clock,
                                 double loss_h, const double *__restrict__ loss_d, int32_t loss_f32, uint64_t version)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    dpwa_header *h = reinterpret_cast<dpwa_header *>(slot);
    const double c = *clock + 1.0;                     // dpwa.py:112
    *clock = c;
    h->clock = c;
    h->loss = read_loss(loss_d, loss_f32, loss_h);
    h->version = version;
    h->n = n;
    h->dtype = dtype;
}

hipError_t launch_publish_header(char *slot, int64_t n, int32_t dtype, double *clock, double loss,
                                 const double *loss_dev, bool loss_f32, uint64_t version, bool system_release,
                                 hipStream_t s)
{
    hipLaunchKernelGGL(k_publish_header, dim3(1), dim3(64), 0, s, slot, n, dtype, clock, loss, loss_dev, (int32_t)loss_f32, version);
    if (system_release) hipLaunchKernelGGL(k_release_system, dim3(256), dim3(64), 0, s);
    return hipGetLastError();
}

// Reuse guard of a header-only publish (the adapter's write-through): writes
// through `param.data` move no version counter, so before a snapshot the last average wrote is
// published as is, the parameters are compared with it at kGuardSamples 16-B words, and what
// differs is copied.  The payload is cut into kGuardSamples chunks, chunk k = words [b(k), b(k+1))
// with b(k) = k (n16-1) / (samples-1) (the last chunk is the last word alone); chunk k is sampled
// at one word, b(k) + gen mod (its length), so the sampled word moves on by one each publish and
// every word of the parameters is compared once in any W = ceil((n16-1)/4095) publishes -- a
// sparse write through `param.data` that one publish's samples miss is published within W
// publishes, at the same per-publish cost.  The first word (and the tail bytes) are compared at
// every publish too.  A chunk whose sample differs is copied from the parameters into the
// payload by the workgroup that sampled it, so one launch does the check and the copy: no
// verdict has to reach other workgroups (round 5 ran a compare and a grid-wide conditional copy
// as two launches).  A workgroup that finds a difference stamps the verdict word with this
// publish's generation `gen` (never cleared; the first stamp of a generation counts a hit).
constexpr int kGuardSamples = 4096;
constexpr int kGuardWave = 64;
constexpr int kGuardChunksPerBlock = 16;     // chunks sampled by one workgroup (lanes 0..15 of wave 0)
constexpr int kGuardBlock = 256;             // 4 waves copy a dirty chunk

// b(k) = k (n16-1) / (samples-1).  samples = min(n16, kGuardSamples): below kGuardSamples words it
// is k itself, otherwise the divisor is the constant kGuardSamples-1, which compiles to a
// multiply-high -- the sampling lanes' addresses wait on this, and a 64-bit division by a
// variable is a long emulated sequence on the VALU.
__device__ __forceinline__ int64_t guard_base(int64_t k, int64_t samples, int64_t n16)
{
    if (samples <= 1) return 0;
    if (samples < kGuardSamples) return k;
    return (int64_t)((uint64_t)k * (uint64_t)(n16 - 1) / (uint64_t)(kGuardSamples - 1));
}

// Byte offset of the word sampled in chunk k (of `samples`) over n16 16-B words at generation `gen`.
__device__ __forceinline__ int64_t guard_offset(int64_t k, int64_t samples, int64_t n16, uint32_t gen)
{
    if (samples <= 1 || k >= samples - 1) return (samples > 1 ? n16 - 1 : 0) << 4;
    const int64_t b = guard_base(k, samples, n16);
    const int64_t len = guard_base(k + 1, samples, n16) - b;        // >= 1
    const int64_t r = len <= (int64_t)UINT32_MAX ? (int64_t)(gen % (uint32_t)len) : (int64_t)(gen % (uint64_t)len);
    return (b + r) << 4;
}

__global__ __launch_bounds__(kGuardBlock) void k_guard_publish(const char *__restrict__ flat,
                                                               char *__restrict__ payload, int64_t nbytes,
                                                               int32_t *__restrict__ dirty,
                                                               uint32_t *__restrict__ hits, int32_t gen)
{
    __shared__ uint32_t s_mask;
    const int64_t n16 = nbytes >> 4;
    const int64_t samples = n16 < kGuardSamples ? n16 : kGuardSamples;
    const int64_t k0 = (int64_t)blockIdx.x * kGuardChunksPerBlock;
    const int t = threadIdx.x;
    if (t < kGuardWave) {
        int diff = 0;
        const int64_t k = k0 + t;
        if (t < kGuardChunksPerBlock && k < samples) {
            const int64_t o = guard_offset(k, samples, n16, (uint32_t)gen);
            const u32x4 a = *reinterpret_cast<const u32x4 *>(flat + o);
            const u32x4 b = *reinterpret_cast<const u32x4 *>(payload + o);
            diff = (a.x != b.x) | (a.y != b.y) | (a.z != b.z) | (a.w != b.w);
        }
        if (blockIdx.x == 0 && t == kGuardChunksPerBlock && n16 > 0) {   // the first word, always: chunk 0
            const u32x4 a = *reinterpret_cast<const u32x4 *>(flat);
            const u32x4 b = *reinterpret_cast<const u32x4 *>(payload);
            if ((a.x != b.x) | (a.y != b.y) | (a.z != b.z) | (a.w != b.w)) diff = 1;
        }
        // bit c: chunk k0 + c differs (the first-word lane reports chunk 0)
        const uint64_t ballot = __ballot(diff);
        uint32_t mask = (uint32_t)(ballot & ((1u << kGuardChunksPerBlock) - 1u));
        if (ballot >> kGuardChunksPerBlock) mask |= 1u;
        if (t == 0) s_mask = mask;
    }
    // the tail bytes (past the last whole word) belong to workgroup 0: compared and copied in place
    int tail_diff = 0;
    if (blockIdx.x == 0 && t >= kGuardWave && t < kGuardWave + (nbytes & 15)) {
        const int64_t j = (n16 << 4) + (t - kGuardWave);
        if (flat[j] != payload[j]) {
            payload[j] = flat[j];
            tail_diff = 1;
        }
    }
    tail_diff = __syncthreads_or(tail_diff);
    const uint32_t mask = s_mask;
    if ((mask || tail_diff) && t == 0) {
        const int32_t old = atomicExch(dirty, gen);
        if (old != gen) atomicAdd(hits, 1u);
    }
    for (uint32_t m = mask; m; m &= m - 1) {
        const int64_t k = k0 + __builtin_ctz(m);
        const int64_t lo = k >= samples - 1 ? (samples > 1 ? n16 - 1 : 0) : guard_base(k, samples, n16);
        const int64_t hi = k >= samples - 1 ? n16 : guard_base(k + 1, samples, n16);
        u32x4 *d = reinterpret_cast<u32x4 *>(payload);
        const u32x4 *src = reinterpret_cast<const u32x4 *>(flat);
        copy16(d, src, hi, lo + t, kGuardBlock);
    }
}

// The same check for operands that are not 16-B aligned (the flat buffers are 256-B aligned, so
// only the stateless ABI reaches it): one thread per chunk compares its sampled word bytewise and
// copies its chunk when it differs.
__global__ __launch_bounds__(kGuardWave) void k_guard_publish_bytes(const char *__restrict__ flat,
                                                                    char *__restrict__ payload, int64_t nbytes,
                                                                    int32_t *__restrict__ dirty,
                                                                    uint32_t *__restrict__ hits, int32_t gen)
{
    const int64_t n16 = nbytes >> 4;
    const int64_t samples = n16 < kGuardSamples ? n16 : kGuardSamples;
    const int64_t k = (int64_t)blockIdx.x * kGuardWave + threadIdx.x;
    int diff = 0;
    if (k < samples) {
        const int64_t o = guard_offset(k, samples, n16, (uint32_t)gen);
        for (int j = 0; j < 16; ++j) diff |= flat[o + j] != payload[o + j];
        if (k == 0)
            for (int j = 0; j < 16; ++j) diff |= flat[j] != payload[j];
        if (diff) {
            const int64_t lo = (k >= samples - 1 ? (samples > 1 ? n16 - 1 : 0) : guard_base(k, samples, n16)) << 4;
            const int64_t hi = (k >= samples - 1 ? n16 : guard_base(k + 1, samples, n16)) << 4;
            for (int64_t i = lo; i < hi; ++i) payload[i] = flat[i];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (nbytes & 15)) {
        const int64_t j = (n16 << 4) + threadIdx.x;
        if (flat[j] != payload[j]) {
            payload[j] = flat[j];
            diff = 1;
        }
    }
    diff = __syncthreads_or(diff);
    if (diff && threadIdx.x == 0) {
        const int32_t old = atomicExch(dirty, gen);
        if (old != gen) atomicAdd(hits, 1u);
    }
}

hipError_t launch_guard_payload(char *payload, const void *flat, int64_t nbytes, int32_t *dirty, uint32_t *hits,
                                int32_t gen, hipStream_t s)
{
    if (nbytes <= 0) return hipSuccess;
    const char *src = (const char *)flat;
    const int64_t n16 = nbytes >> 4;
    const int64_t samples = n16 < kGuardSamples ? n16 : kGuardSamples;
    if (aligned16(flat) && aligned16(payload)) {
        const uint32_t g = (uint32_t)std::max<int64_t>(1, (samples + kGuardChunksPerBlock - 1) / kGuardChunksPerBlock);
        hipLaunchKernelGGL(k_guard_publish, dim3(g), dim3(kGuardBlock), 0, s, src, payload, nbytes, dirty, hits, gen);
    } else {
        const uint32_t g = (uint32_t)std::max<int64_t>(1, (samples + kGuardWave - 1) / kGuardWave);
        hipLaunchKernelGGL(k_guard_publish_bytes, dim3(g), dim3(kGuardWave), 0, s, src, payload, nbytes, dirty, hits,
                           gen);
    }
    return hipGetLastError();
}

// Window guard of resident parameters.  Between update_send and update_wait the resident
// parameters ARE the snapshot peers read; writes through `param.data` there move no version
// counter.  One launch per publish: the payload published last time -- untouched since its
// window closed, until the average after this publish overwrites that slot -- is compared with the
// samples saved when it was published (k_guard_publish's offsets of that publish's generation
// `gen`), then the samples of the payload published now (generation `cur_gen`, the offsets moved on
// by one) are saved in their place.  Each lane owns one sample, so the compare and the save of a
// sample are in one lane, in order.  `old` NULL: save only; `cur` NULL: compare only.  Layout of
// `sample`: kGuardSamples words, the tail bytes, the first word, the last word.
static_assert(kWindowSampleBytes == (kGuardSamples + 3) * 16, "window sample layout");

__global__ __launch_bounds__(kGuardWave) void k_window_roll(const char *__restrict__ old, const char *__restrict__ cur,
                                                            int64_t nbytes, char *__restrict__ sample,
                                                            int32_t *__restrict__ dirty, uint32_t *__restrict__ hits,
                                                            uint32_t *__restrict__ host, int32_t gen, int32_t cur_gen)
{
    const int64_t n16 = nbytes >> 4;
    const int64_t samples = n16 < kGuardSamples ? n16 : kGuardSamples;
    const int64_t k = (int64_t)blockIdx.x * kGuardWave + threadIdx.x;
    const bool tail = blockIdx.x == 0 && threadIdx.x < (nbytes & 15);
    char *const tail_sample = sample + kGuardSamples * 16 + threadIdx.x;
    u32x4 *const sk = reinterpret_cast<u32x4 *>(sample) + k;
    // lanes 0 and 1 of workgroup 0 also own the first and the last word (fixed, every window)
    const bool edge = blockIdx.x == 0 && threadIdx.x < 2 && n16 > 0;
    const int64_t edge_off = threadIdx.x ? (n16 - 1) << 4 : 0;
    u32x4 *const se = reinterpret_cast<u32x4 *>(sample) + kGuardSamples + 1 + threadIdx.x;
    int diff = 0;
    if (old) {
        if (k < samples) {
            const u32x4 a = *reinterpret_cast<const u32x4 *>(old + guard_offset(k, samples, n16, (uint32_t)gen));
            const u32x4 b = *sk;
            diff = (a.x != b.x) | (a.y != b.y) | (a.z != b.z) | (a.w != b.w);
        }
        if (tail) diff |= old[(n16 << 4) + threadIdx.x] != *tail_sample;
        if (edge) {
            const u32x4 a = *reinterpret_cast<const u32x4 *>(old + edge_off);
            const u32x4 b = *se;
            diff |= (a.x != b.x) | (a.y != b.y) | (a.z != b.z) | (a.w != b.w);
        }
    }
    if (cur) {
        if (k < samples) *sk = *reinterpret_cast<const u32x4 *>(cur + guard_offset(k, samples, n16, (uint32_t)cur_gen));
        if (tail) *tail_sample = cur[(n16 << 4) + threadIdx.x];
        if (edge) *se = *reinterpret_cast<const u32x4 *>(cur + edge_off);
    }
    if (!old) return;
    diff = __syncthreads_or(diff);
    if (diff && threadIdx.x == 0) {
        const int32_t prev = atomicExch(dirty, gen);
        if (prev != gen) *host = atomicAdd(hits, 1u) + 1u;   // one workgroup per window
    }
}

hipError_t launch_window_roll(const char *old, const char *cur, int64_t nbytes, char *sample, int32_t *dirty,
                              uint32_t *hits, uint32_t *host, int32_t gen, int32_t cur_gen, hipStream_t s)
{
    if (nbytes <= 0 || (!old && !cur)) return hipSuccess;
    if (!aligned16(old) || !aligned16(cur) || !aligned16(sample)) return hipErrorInvalidValue;
    const int64_t n16 = nbytes >> 4;
    const int64_t samples = n16 < kGuardSamples ? n16 : kGuardSamples;
    const uint32_t g = (uint32_t)((samples + kGuardWave - 1) / kGuardWave + (samples == 0 ? 1 : 0));
    hipLaunchKernelGGL(k_window_roll, dim3(g), dim3(kGuardWave), 0, s, old, cur, nbytes, sample, dirty, hits, host,
                       gen, cur_gen);
    return hipGetLastError();
}

// The access mix of an averaging kernel with nothing else in it, for measurement only
// (dpwa_stream_mix, bench.py `roofline.mix_ceiling`): each one-wave workgroup loads the same
// 1-KiB span of NR source buffers and stores one combination of them into the span of NW
// destinations, with exactly the product kernel's instruction shapes and cache policy
// (the first source loaded as the peer is, `nt`, the second as the parameters are; the first
// destination stored as the parameters are, the others as the snapshot is; POLICY is what an
// average of nbytes takes, lerp_policy(nbytes)) but no factor and no arithmetic beyond one add
// per word: the ceiling that launch shape reaches on this chip at a given size, timed in the same
// run as the product kernel.
template <int NR, int NW, int POLICY>
__global__ __launch_bounds__(kStreamBlock) void k_stream_mix(StreamMixArgs a)
{
    constexpr int SPAN = kStreamBlock * 16;
    const int64_t span_off = (int64_t)blockIdx.x * SPAN;
    const int lane_off = threadIdx.x * 16;
    u32x4 v[NR];
    v[0] = __builtin_amdgcn_raw_buffer_load_b128(span_rsrc<SPAN>(a.src[0], span_off, a.nbytes), lane_off, 0, kAuxStream);
#pragma unroll
    for (int i = 1; i < NR; ++i)
        v[i] = __builtin_amdgcn_raw_buffer_load_b128(span_rsrc<SPAN>(a.src[i], span_off, a.nbytes), lane_off, 0,
                                                     LerpPolicy<POLICY>::param_load);
    u32x4 r = v[0];
#pragma unroll
    for (int i = 1; i < NR; ++i) r = r + v[i];
    __builtin_amdgcn_raw_buffer_store_b128(r, span_rsrc<SPAN>(a.dst[0], span_off, a.nbytes), lane_off, 0,
                                           LerpPolicy<POLICY>::store);
    if (NW > 1)
        __builtin_amdgcn_raw_buffer_store_b128(r, span_rsrc<SPAN>(a.dst[1], span_off, a.nbytes), lane_off, 0,
                                               LerpPolicy<POLICY>::snap_store);
}

hipError_t launch_stream_mix(const StreamMixArgs &a, hipStream_t s, const LaunchTiming *timing)
{
    if (a.nr < 1 || a.nr > 2 || a.nw < 1 || a.nw > 2 || a.nbytes < 0 || (a.nbytes & 15)) return hipErrorInvalidValue;
    const uint32_t g = (uint32_t)(a.nbytes / (kStreamBlock * 16) + 1);
    return BySizePolicies::with(lerp_policy(a.nbytes), [&](auto policy) {
        constexpr int P = decltype(policy)::value;
        void (*k)(StreamMixArgs) = a.nr == 1 ? (a.nw == 1 ? k_stream_mix<1, 1, P> : k_stream_mix<1, 2, P>)
                                             : (a.nw == 1 ? k_stream_mix<2, 1, P> : k_stream_mix<2, 2, P>);
        return launch(k, dim3(g), dim3(kStreamBlock), s, timing, a);
    });
}

// One 64-bit word into (host-mapped) memory after everything before it on the stream: a
// system-scope release store, so the bytes written before it are visible first.  Used by
// the gossip board (board.cpp) for versions and read marks.
__global__ void k_store_u64(uint64_t *p, uint64_t v)
{
    if (threadIdx.x == 0) __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t launch_store_u64(uint64_t *p, uint64_t v, hipStream_t s)
{
    hipLaunchKernelGGL(k_store_u64, dim3(1), dim3(64), 0, s, p, v);
    return hipGetLastError();
}

// ---------------------------------------------------------------- consensus of a group
// Opt-in and read-only (include/dpwa_hip.h dpwa_consensus): the element-wise mean of U = 1..8 published
// snapshots and how far the members are from it, in one pass that reads every source once.  For
// every element, the members in the order given:
//   s = ((x_0 + x_1) + ...) + x_{U-1}     each operand widened exactly to fp64, fp64 adds
//   m = s * r                             r = 1.0 / U formed once by the host: a multiply, no division
//   out = f32(m)                          v_cvt_f32_f64, RNE, subnormals kept; a 16-bit payload then
//                                         rounds that fp32 value RNE with the converts OpsBF16 / OpsF16
//                                         use -- two roundings, on purpose
//   norm2 += m * m      spread2_i += (x_i - m) * (x_i - m)      against the fp64 m, all in fp64
// group_span's shape: one-wave workgroups over an exact grid of 1-KiB spans, all U 16-byte loads
// issued first (`nt`: every byte is read once), one 16-byte store of the mean (`sc1`, as a
// snapshot store); lanes past the end load zeros, whose mean is zero and which add 0 to every sum;
// the ragged tail of a single-dtype payload element by element in workgroup 0.  TRACK: the wave
// sums its U + 1 partial sums with the butterfly and lanes 0..U add them with ONE fp64 atomic
// instruction into the 128-byte row `span mod kDistAccs` of the workspace -- norm2 first, then
// spread2_0.. -- which k_consensus_finish sums in a fixed order and leaves zero.  STORE off:
// nothing is stored to any payload.
struct ConsensusArgs {
    const void *src[kMaxConsensus];
    void *out;      // STORE
    double *acc;    // TRACK
    double r;
};

// element e of a lane's 16-byte item / one element of the tail, widened exactly to fp64
__device__ __forceinline__ double cons_elem(OpsF32, u32x4 v, int e) { return (double)__uint_as_float(v[e]); }
__device__ __forceinline__ double cons_elem(OpsBF16, u32x4 v, int e)
{
    return (double)((e & 1) ? bf_hi(v[e >> 1]) : bf_lo(v[e >> 1]));
}
__device__ __forceinline__ double cons_elem(OpsF16, u32x4 v, int e)
{
    const uint32_t w = v[e >> 1];   // (a value of its own: a bit_cast of the vector's element read word 0 for every e)
    const f16x2v h = __builtin_bit_cast(f16x2v, w);
    return (double)((e & 1) ? h.y : h.x);
}
__device__ __forceinline__ double cons_elem_s(OpsF32, float x) { return (double)x; }
__device__ __forceinline__ double cons_elem_s(OpsBF16, uint16_t x) { return (double)bf_lo(x); }
__device__ __forceinline__ double cons_elem_s(OpsF16, uint16_t x) { return (double)__builtin_bit_cast(_Float16, x); }

// the fp32 means of an item as the payload's type
__device__ __forceinline__ u32x4 cons_pack(OpsF32, const float *f)
{
    return u32x4{__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3])};
}
__device__ __forceinline__ u32x4 cons_pack(OpsBF16, const float *f)
{
    return u32x4{pk_bf16(f[0], f[1]), pk_bf16(f[2], f[3]), pk_bf16(f[4], f[5]), pk_bf16(f[6], f[7])};
}
__device__ __forceinline__ u32x4 cons_pack(OpsF16, const float *f)
{
    return u32x4{pk_f16(f[0], f[1]), pk_f16(f[2], f[3]), pk_f16(f[4], f[5]), pk_f16(f[6], f[7])};
}
__device__ __forceinline__ float cons_pack_s(OpsF32, float f) { return f; }
__device__ __forceinline__ uint16_t cons_pack_s(OpsBF16, float f) { return (uint16_t)(pk_bf16(f, 0.0f) & 0xffffu); }
__device__ __forceinline__ uint16_t cons_pack_s(OpsF16, float f) { return (uint16_t)(pk_f16(f, 0.0f) & 0xffffu); }

// One element: the members' values in order -> the fp32 mean; TRACK: its terms into the lane's sums.
template <int U, bool TRACK>
__device__ __forceinline__ float cons_one(const double (&x)[U], double r, double &n2, double (&sp)[U])
{
    double s = x[0];
#pragma unroll
    for (int i = 1; i < U; ++i) s = s + x[i];
    const double m = s * r;
    if constexpr (TRACK) {
        n2 = n2 + m * m;
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const double d = x[i] - m;
            sp[i] = sp[i] + d * d;
        }
    }
    return (float)m;
}

// A lane's item of every member -> the item of the mean, its elements in order.
template <class Ops, int U, bool TRACK>
__device__ __forceinline__ u32x4 cons_item(const u32x4 (&v)[U], double r, double &n2, double (&sp)[U])
{
    float f[Ops::PER];
#pragma unroll
    for (int e = 0; e < Ops::PER; ++e) {
        double x[U];
#pragma unroll
        for (int i = 0; i < U; ++i) x[i] = cons_elem(Ops{}, v[i], e);
        f[e] = cons_one<U, TRACK>(x, r, n2, sp);
    }
    return cons_pack(Ops{}, f);
}

// The wave's U + 1 sums into the row of `span`: one atomic instruction, lane 0 adding norm2 and
// lane 1 + i member i's spread2 (a select over registers by the lane, no indexed access).
template <int U>
__device__ __forceinline__ void cons_commit(double *acc, uint32_t span, double n2, double (&sp)[U])
{
    static_assert(U + 1 <= kDistAccStride, "the sums of one span share a row");
    const int lane = threadIdx.x & 63;
    double v = wave_sum(n2);
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const double t = wave_sum(sp[i]);
        v = lane == i + 1 ? t : v;
    }
    if (lane <= U) unsafeAtomicAdd(acc + (size_t)(span % kDistAccs) * kDistAccStride + lane, v);
}

template <class Ops, int U, bool STORE, bool TRACK>
__global__ __launch_bounds__(kStreamBlock) void k_consensus(ConsensusArgs a, int64_t n)
{
    using S = typename Ops::S;
    constexpr int SPAN = kStreamBlock * 16;
    const int64_t vbytes = n / Ops::PER * 16;
    const int64_t off = (int64_t)blockIdx.x * SPAN;
    const int lane_off = threadIdx.x * 16;
    u32x4 v[U];
#pragma unroll
    for (int j = 0; j < U; ++j)   // all loads first
        v[j] = span_load<u32x4>(span_rsrc<SPAN>(a.src[j], off, vbytes), lane_off);
    __builtin_amdgcn_sched_barrier(0);   // (left alone, the scheduler issues the 8th load behind the first seven's adds)
    [[maybe_unused]] double n2 = 0.0, sp[U];
#pragma unroll
    for (int i = 0; i < U; ++i) sp[i] = 0.0;
    const u32x4 mean = cons_item<Ops, U, TRACK>(v, a.r, n2, sp);
    if constexpr (STORE) span_store<u32x4>(span_rsrc<SPAN>(a.out, off, vbytes), lane_off, mean);
    const int64_t tail = n / Ops::PER * Ops::PER;
    if (blockIdx.x == 0 && threadIdx.x < n - tail) {
        const int64_t j = tail + threadIdx.x;
        double x[U];
#pragma unroll
        for (int i = 0; i < U; ++i) x[i] = cons_elem_s(Ops{}, reinterpret_cast<const S *>(a.src[i])[j]);
        const float f = cons_one<U, TRACK>(x, a.r, n2, sp);
        if constexpr (STORE) reinterpret_cast<S *>(a.out)[j] = cons_pack_s(Ops{}, f);
    }
    if constexpr (TRACK) cons_commit<U>(a.acc, blockIdx.x, n2, sp);
}

// The same span code over a segmented payload: the span's element type is its segment's, looked up
// from the span's byte offset after the loads were issued (as k_lerp_mixed); no ragged tail;
// padding bytes are zeros in every member, whose mean is zero and which add 0.
template <int U, bool STORE, bool TRACK>
__global__ __launch_bounds__(kStreamBlock) void k_consensus_mixed(ConsensusArgs a, int64_t total, SegTable segs)
{
    constexpr int SPAN = kStreamBlock * 16;
    const int64_t off = (int64_t)blockIdx.x * SPAN;
    const int lane_off = threadIdx.x * 16;
    u32x4 v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = span_load<u32x4>(span_rsrc<SPAN>(a.src[j], off, total), lane_off);
    __builtin_amdgcn_sched_barrier(0);   // (left alone, the scheduler issues the 8th load behind the first seven's adds)
    [[maybe_unused]] double n2 = 0.0, sp[U];
#pragma unroll
    for (int i = 0; i < U; ++i) sp[i] = 0.0;
    const int32_t dtype = seg_dtype(segs, off);
    u32x4 mean;
    if (dtype == DPWA_F32) mean = cons_item<OpsF32, U, TRACK>(v, a.r, n2, sp);
    else if (dtype == DPWA_BF16) mean = cons_item<OpsBF16, U, TRACK>(v, a.r, n2, sp);
    else mean = cons_item<OpsF16, U, TRACK>(v, a.r, n2, sp);
    if constexpr (STORE) span_store<u32x4>(span_rsrc<SPAN>(a.out, off, total), lane_off, mean);
    if constexpr (TRACK) cons_commit<U>(a.acc, blockIdx.x, n2, sp);
}

// Finishing (one workgroup behind the pass on the same stream, as k_distance_finish): lane i loads
// and zeroes row i, the sums are taken in a fixed order -- the butterfly inside each wave, then the
// waves in order, then spread2 over the members in order -- and the record is written whole.
constexpr int kConsensusSums = kMaxConsensus + 1;

__global__ __launch_bounds__(kDistFinishBlock) void k_consensus_finish(double *__restrict__ acc,
                                                                       dpwa_consensus_record *__restrict__ out, int64_t n,
                                                                       int32_t members, uint64_t version)
{
    __shared__ double s_sum[kConsensusSums][kDistFinishBlock / 64];
    double *a = acc + (size_t)threadIdx.x * kDistAccStride;
    double v[kConsensusSums];
#pragma unroll
    for (int k = 0; k < kConsensusSums; ++k) v[k] = __hip_atomic_load(a + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int k = 0; k < kConsensusSums; ++k) __hip_atomic_store(a + k, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int k = 0; k < kConsensusSums; ++k) {
        const double t = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) s_sum[k][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    __shared__ double s_total[kConsensusSums];
    if (threadIdx.x < kConsensusSums) {   // lane k: sum k over the waves in order
        double t = s_sum[threadIdx.x][0];
        for (int w = 1; w < kDistFinishBlock / 64; ++w) t = t + s_sum[threadIdx.x][w];
        s_total[threadIdx.x] = threadIdx.x <= (unsigned)members ? t : 0.0;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double spread2 = s_total[1];
    out->member_spread2[0] = spread2;
    for (int i = 1; i < kMaxConsensus; ++i) {
        out->member_spread2[i] = s_total[1 + i];
        if (i < members) spread2 = spread2 + s_total[1 + i];
    }
    out->norm2 = s_total[0];
    out->spread2 = spread2;
    out->n = n;
    out->members = members;
    out->reserved = 0;
    out->version = version;
#pragma unroll
    for (int k = 0; k < (int)(sizeof(out->pad) / sizeof(out->pad[0])); ++k) out->pad[k] = 0;
}

// The bytes [p, p + bytes) and [q, q + bytes) share one.
static bool overlaps(const void *p, const void *q, int64_t bytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)bytes && b < a + (uintptr_t)bytes;
}

hipError_t launch_consensus(const Elems &e, const void *const *src, int count, double r, void *out, double *acc,
                            bool remote, hipStream_t s, const LaunchTiming *timing)
{
    if (count < 1 || count > kMaxConsensus || !src || (!out && !acc) || !aligned16(out, acc)) return hipErrorInvalidValue;
    if (!e.segmented() && (e.n < 0 || !is_float_dtype(e.dtype))) return hipErrorInvalidValue;
    if (e.segmented() && (!e.layout || layout_problem(*e.layout, -1))) return hipErrorInvalidValue;
    const int64_t bytes = e.segmented() ? layout_bytes(*e.layout) : e.bytes();
    ConsensusArgs a{};
    for (int i = 0; i < count; ++i) {
        if (absent_or_unaligned(src[i]) || (out && (src[i] == out || overlaps(src[i], out, bytes)))) return hipErrorInvalidValue;
        a.src[i] = src[i];
    }
    a.out = out;
    a.acc = acc;
    a.r = r;
    const bool store = out != nullptr, track = acc != nullptr;
    const auto acquire = [&] {   // (after every refusal: a refused launch queues nothing)
        if (remote) hipLaunchKernelGGL(k_acquire_system, dim3(256), dim3(64), 0, s);
    };
    return Choice<1, 2, 3, 4, 5, 6, 7, 8>::with(count, [&](auto members) {
        constexpr int U = decltype(members)::value;
        if (e.segmented())
            return with_segments(e, false, [&](int64_t total, dim3 grid, const SegTable &t) {
                acquire();
                return launch(store ? (track ? k_consensus_mixed<U, true, true> : k_consensus_mixed<U, true, false>)
                                    : k_consensus_mixed<U, false, true>,
                              grid, dim3(kStreamBlock), s, timing, a, total, t);
            });
        if (e.n == 0) return hipSuccess;
        return with_ops(e.dtype, [&](auto ops) {
            using Ops = decltype(ops);
            if (span_grid<Ops>(e.n, kStreamBlock) > 0x7fffffffLL) return hipErrorInvalidValue;
            acquire();
            return launch(store ? (track ? k_consensus<Ops, U, true, true> : k_consensus<Ops, U, true, false>)
                                : k_consensus<Ops, U, false, true>,
                          dim3((uint32_t)span_grid<Ops>(e.n, kStreamBlock)), dim3(kStreamBlock), s, timing, a, e.n);
        });
    });
}

hipError_t launch_consensus_finish(double *acc, dpwa_consensus_record *out, int64_t n, int members, uint64_t version,
                                   hipStream_t s, const LaunchTiming *timing)
{
    if (!acc || !out || members < 1 || members > kMaxConsensus || n < 0) return hipErrorInvalidValue;
    return launch(k_consensus_finish, dim3(1), dim3(kDistFinishBlock), s, timing, acc, out, n, members, version);
}

}  // namespace dpwa
