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
//             and float16 parameters (k_lerp<OpsMixed, ..., SegTable>): each one-wave span rounds as its segment's type.
//  * distance: opt-in -- the round's distance to the peer, sum (q - p)^2 and sum p^2 in fp64, formed
//             by a tracked form of the fused average from the operands it holds anyway
//             (k_lerp<..., DistTrack>), or by a stand-alone pass (k_distance*), added across workgroups with
//             the hardware fp64 add and finished by k_distance_finish.
//             Opt-in too: the same sums for every parameter tensor over its own elements, by a
//             stand-alone pass that looks each span's tensors up in a device table
//             (k_param_distance) and one finishing workgroup per tensor (k_param_distance_finish).
//  * non-finite peer check: opt-in -- one read of the fetched peer snapshot before the average
//             (k_peer_finite*), a test on the exponent bits; a lane that finds a NaN or an inf
//             stores the round's stamp into the learner's veto word, and the factor of a round
//             whose stamp it finds there is the no-op's, with a status of its own.
//  * healing: opt-in -- guarded forms of the single-learner average (k_lerp<..., HealGuard>) that select every
//             result element by the exponent bits of q and p: never a NaN or an inf from the peer, a NaN
//             or an inf of our own replaced by the peer's finite element, both counted.
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
#include <utility>

#include "kernels.hpp"
#include "policy.hpp"

#include <hip/hip_ext.h>

namespace dpwa {

constexpr int kBlock = 256;   // 4 waves of 64

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
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
// which `first_wg` holds commits the factor.  `new_clock` (the guarded kernels, one-wave workgroups, device or
// fused coefficients): where to leave the round's new clock.
template <int MODE, bool LDS = false>
__device__ __forceinline__ bool lerp_coef(const LerpArgs &args, bool first_wg, float &a, float &b,
                                          double *new_clock = nullptr)
{
    if (MODE == COEF_HOST) {
        a = args.a;
        b = args.b;
        return true;
    } else if (MODE == COEF_DEV) {
        if (args.coef->status != DPWA_STATUS_OK) return false;
        a = args.coef->a;
        b = args.coef->b;
        if (new_clock) *new_clock = args.coef->new_clock;
        return true;
    } else if (!LDS) {
        const dpwa_coef c = fused_factor(args.fused, first_wg && threadIdx.x == 0);
        a = c.a;
        b = c.b;
        if (new_clock) *new_clock = c.new_clock;
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

// What lerp_span does about the distance: nothing (every averaging kernel but the tracked k_lerp), or
// the sums above into `acc`.  (Arg: what k_lerp takes for it as a kernel argument.)
struct NoTrack {
    static constexpr bool ON = false;
};
struct DistTrack {
    static constexpr bool ON = true;
    using Arg = double *__restrict__;
    double *acc;
    operator double *() const { return acc; }
};

// ---------------------------------------------------------------- healing non-finite elements
// Opt-in (dpwa_learner_set_heal; the rule is stated in include/dpwa_hip.h "healing"): the guarded averaging
// kernels select every result element from what the lane holds anyway -- the peer's q, our p and the lerp r of
// the whole item -- by the exponent bits of q and p (all ones: bad; the test of the non-finite peer check):
//     q good, p good: r        q bad: p (refused)        q good, p bad: q (healed)
// No factor can do this (1*q + 0*p is NaN for a NaN p), so it is a select on the operands: per element two
// masks of whole elements, mq and mp, and two bit-field inserts (v_bfi_b32) into r.  A dword of a 16-bit type
// holds two elements that may fall in different rows, so each half's mask comes from its own half's exponent.
// No branch per element, no LDS.  The bad operands have been through the lerp; what it made of them is masked.
//
// Counting: a lane counts its healed and refused elements (at most 9 of each: the 8 of a 16-bit item and one
// tail element) in the halves of one register.  The wave's totals come from ballots: one ballot says whether
// any lane counted anything -- a clean span, which is what every round pays, ends there with no atomic -- and
// in a span that did, four ballots and population counts per counter (one per bit of the lane counts) add them
// up on the scalar unit; a DPP or shuffle reduction would move data across lanes six steps deep for the same
// two numbers and would have no cheaper answer to "anything at all?".  Lane 0 then adds the non-zero totals to
// the cumulative record with 64-bit vector global atomics; integer adds commute, so the record is bit-exact
// from run to run.  `rounds` and `clock` are written by the lane that commits the factor (COEF_DEV: lane 0 of
// global workgroup 0), for a round that averaged.
struct NoGuard {
    static constexpr bool ON = false;
};
struct HealGuard {
    static constexpr bool ON = true;
    using Arg = dpwa_heal_record *__restrict__;
    dpwa_heal_record *rec;
    operator dpwa_heal_record *() const { return rec; }
};

__device__ __forceinline__ uint32_t bad_mask_f32(uint32_t w) { return (w & 0x7f800000u) == 0x7f800000u ? 0xffffffffu : 0u; }
// the two 16-bit elements of a dword, exponent mask M (bf16 0x7f80, fp16 0x7c00): 0xffff over each bad half
template <uint32_t M> __device__ __forceinline__ uint32_t bad_mask_16x2(uint32_t w)
{
    return ((w & M) == M ? 0x0000ffffu : 0u) | ((w & (M << 16)) == (M << 16) ? 0xffff0000u : 0u);
}

// One dword: mq / mp cover the bad elements of q / p, E has the lowest bit of every element of the dword set.
template <uint32_t E>
__device__ __forceinline__ uint32_t heal_word(uint32_t q, uint32_t p, uint32_t r, uint32_t mq, uint32_t mp, uint32_t &counts)
{
    const uint32_t take_q = mp & ~mq;
    counts += (uint32_t)__builtin_popcount(take_q & E) + ((uint32_t)__builtin_popcount(mq & E) << 16);
    r = (q & take_q) | (r & ~take_q);
    return (p & mq) | (r & ~mq);
}

__device__ __forceinline__ f32x4 heal_item(OpsF32, f32x4 q, f32x4 p, f32x4 r, uint32_t &counts)
{
    const u32x4 qb = __builtin_bit_cast(u32x4, q), pb = __builtin_bit_cast(u32x4, p), rb = __builtin_bit_cast(u32x4, r);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = heal_word<1u>(qb[e], pb[e], rb[e], bad_mask_f32(qb[e]), bad_mask_f32(pb[e]), counts);
    return __builtin_bit_cast(f32x4, o);
}

template <uint32_t M> __device__ __forceinline__ u32x4 heal_item16(u32x4 q, u32x4 p, u32x4 r, uint32_t &counts)
{
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        o[e] = heal_word<0x00010001u>(q[e], p[e], r[e], bad_mask_16x2<M>(q[e]), bad_mask_16x2<M>(p[e]), counts);
    return o;
}
__device__ __forceinline__ u32x4 heal_item(OpsBF16, u32x4 q, u32x4 p, u32x4 r, uint32_t &counts)
{
    return heal_item16<0x7f80u>(q, p, r, counts);
}
__device__ __forceinline__ u32x4 heal_item(OpsF16, u32x4 q, u32x4 p, u32x4 r, uint32_t &counts)
{
    return heal_item16<0x7c00u>(q, p, r, counts);
}

// One element (the ragged tail); a 16-bit element is the low half of a dword whose high half is zero (good).
__device__ __forceinline__ float heal_s(OpsF32, float q, float p, float r, uint32_t &counts)
{
    const uint32_t qb = __float_as_uint(q), pb = __float_as_uint(p);
    return __uint_as_float(heal_word<1u>(qb, pb, __float_as_uint(r), bad_mask_f32(qb), bad_mask_f32(pb), counts));
}
__device__ __forceinline__ uint16_t heal_s(OpsBF16, uint16_t q, uint16_t p, uint16_t r, uint32_t &counts)
{
    return (uint16_t)heal_word<1u>(q, p, r, bad_mask_16x2<0x7f80u>(q), bad_mask_16x2<0x7f80u>(p), counts);
}
__device__ __forceinline__ uint16_t heal_s(OpsF16, uint16_t q, uint16_t p, uint16_t r, uint32_t &counts)
{
    return (uint16_t)heal_word<1u>(q, p, r, bad_mask_16x2<0x7c00u>(q), bad_mask_16x2<0x7c00u>(p), counts);
}

__device__ __forceinline__ void heal_commit(dpwa_heal_record *rec, bool first_wg, uint32_t counts, double new_clock)
{
    if (first_wg && threadIdx.x == 0) {   // (this lane alone writes them)
        rec->rounds = rec->rounds + 1;
        rec->clock = new_clock;
    }
    if (__builtin_amdgcn_ballot_w64(counts != 0) == 0) return;   // uniform: a clean span
    uint32_t healed = 0, refused = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // lane counts are <= 9: four bit planes
        healed += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((counts >> k) & 1u)) << k;
        refused += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((counts >> (16 + k)) & 1u)) << k;
    }
    if (threadIdx.x != 0) return;
    if (healed) __hip_atomic_fetch_add(&rec->healed, (uint64_t)healed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (refused) __hip_atomic_fetch_add(&rec->refused, (uint64_t)refused, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One 16-byte item per lane; items beyond n/PER (the ragged tail) go to block 0.
// DUAL also stores the result into args.snap (write-through snapshot: the next publish of
// these parameters then needs no copy).  OOP (with DUAL): the result is stored into args.snap
// ONLY -- the resident form, whose parameters live in the learner's own snapshot slots and move
// from the published slot to the next one at every average (2 reads + 1 write per element, the
// averaging's own bytes; learner.cpp "resident").  BLOCK lanes per workgroup (kStreamBlock).
// Track (DistTrack, one-wave workgroups only): a round that averages also adds its distance sums,
// formed from the q and p this lane loaded anyway; a no-op round adds nothing.
// Guard (HealGuard, one-wave workgroups, device or fused coefficients; "healing non-finite elements" above): a
// round that averages selects every result element by the rule of include/dpwa_hip.h and counts what it healed
// and refused; a no-op round selects and counts nothing.
template <class Ops, int MODE, bool DUAL, int BLOCK, int POLICY, class Src, bool OOP = false, class Track = NoTrack,
          class Guard = NoGuard>
__device__ __forceinline__ void lerp_span(uint32_t blk, typename Ops::V *__restrict__ param, const Src &src,
                                          int64_t n, const LerpArgs &args, const Ops &ops = Ops{},
                                          const Track &track = Track{}, const Guard &guard = Guard{})
{
    static_assert(!Track::ON || BLOCK == 64, "the tracked form runs one-wave workgroups");
    static_assert(!Guard::ON || (BLOCK == 64 && MODE != COEF_HOST), "the guarded form: one wave, a dpwa_coef");
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
    [[maybe_unused]] double new_clock = 0.0;
    if (!lerp_coef<MODE, BLOCK != 64>(args, blk == 0, a, b, Guard::ON ? &new_clock : nullptr)) {
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
    V r = ops.lerp(a, b, q, p);
    [[maybe_unused]] uint32_t counts = 0;   // HealGuard: this lane's healed | refused << 16
    if constexpr (Guard::ON) r = heal_item(ops, q, p, r, counts);
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
            S t = Ops::lerp_s(a, b, qs, pj);
            if constexpr (Guard::ON) t = heal_s(ops, qs, pj, t, counts);
            if (!OOP) ps[j] = t;
            if (DUAL) reinterpret_cast<S *>(args.snap)[j] = t;
            if constexpr (Track::ON) dist_add_s(ops, qs, pj, d2, n2);
        }
    }
    if constexpr (Track::ON) dist_commit(track.acc, blk, d2, n2);
    if constexpr (Guard::ON) heal_commit(guard.rec, blk == 0, counts, new_clock);
}

// ---------------------------------------------------------------- segmented (DPWA_MIXED) payloads
// A model that mixes float32, bfloat16 and float16 parameters has a payload of up to three
// segments, one per type, each a whole number of 4-KiB blocks (dpwa_layout, include/dpwa_hip.h): a
// 1-KiB span lies inside one segment.  The table travels by value; unused entries begin at
// INT64_MAX, so the lookup is two compares whatever the count.
struct SegTable {
    using Arg = SegTable;
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

// The same test over a segmented payload: the span's test, like its lerp, is its segment's (seg_dtype from the
// span's byte offset; padding bytes are zeros on both sides: good, and they stay zeros).
__device__ __forceinline__ u32x4 heal_item(const OpsMixed &ops, u32x4 q, u32x4 p, u32x4 r, uint32_t &counts)
{
    const int32_t dtype = seg_dtype(ops.segs, ops.span_off);
    if (dtype == DPWA_F32)
        return __builtin_bit_cast(u32x4, heal_item(OpsF32{}, __builtin_bit_cast(f32x4, q), __builtin_bit_cast(f32x4, p),
                                                   __builtin_bit_cast(f32x4, r), counts));
    if (dtype == DPWA_BF16) return heal_item(OpsBF16{}, q, p, r, counts);
    return heal_item(OpsF16{}, q, p, r, counts);
}

// A trailing kernel argument (Form::Arg) as lerp_span takes it: the table itself, DistTrack{acc}, HealGuard{rec}.
template <class Form> __device__ __forceinline__ decltype(auto) as_form(const typename Form::Arg &a)
{
    if constexpr (std::is_same_v<Form, typename Form::Arg>) return (a);
    else return Form{a};
}
// The one of type T among xs (a kernel's trailing arguments, then the defaults of those a form leaves out).
template <class T, class X, class... Xs> __device__ __forceinline__ const T &arg_of(const X &x, const Xs &...xs)
{
    if constexpr (std::is_same_v<T, X>) return x;
    else return arg_of<T>(xs...);
}
// The element op of workgroup `blk`'s span: a segmented payload's finds its segment in the SegTable among xs.
template <class Ops, int SPAN, class... Xs>
__device__ __forceinline__ Ops span_ops(const ContigSrc &src, uint32_t blk, const Xs &...xs)
{
    if constexpr (std::is_same_v<Ops, OpsMixed>) return OpsMixed{arg_of<SegTable>(xs...), src.span_of<SPAN>(blk)};
    else return Ops{};
}

// The single-learner average over a contiguous peer payload, every form of it: lerp_span behind the kernel
// arguments (param, peer, n, args) and, only in the instantiations that use them, in this order
//     SegTable   a segmented payload (Ops = OpsMixed; `n` counts its bytes): the span's element op is chosen by
//                the span's byte offset -- not by the workgroup index: right for any span order -- and the
//                commit is by one lane of the grid, of global workgroup 0, not of each segment's first workgroup;
//                no ragged tail, no unaligned form, an exact grid, one-wave workgroups
//     DistTrack  the tracked form of the fused average: the averaged bits are the untracked ones
//     HealGuard  the guarded forms ("healing non-finite elements"): a good/good element has the unguarded bits;
//                fused or device coefficients (the lerp of a split round)
// DistTrack and HealGuard run one-wave workgroups over 16-B aligned operands, and never together: there is no
// guarded tracked form.  What is launched for which call: "averaging launches" below.
template <class Ops, int MODE, bool DUAL, int BLOCK = kBlock, int POLICY = 0, bool OOP = false, class... Form>
__global__ __launch_bounds__(BLOCK) void k_lerp(typename Ops::V *__restrict__ param,
                                                const typename Ops::V *__restrict__ peer, int64_t n, LerpArgs args,
                                                typename Form::Arg... form)
{
    using Track = std::conditional_t<(std::is_same_v<Form, DistTrack> || ...), DistTrack, NoTrack>;
    using Guard = std::conditional_t<(std::is_same_v<Form, HealGuard> || ...), HealGuard, NoGuard>;
    const ContigSrc src{(const char *)peer};
    lerp_span<Ops, MODE, DUAL, BLOCK, POLICY, ContigSrc, OOP, Track, Guard>(
        blockIdx.x, param, src, n, args, span_ops<Ops, BLOCK * 16>(src, blockIdx.x, as_form<Form>(form)...),
        arg_of<Track>(as_form<Form>(form)..., NoTrack{}), arg_of<Guard>(as_form<Form>(form)..., NoGuard{}));
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
// byte offset, as the segmented k_lerp; no ragged tail; padding bytes are zeros, which are finite).
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
// the tracked, guarded and segmented k_lerp (not resident), k_stream_mix: the two policies the size chooses between
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
// (range-checked).  A payload with no ragged tail (segmented: whole 4-KiB blocks) has an exact grid.
template <class Ops> static int64_t span_grid(int64_t n, int block) { return (n / Ops::PER) / block + (Ops::TAIL ? 1 : 0); }
// Workgroups of the grid-stride kernels for operands that are not 16-B aligned.
static dim3 unaligned_grid(int64_t n) { return dim3((uint32_t)std::min<int64_t>(blocks_for(n), 8192)); }

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

// One single-learner average or lerp over a contiguous peer payload (k_lerp), as the entry points below describe
// it: which form, what is averaged, where the coefficients come from (COEF_*), `oop` (resident: the result goes
// to args.snap only), the operands, and what the form adds -- `acc` (tracked), `rec` (guarded).
enum class SpanForm { plain, tracked, guarded };
struct SpanAverage {
    SpanForm form;
    const Elems &e;
    int mode;
    bool oop;
    void *param;
    const void *peer;
    LerpArgs args;
    double *acc;
    dpwa_heal_record *rec;
    hipStream_t s;
    const LaunchTiming *timing;
};

// What each path to k_lerp launches and refuses (one dtype / segmented: Elems; a valid layout is never empty, so
// n == 0 is a single-dtype case).  Refusals are hipErrorInvalidValue with nothing queued.
//
//   path                    | coefficients | lanes        | policy table (requested)          resident (oop)
//   plain, one dtype        | host/dev/fus.| lerp_block() | Lerp64- / LerpWidePolicies (bytes)  ResidentPolicies (knob)
//   plain, segmented        | dev / fused  | 64           | BySizePolicies (bytes)              kProductPolicy, fixed
//   tracked, one dtype      | fused        | 64           | BySizePolicies (bytes)              kProductPolicy, fixed
//   guarded, either payload | dev / fused  | 64           | BySizePolicies (bytes)              kProductPolicy, fixed
//
//   path                    | n == 0             | misaligned operand     | null param / peer | spans > 2^31 - 1
//   plain, one dtype        | fused: launched *  | k_lerp_unaligned **    | launched          | launched
//   plain, one dtype, oop   | launched           | refused                | launched          | launched
//   plain, segmented        | --                 | refused                | refused           | refused
//   tracked, one dtype      | launched           | refused                | launched          | refused
//   guarded, one dtype      | fused: launched *  | refused                | refused if n > 0  | refused
//   guarded, segmented      | --                 | refused                | refused           | refused
//   *  host and device coefficients: success with no launch, before the dtype is looked at
//   ** never timed
//
// Every path refuses n < 0, an unknown dtype, a segmented payload without a valid layout, `oop` without args.snap
// when n > 0, and coefficients its form has no kernel for; tracked refuses no `acc`, guarded no `rec` or one not
// 8-B aligned.  DUAL is args.snap != null of a fused launch, and always of an `oop` one.
//
// The form's trailing kernel arguments, then the launch of <Ops, that form>: coefficients, lanes, policy.
template <class Ops, class... Table> static hipError_t launch_spans(const SpanAverage &l, int64_t n, const Table &...table)
{
    const auto launch_form = [&](const auto &...form) -> hipError_t {
        constexpr bool kSolo = sizeof...(Table) + sizeof...(form) == 0;   // k_lerp's own argument list
        constexpr bool kTracked = (std::is_same_v<std::decay_t<decltype(form)>, DistTrack> || ...);
        const auto shaped = [&](auto mode, auto dual, auto oop) -> hipError_t {
            constexpr int MODE = decltype(mode)::value;
            constexpr bool DUAL = decltype(dual)::value, OOP = decltype(oop)::value;
            if constexpr ((MODE == COEF_HOST && !kSolo) || (MODE != COEF_FUSED && kTracked)) {
                return hipErrorInvalidValue;   // (no such kernel)
            } else {
                if constexpr (kSolo && !OOP)
                    if (!aligned16(l.param) || !aligned16(l.peer) || !aligned16(l.args.snap))
                        return launch(k_lerp_unaligned<Ops, MODE, DUAL>, unaligned_grid(n), dim3(kBlock), l.s, nullptr,
                                      l.param, l.peer, n, l.args);
                using Blocks = std::conditional_t<kSolo && !OOP, Choice<256, 64, 128, 512>, Choice<kStreamBlock>>;
                return Blocks::with(lerp_block(), [&](auto block) {
                    constexpr int BLOCK = decltype(block)::value;
                    using Sized = std::conditional_t<!kSolo, BySizePolicies,
                                                     std::conditional_t<BLOCK == 64, Lerp64Policies, LerpWidePolicies>>;
                    using Policies = std::conditional_t<!OOP, Sized, std::conditional_t<kSolo, ResidentPolicies, Choice<kProductPolicy>>>;
                    const int64_t grid = span_grid<Ops>(n, BLOCK);
                    if (!kSolo && grid > 0x7fffffffLL) return hipErrorInvalidValue;
                    return Policies::with(OOP ? lerp_policy() : lerp_policy(n * (16 / Ops::PER)), [&](auto policy) {
                        return launch(k_lerp<Ops, MODE, DUAL, BLOCK, decltype(policy)::value, OOP, Table...,
                                             std::decay_t<decltype(form)>...>,
                                      dim3((uint32_t)grid), dim3(BLOCK), l.s, l.timing, l.param, l.peer, n, l.args, table...,
                                      form...);
                    });
                });
            }
        };
        using std::false_type, std::true_type;
        if (l.mode == COEF_HOST) return shaped(std::integral_constant<int, COEF_HOST>{}, false_type{}, false_type{});
        if (l.mode == COEF_DEV) return shaped(std::integral_constant<int, COEF_DEV>{}, false_type{}, false_type{});
        const std::integral_constant<int, COEF_FUSED> fused;
        if (l.oop) return shaped(fused, true_type{}, true_type{});
        return l.args.snap ? shaped(fused, true_type{}, false_type{}) : shaped(fused, false_type{}, false_type{});
    };
    switch (l.form) {
    case SpanForm::plain: return launch_form();
    case SpanForm::guarded: return launch_form(HealGuard{l.rec});
    case SpanForm::tracked:
        if constexpr (sizeof...(Table) == 0) return launch_form(DistTrack{l.acc});   // (a single dtype only)
    }
    return hipErrorInvalidValue;
}

static hipError_t launch_span_average(const SpanAverage &l)
{
    const bool segmented = l.e.segmented(), plain = l.form == SpanForm::plain;
    const bool some = segmented || l.e.n > 0;
    if (l.form == SpanForm::tracked && !l.acc) return hipErrorInvalidValue;
    if (l.form == SpanForm::guarded && (!l.rec || ((uintptr_t)l.rec & 7))) return hipErrorInvalidValue;
    if (!segmented && l.e.n < 0) return hipErrorInvalidValue;
    if ((segmented || l.oop || !plain) && (!aligned16(l.param) || !aligned16(l.peer) || !aligned16(l.args.snap)))
        return hipErrorInvalidValue;   // (else: k_lerp_unaligned)
    if (l.oop && !l.args.snap && some) return hipErrorInvalidValue;
    if ((segmented || l.form == SpanForm::guarded) && some && (!l.param || !l.peer)) return hipErrorInvalidValue;
    if (segmented)
        return with_segments(l.e, false, [&](int64_t total, dim3, const SegTable &t) { return launch_spans<OpsMixed>(l, total, t); });
    if (l.e.n == 0 && l.mode != COEF_FUSED) return hipSuccess;
    return with_ops(l.e.dtype, [&](auto ops) { return launch_spans<decltype(ops)>(l, l.e.n); });
}

static LerpArgs fused_lerp_args(const FusedArgs &fa, void *snap)
{
    LerpArgs args{};
    args.fused = fa;
    args.snap = snap;
    return args;
}

hipError_t launch_lerp(const Elems &e, void *param, const void *peer, const dpwa_coef *coef, float a, float b,
                       hipStream_t s)
{
    LerpArgs args{};
    args.a = a;
    args.b = b;
    args.coef = coef;
    return launch_span_average({SpanForm::plain, e, coef ? COEF_DEV : COEF_HOST, false, param, peer, args, nullptr, nullptr, s, nullptr});
}

hipError_t launch_average(const Elems &e, void *param, const void *peer, const FusedArgs &fa, void *snap, hipStream_t s,
                          const LaunchTiming *timing, bool oop)
{
    return launch_span_average(
        {SpanForm::plain, e, COEF_FUSED, oop, param, peer, fused_lerp_args(fa, snap), nullptr, nullptr, s, timing});
}

// ---------------------------------------------------------------- distance launches
hipError_t launch_average_tracked(int32_t dtype, void *param, const void *peer, int64_t n, const FusedArgs &fa,
                                  void *snap, bool oop, double *acc, hipStream_t s, const LaunchTiming *timing)
{
    const Elems e{dtype, n, nullptr};
    return launch_span_average(
        {SpanForm::tracked, e, COEF_FUSED, oop, param, peer, fused_lerp_args(fa, snap), acc, nullptr, s, timing});
}

// ---------------------------------------------------------------- guarded (healing) launches
hipError_t launch_average_guarded(const Elems &e, void *param, const void *peer, const FusedArgs &fa, void *snap,
                                  dpwa_heal_record *rec, hipStream_t s, const LaunchTiming *timing, bool oop)
{
    return launch_span_average(
        {SpanForm::guarded, e, COEF_FUSED, oop, param, peer, fused_lerp_args(fa, snap), nullptr, rec, s, timing});
}

hipError_t launch_lerp_guarded(const Elems &e, void *param, const void *peer, const dpwa_coef *coef,
                               dpwa_heal_record *rec, hipStream_t s)
{
    if (!coef) return hipErrorInvalidValue;
    LerpArgs args{};
    args.coef = coef;
    return launch_span_average({SpanForm::guarded, e, COEF_DEV, false, param, peer, args, nullptr, rec, s, nullptr});
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
// from the span's byte offset after the loads were issued (as the segmented k_lerp); no ragged tail;
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

// ---- the trimmed consensus (include/dpwa_hip.h dpwa_consensus_trimmed, where the rule is fixed to the bit)
// The centre of U = 3..8 members with the t smallest and t largest values of every element dropped,
// 1 <= t <= (U - 1) / 2 (the median at the upper end), and every sum against that centre:
//   key(x) = bits ^ (sign ? all-ones : sign-bit), compared unsigned: -NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN
//   y_0 <= .. <= y_{U-1}   the U values in key order (equal keys are equal bits: ties need no rule)
//   s = ((y_t + y_{t+1}) + ..) + y_{U-t-1}    widened exactly to fp64, fp64 adds, ascending
//   m = s * r              r = 1.0 / (U - 2t) from the host;  out = f32(m), then cons_pack: the mean's two roundings
//   norm2 += m * m         spread2_i += (x_i - m) * (x_i - m) for EVERY member i, trimmed or not
// k_consensus's shape (spans, loads first, one store, zeros past the end, tail in workgroup 0, commit);
// what is new sits between the loads and the sums, one dword of every member at a time, all in VGPRs:
//   keys     fp32: v_ashrrev_i32, v_or, v_xor.  bf16 / fp16: the same three PACKED 16-bit instructions on the
//            dword, so both elements of a dword are keyed -- and then sorted -- at once (widening a 16-bit
//            value to fp32 is monotone in the key order, so the 16-bit key orders as the fp32 one would)
//   sort     a fixed compare-exchange network of optimal size (3, 5, 9, 12, 16, 19 exchanges for
//            U = 3..8), fully unrolled: one v_min_u32 / v_max_u32 pair per exchange, or one
//            v_pk_min_u16 / v_pk_max_u16 pair for two elements.  No LDS, no cross-lane traffic, no
//            branch on data.  U = 3 fp32 needs the median only: one v_med3_u32, no network
//   values   the inverse xor, and only y_1 .. y_{U-2} are widened: y_0 and y_{U-1} are trimmed by every t
//   sum      t is a kernel argument (uniform), not a template argument: the middle values every t keeps
//            are added unconditionally, the others under the uniform predicate t <= i < U - t, from
//            s = -0.0 -- (-0.0) + x is x to the bit for every x, -0.0 and NaN included
// A lane past the end holds zeros in every member: their centre is +0.0 and every term is 0.
typedef uint16_t u16x2v __attribute__((ext_vector_type(2)));
typedef int16_t i16x2v __attribute__((ext_vector_type(2)));

struct CxPair { int a, b; };
template <int U> struct SortNet;
template <> struct SortNet<3> { static constexpr CxPair cx[3] = {{0, 2}, {0, 1}, {1, 2}}; };
template <> struct SortNet<4> { static constexpr CxPair cx[5] = {{0, 2}, {1, 3}, {0, 1}, {2, 3}, {1, 2}}; };
template <> struct SortNet<5> {
    static constexpr CxPair cx[9] = {{0, 3}, {1, 4}, {0, 2}, {1, 3}, {0, 1}, {2, 4}, {1, 2}, {3, 4}, {2, 3}};
};
template <> struct SortNet<6> {
    static constexpr CxPair cx[12] = {{0, 5}, {1, 3}, {2, 4}, {1, 2}, {3, 4}, {0, 3}, {2, 5}, {0, 1}, {2, 3}, {4, 5}, {1, 2},
                                      {3, 4}};
};
template <> struct SortNet<7> {
    static constexpr CxPair cx[16] = {{0, 6}, {2, 3}, {4, 5}, {0, 2}, {1, 4}, {3, 6}, {0, 1}, {2, 5},
                                      {3, 4}, {1, 2}, {4, 6}, {2, 3}, {4, 5}, {1, 2}, {3, 4}, {5, 6}};
};
template <> struct SortNet<8> {
    static constexpr CxPair cx[19] = {{0, 2}, {1, 3}, {4, 6}, {5, 7}, {0, 4}, {1, 5}, {2, 6}, {3, 7}, {0, 1}, {2, 3},
                                      {4, 5}, {6, 7}, {2, 4}, {3, 5}, {1, 4}, {3, 6}, {1, 2}, {3, 4}, {5, 6}};
};

// The zero-one principle, at compile time: a network that sorts every 0/1 input sorts every input.
template <int U> constexpr bool sorts_every_input()
{
    for (unsigned in = 0; in < (1u << U); ++in) {
        unsigned v = in;
        for (const CxPair &p : SortNet<U>::cx) {
            const unsigned a = (v >> p.a) & 1, b = (v >> p.b) & 1;
            v = (v & ~((1u << p.a) | (1u << p.b))) | ((a & b) << p.a) | ((a | b) << p.b);
        }
        for (int i = 0; i + 1 < U; ++i)
            if (((v >> i) & 1) > ((v >> (i + 1)) & 1)) return false;
    }
    return true;
}
static_assert(sorts_every_input<3>() && sorts_every_input<4>() && sorts_every_input<5>() && sorts_every_input<6>() &&
                  sorts_every_input<7>() && sorts_every_input<8>(),
              "a consensus network does not sort");

// A dword of the payload -> its key(s) and back; the exchange.  16-bit types: both halves at once.
__device__ __forceinline__ uint32_t trim_key(OpsF32, uint32_t w) { return w ^ ((uint32_t)((int32_t)w >> 31) | 0x80000000u); }
__device__ __forceinline__ uint32_t trim_unkey(OpsF32, uint32_t k) { return k ^ ((uint32_t)((int32_t)~k >> 31) | 0x80000000u); }
__device__ __forceinline__ void trim_cx(OpsF32, uint32_t &a, uint32_t &b)
{
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}
__device__ __forceinline__ uint32_t trim_key16(uint32_t w)
{
    const u16x2v m = __builtin_bit_cast(u16x2v, __builtin_bit_cast(i16x2v, w) >> 15) | (uint16_t)0x8000;
    return w ^ __builtin_bit_cast(uint32_t, m);
}
__device__ __forceinline__ void trim_cx16(uint32_t &a, uint32_t &b)
{
    const u16x2v x = __builtin_bit_cast(u16x2v, a), y = __builtin_bit_cast(u16x2v, b);
    a = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(x, y));
    b = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(x, y));
}
__device__ __forceinline__ uint32_t trim_key(OpsBF16, uint32_t w) { return trim_key16(w); }
__device__ __forceinline__ uint32_t trim_key(OpsF16, uint32_t w) { return trim_key16(w); }
__device__ __forceinline__ uint32_t trim_unkey16(uint32_t k)
{
    const u16x2v m = __builtin_bit_cast(u16x2v, __builtin_bit_cast(i16x2v, ~k) >> 15) | (uint16_t)0x8000;
    return k ^ __builtin_bit_cast(uint32_t, m);
}
__device__ __forceinline__ uint32_t trim_unkey(OpsBF16, uint32_t k) { return trim_unkey16(k); }
__device__ __forceinline__ uint32_t trim_unkey(OpsF16, uint32_t k) { return trim_unkey16(k); }
__device__ __forceinline__ void trim_cx(OpsBF16, uint32_t &a, uint32_t &b) { trim_cx16(a, b); }
__device__ __forceinline__ void trim_cx(OpsF16, uint32_t &a, uint32_t &b) { trim_cx16(a, b); }

// the network of U over y, every index a constant
template <class Ops, int U, size_t... J>
__device__ __forceinline__ void trim_sort(uint32_t (&y)[U], std::index_sequence<J...>)
{
    (trim_cx(Ops{}, y[SortNet<U>::cx[J].a], y[SortNet<U>::cx[J].b]), ...);
}

// element h of a payload dword, widened exactly to fp64 (h = 0 for fp32)
__device__ __forceinline__ double cons_word(OpsF32, uint32_t w, int) { return (double)__uint_as_float(w); }
__device__ __forceinline__ double cons_word(OpsBF16, uint32_t w, int h) { return (double)(h ? bf_hi(w) : bf_lo(w)); }
__device__ __forceinline__ double cons_word(OpsF16, uint32_t w, int h)
{
    const f16x2v v = __builtin_bit_cast(f16x2v, w);
    return (double)(h ? v.y : v.x);
}

// One dword of every member, in member order: its H elements' centres into f[0..H), TRACK: their terms.
template <class Ops, int U, bool TRACK, int H>
__device__ __forceinline__ void trim_word(const uint32_t (&w)[U], int t, double r, float *f, double &n2, double (&sp)[U])
{
    constexpr int TMAX = (U - 1) / 2;   // y_i with TMAX <= i < U - TMAX is kept whatever t
    uint32_t y[U];
    if constexpr (U == 3 && std::is_same<Ops, OpsF32>::value) {
        const uint32_t a = trim_key(Ops{}, w[0]), b = trim_key(Ops{}, w[1]), c = trim_key(Ops{}, w[2]);
        const uint32_t lo = a < b ? a : b, hi = a < b ? b : a, up = lo < c ? c : lo;   // max(min(a, b), c)
        y[1] = trim_unkey(Ops{}, hi < up ? hi : up);                                  // v_med3_u32
    } else {
#pragma unroll
        for (int i = 0; i < U; ++i) y[i] = trim_key(Ops{}, w[i]);
        trim_sort<Ops, U>(y, std::make_index_sequence<sizeof(SortNet<U>::cx) / sizeof(CxPair)>{});
#pragma unroll
        for (int i = 1; i < U - 1; ++i) y[i] = trim_unkey(Ops{}, y[i]);
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
        double s = -0.0;
#pragma unroll
        for (int i = 1; i < U - 1; ++i) {
            const double v = cons_word(Ops{}, y[i], h);
            if (i >= TMAX && i < U - TMAX) s = s + v;
            else s = (i >= t && i < U - t) ? s + v : s;
        }
        const double m = s * r;
        if constexpr (TRACK) {
            n2 = n2 + m * m;
#pragma unroll
            for (int i = 0; i < U; ++i) {
                const double d = cons_word(Ops{}, w[i], h) - m;
                sp[i] = sp[i] + d * d;
            }
        }
        f[h] = (float)m;
    }
}

// A lane's item of every member -> the item of the centre.
template <class Ops, int U, bool TRACK>
__device__ __forceinline__ u32x4 trim_item(const u32x4 (&v)[U], int t, double r, double &n2, double (&sp)[U])
{
    constexpr int H = Ops::PER / 4;
    float f[Ops::PER];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        uint32_t w[U];
#pragma unroll
        for (int i = 0; i < U; ++i) w[i] = v[i][d];
        trim_word<Ops, U, TRACK, H>(w, t, r, f + d * H, n2, sp);
    }
    return cons_pack(Ops{}, f);
}

template <class Ops, int U, bool STORE, bool TRACK>
__global__ __launch_bounds__(kStreamBlock) void k_consensus_trimmed(ConsensusArgs a, int64_t n, int t)
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
    __builtin_amdgcn_sched_barrier(0);
    [[maybe_unused]] double n2 = 0.0, sp[U];
#pragma unroll
    for (int i = 0; i < U; ++i) sp[i] = 0.0;
    const u32x4 centre = trim_item<Ops, U, TRACK>(v, t, a.r, n2, sp);
    if constexpr (STORE) span_store<u32x4>(span_rsrc<SPAN>(a.out, off, vbytes), lane_off, centre);
    const int64_t tail = n / Ops::PER * Ops::PER;
    if (blockIdx.x == 0 && threadIdx.x < n - tail) {   // one element in the low half of a dword; the other half zeros
        const int64_t j = tail + threadIdx.x;
        uint32_t w[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const S x = reinterpret_cast<const S *>(a.src[i])[j];
            if constexpr (sizeof(S) == 4) w[i] = __float_as_uint(x);
            else w[i] = x;
        }
        float f;
        trim_word<Ops, U, TRACK, 1>(w, t, a.r, &f, n2, sp);
        if constexpr (STORE) reinterpret_cast<S *>(a.out)[j] = cons_pack_s(Ops{}, f);
    }
    if constexpr (TRACK) cons_commit<U>(a.acc, blockIdx.x, n2, sp);
}

// Over a segmented payload, as k_consensus_mixed: the span's element type under a uniform branch.
template <int U, bool STORE, bool TRACK>
__global__ __launch_bounds__(kStreamBlock) void k_consensus_trimmed_mixed(ConsensusArgs a, int64_t total, SegTable segs, int t)
{
    constexpr int SPAN = kStreamBlock * 16;
    const int64_t off = (int64_t)blockIdx.x * SPAN;
    const int lane_off = threadIdx.x * 16;
    u32x4 v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = span_load<u32x4>(span_rsrc<SPAN>(a.src[j], off, total), lane_off);
    __builtin_amdgcn_sched_barrier(0);
    [[maybe_unused]] double n2 = 0.0, sp[U];
#pragma unroll
    for (int i = 0; i < U; ++i) sp[i] = 0.0;
    const int32_t dtype = seg_dtype(segs, off);
    u32x4 centre;
    if (dtype == DPWA_F32) centre = trim_item<OpsF32, U, TRACK>(v, t, a.r, n2, sp);
    else if (dtype == DPWA_BF16) centre = trim_item<OpsBF16, U, TRACK>(v, t, a.r, n2, sp);
    else centre = trim_item<OpsF16, U, TRACK>(v, t, a.r, n2, sp);
    if constexpr (STORE) span_store<u32x4>(span_rsrc<SPAN>(a.out, off, total), lane_off, centre);
    if constexpr (TRACK) cons_commit<U>(a.acc, blockIdx.x, n2, sp);
}

// Finishing (one workgroup behind the pass on the same stream, as k_distance_finish): lane i loads
// and zeroes row i, the sums are taken in a fixed order -- the butterfly inside each wave, then the
// waves in order, then spread2 over the members in order -- and the record is written whole
// (`reserved`: the trim of a trimmed pass, 0 from the mean's).
constexpr int kConsensusSums = kMaxConsensus + 1;

__global__ __launch_bounds__(kDistFinishBlock) void k_consensus_finish(double *__restrict__ acc,
                                                                       dpwa_consensus_record *__restrict__ out, int64_t n,
                                                                       int32_t members, uint64_t version, int32_t reserved)
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
    out->reserved = reserved;
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

// What launch_consensus and launch_consensus_trimmed refuse alike; accepted, the kernels' arguments in `a`.
static bool consensus_args(const Elems &e, const void *const *src, int count, double r, void *out, double *acc,
                           ConsensusArgs &a)
{
    if (count < 1 || count > kMaxConsensus || !src || (!out && !acc) || !aligned16(out, acc)) return false;
    if (!e.segmented() && (e.n < 0 || !is_float_dtype(e.dtype))) return false;
    if (e.segmented() && (!e.layout || layout_problem(*e.layout, -1))) return false;
    const int64_t bytes = e.segmented() ? layout_bytes(*e.layout) : e.bytes();
    for (int i = 0; i < count; ++i) {
        if (absent_or_unaligned(src[i]) || (out && (src[i] == out || overlaps(src[i], out, bytes)))) return false;
        a.src[i] = src[i];
    }
    a.out = out;
    a.acc = acc;
    a.r = r;
    return true;
}

hipError_t launch_consensus(const Elems &e, const void *const *src, int count, double r, void *out, double *acc,
                            bool remote, hipStream_t s, const LaunchTiming *timing)
{
    ConsensusArgs a{};
    if (!consensus_args(e, src, count, r, out, acc, a)) return hipErrorInvalidValue;
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

hipError_t launch_consensus_trimmed(const Elems &e, const void *const *src, int count, int trim, double r, void *out,
                                    double *acc, bool remote, hipStream_t s, const LaunchTiming *timing)
{
    ConsensusArgs a{};
    if (count < 3 || trim < 1 || 2 * trim >= count || !consensus_args(e, src, count, r, out, acc, a))
        return hipErrorInvalidValue;
    const bool store = out != nullptr, track = acc != nullptr;
    const auto acquire = [&] {   // (after every refusal: a refused launch queues nothing)
        if (remote) hipLaunchKernelGGL(k_acquire_system, dim3(256), dim3(64), 0, s);
    };
    return Choice<3, 4, 5, 6, 7, 8>::with(count, [&](auto members) {
        constexpr int U = decltype(members)::value;
        if (e.segmented())
            return with_segments(e, false, [&](int64_t total, dim3 grid, const SegTable &tab) {
                acquire();
                return launch(store ? (track ? k_consensus_trimmed_mixed<U, true, true> : k_consensus_trimmed_mixed<U, true, false>)
                                    : k_consensus_trimmed_mixed<U, false, true>,
                              grid, dim3(kStreamBlock), s, timing, a, total, tab, trim);
            });
        if (e.n == 0) return hipSuccess;
        return with_ops(e.dtype, [&](auto ops) {
            using Ops = decltype(ops);
            if (span_grid<Ops>(e.n, kStreamBlock) > 0x7fffffffLL) return hipErrorInvalidValue;
            acquire();
            return launch(store ? (track ? k_consensus_trimmed<Ops, U, true, true> : k_consensus_trimmed<Ops, U, true, false>)
                                : k_consensus_trimmed<Ops, U, false, true>,
                          dim3((uint32_t)span_grid<Ops>(e.n, kStreamBlock)), dim3(kStreamBlock), s, timing, a, e.n, trim);
        });
    });
}

hipError_t launch_consensus_finish(double *acc, dpwa_consensus_record *out, int64_t n, int members, uint64_t version,
                                   hipStream_t s, const LaunchTiming *timing, int reserved)
{
    if (!acc || !out || members < 1 || members > kMaxConsensus || n < 0 || reserved < 0) return hipErrorInvalidValue;
    return launch(k_consensus_finish, dim3(1), dim3(kDistFinishBlock), s, timing, acc, out, n, members, version, reserved);
}

// ---------------------------------------------------------------- packed snapshots
// Opt-in (include/dpwa_hip.h "packed snapshots", where the codec is fixed to the bit): the publisher
// keeps an int8 block-scaled image of each snapshot (k_pack), and a puller reads that image instead
// of the payload and expands it on arrival (k_pull_unpack), so 68 B (fp32) or 132 B (bf16 / fp16)
// cross the link for every 256 B of payload.
//
// How the work is split, both ways: one wave owns one 4-KiB payload block and lane l owns its bytes
// [64 l, 64 l + 64) -- four 16-byte items -- so the q bytes of a lane are contiguous (16 for fp32, 32
// for the 16-bit types) and a 256-byte group is exactly the four lanes of a quad.  What a group shares
// (amax and the non-finite flag on the way in, the scale on the way out) therefore never leaves the
// quad: two DPP quad_perm moves, no LDS memory and no ds_bpermute.  The payload side goes through
// buffer descriptors ranged to the payload's whole 16-byte items, as every streaming kernel's: lanes
// past the end load zeros and their stores are dropped, so slots need not be zero behind the payload.
// The image side needs no range: both planes are padded to whole blocks.  The ragged item of a payload
// that is no multiple of 16 bytes is read and written 2 bytes at a time by the one lane that owns it.
// Both kernels keep one fp32 multiply per lane and element: no packed fp32 instructions (device pass only;
// the host pass knows no such target feature).
#if defined(__HIP_DEVICE_COMPILE__)
#define DPWA_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define DPWA_NO_PK_F32
#endif
constexpr int kPackBlock = 4096;        // payload bytes per wave
constexpr int kPackLane = 64;           // payload bytes per lane
constexpr int kPackScales = kPackBlock / 256;   // groups, and scales, per block
constexpr int kPackIfBlocks = 2048;     // k_pack_if's grid at most: 8 waves a CU
static_assert(kPackBlock == kStreamBlock * kPackLane && kPackLane == 4 * 16, "a lane owns four 16-byte items");

// Bit casts as builtins: the two kernels carry a target attribute, and a helper of another feature set (the
// HIP headers' __float_as_uint, bf_lo above) is not inlined into them but called.
__device__ __forceinline__ uint32_t pk_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ float pk_float(uint32_t w) { return __builtin_bit_cast(float, w); }

// One 16-byte item widened exactly to fp32, elements in payload order, and fp32 values rounded back to one.
__device__ __forceinline__ void pack_widen(OpsF32, u32x4 v, float *x)
{
    x[0] = pk_float(v.x), x[1] = pk_float(v.y), x[2] = pk_float(v.z), x[3] = pk_float(v.w);
}
__device__ __forceinline__ void pack_widen(OpsBF16, u32x4 v, float *x)
{
    x[0] = pk_float(v.x << 16), x[1] = pk_float(v.x & 0xffff0000u), x[2] = pk_float(v.y << 16);
    x[3] = pk_float(v.y & 0xffff0000u), x[4] = pk_float(v.z << 16), x[5] = pk_float(v.z & 0xffff0000u);
    x[6] = pk_float(v.w << 16), x[7] = pk_float(v.w & 0xffff0000u);
}
__device__ __forceinline__ void pack_widen(OpsF16, u32x4 v, float *x)
{
    const float2v a = unpk_f16(v.x), b = unpk_f16(v.y), c = unpk_f16(v.z), d = unpk_f16(v.w);
    x[0] = a.x, x[1] = a.y, x[2] = b.x, x[3] = b.y, x[4] = c.x, x[5] = c.y, x[6] = d.x, x[7] = d.y;
}
__device__ __forceinline__ u32x4 pack_narrow(OpsF32, const float *x)
{
    return u32x4{pk_bits(x[0]), pk_bits(x[1]), pk_bits(x[2]), pk_bits(x[3])};
}
__device__ __forceinline__ u32x4 pack_narrow(OpsBF16, const float *x)
{
    return u32x4{pk_bf16(x[0], x[1]), pk_bf16(x[2], x[3]), pk_bf16(x[4], x[5]), pk_bf16(x[6], x[7])};
}
__device__ __forceinline__ u32x4 pack_narrow(OpsF16, const float *x)
{
    return u32x4{pk_f16(x[0], x[1]), pk_f16(x[2], x[3]), pk_f16(x[4], x[5]), pk_f16(x[6], x[7])};
}

// The unsigned maximum over the four lanes of a quad, the same in all four: lane ^ 1 then lane ^ 2,
// quad_perm [1,0,3,2] and [2,3,0,1].  Every lane of the wave is active where this is called.
__device__ __forceinline__ uint32_t quad_umax(uint32_t v)
{
    uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
    v = v > o ? v : o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
    return v > o ? v : o;
}

// Where the ragged item of a payload lies for the wave of block `off`: the lane and the item of that lane
// (ragged_at), or lane -1 when the block has none.  Uniform.
struct Ragged {
    int lane, item, bytes;
};
__device__ __forceinline__ Ragged ragged_at(int64_t off, int64_t nbytes)
{
    const int64_t at = (nbytes & ~(int64_t)15) - off;
    const int rem = (int)(nbytes & 15);
    if (!rem || at < 0 || at >= kPackBlock) return Ragged{-1, 0, 0};
    return Ragged{(int)at / kPackLane, ((int)at % kPackLane) / 16, rem};
}

// q = clamp(rint(x * inv), -127, 127) as the low byte of the result.
__device__ __forceinline__ uint32_t pack_q(float x, float inv)
{
    float r = __builtin_rintf(x * inv);   // v_rndne_f32
    r = __builtin_fminf(__builtin_fmaxf(r, -127.0f), 127.0f);
    return (uint32_t)(int)r & 0xffu;
}

// pack_q's stochastic sibling (include/dpwa_hip.h "stochastic rounding"): floor(t) plus one where the
// element's noise u in [0, 1) lies below frac(t).  t, f and frac are three separately rounded operations
// (v_mul_f32, v_floor_f32, v_sub_f32); f is an integer of [-128, 127], so f + 1.0f is the integer sum.
// A zero gives frac = 0 and stays 0 whatever u is.
__device__ __forceinline__ uint32_t pack_q_sr(float x, float inv, float u)
{
    const float t = x * inv;
    const float f = __builtin_floorf(t);
    const float frac = t - f;
    float r = f + (u < frac ? 1.0f : 0.0f);
    r = __builtin_fminf(__builtin_fmaxf(r, -127.0f), 127.0f);
    return (uint32_t)(int)r & 0xffu;
}

// murmur3's 32-bit finaliser: two multiplies and three shift-xors, all uint32.
__device__ __forceinline__ uint32_t fmix32(uint32_t h)
{
    h ^= h >> 16, h *= 0x85ebca6bu, h ^= h >> 13, h *= 0xc2b2ae35u, h ^= h >> 16;
    return h;
}

// How an image-writing kernel rounds (k_pack, k_pack_if, k_lerp_emit): a policy object that travels as the
// kernel's last argument.  noise<E>(j0) is what the lane needs for its E elements j0 .. j0 + E - 1 before it
// knows anything about their values, and Noise::q(e, x, inv) the q byte of element e.  RoundNearest holds
// nothing and q is pack_q: those instantiations have no branch on the policy and are the kernels as they
// were, instruction for instruction (gfx950: k_pack_if and k_lerp_emit to the register; k_pack's one-byte
// argument moved its allocation by one VGPR, 24 / 51 / 41 for 23 / 50 / 40, the instructions being the same).
// RoundStochastic holds the image's nonce; its noise is the counter-based hash of (element index, nonce) of
// the header's rule, two fmix32 per element in registers -- no memory, no LDS, no state -- and since it
// depends on indices and the nonce alone every caller asks for it right behind its loads, ahead of the
// cross-lane amax, so the integer pipe can work while the loads are in flight (k_pack's does; in k_lerp_emit
// the compiler sinks it below the factor's branch, ahead of row_umax -- DESIGN §3).  j0 is a multiple of E and E a
// power of two, so element e's index is j0 | e: the high word, and with it hi, is the lane's one value (in
// fact the wave's) and the low words differ in the low bits only.
struct RoundNearest {
    template <int E> struct Noise {
        __device__ __forceinline__ uint32_t q(int, float x, float inv) const { return pack_q(x, inv); }
    };
    template <int E> __device__ __forceinline__ Noise<E> noise(uint64_t) const { return {}; }
};
struct RoundStochastic {
    uint64_t nonce;
    template <int E> struct Noise {
        float u[E];
        __device__ __forceinline__ uint32_t q(int e, float x, float inv) const { return pack_q_sr(x, inv, u[e]); }
    };
    template <int E> __device__ __forceinline__ Noise<E> noise(uint64_t j0) const
    {
        static_assert((E & (E - 1)) == 0, "the lane's elements share all index bits above log2 E");
        const uint32_t lo = (uint32_t)j0 ^ (uint32_t)nonce;
        const uint32_t hi = (uint32_t)(j0 >> 32) ^ (uint32_t)(nonce >> 32);
        Noise<E> z;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t h = fmix32(fmix32(lo ^ (uint32_t)e) ^ hi);
            z.u[e] = (float)(h >> 8) * 0x1p-24f;   // 24 bits: the conversion and the product are exact
        }
        return z;
    }
};

// One wave packs payload block `blk`.
template <class Ops, class Round>
DPWA_NO_PK_F32 __device__ __forceinline__ void pack_block(int64_t blk, const char *__restrict__ payload, int64_t nbytes,
                                                          char *__restrict__ q_plane, float *__restrict__ scales,
                                                          const Round &round)
{
    constexpr int PER = Ops::PER;          // elements of a 16-byte item
    constexpr int QB = 4 * PER;            // q bytes of a lane
    const int lane = threadIdx.x;
    const int64_t off = blk * kPackBlock;
    const __amdgpu_buffer_rsrc_t r = span_rsrc<kPackBlock>(payload, off, nbytes & ~(int64_t)15);
    // the payload was just written by the publish or the average: the default cache policy
    u32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = span_load<u32x4, 0>(r, lane * kPackLane + j * 16);
    // (the lane's first element, counted from the payload's first: 4 PER elements a lane)
    const auto noise = round.template noise<4 * PER>((uint64_t)(blk * kStreamBlock + lane) * (4 * PER));
    const Ragged rg = ragged_at(off, nbytes);
    if (rg.lane == lane) {
        const uint16_t *p = reinterpret_cast<const uint16_t *>(payload + (nbytes & ~(int64_t)15));
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 7; ++i)
            if (2 * i < rg.bytes) w[i / 2] |= (uint32_t)p[i] << (16 * (i & 1));
        const u32x4 t{w[0], w[1], w[2], w[3]};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (rg.item == j) v[j] = t;
    }
    float x[4 * PER];
#pragma unroll
    for (int j = 0; j < 4; ++j) pack_widen(Ops{}, v[j], x + j * PER);
    // amax as the unsigned maximum of the |x| bit patterns: that of the values when all are finite, and
    // at or above the exponent mask exactly when one is a NaN or an inf (k_peer_finite's test)
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 4 * PER; ++e) {
        const uint32_t a = pk_bits(x[e]) & 0x7fffffffu;
        m = m > a ? m : a;
    }
    m = quad_umax(m);
    const bool nonfinite = m >= 0x7f800000u;
    const float amax = pk_float(m);
    const bool normal = !nonfinite && amax >= 0x1p-100f;
    const float den = normal ? amax : 1.0f;
    const float inv = 127.0f / den;                  // the two divisions, once per lane
    const float scale = nonfinite ? pk_float(0x7fc00000u) : normal ? den / 127.0f : 0.0f;
    uint32_t q[QB / 4];
#pragma unroll
    for (int d = 0; d < QB / 4; ++d) {
        const uint32_t w = noise.q(4 * d, x[4 * d], inv) | noise.q(4 * d + 1, x[4 * d + 1], inv) << 8 |
                           noise.q(4 * d + 2, x[4 * d + 2], inv) << 16 | noise.q(4 * d + 3, x[4 * d + 3], inv) << 24;
        q[d] = normal ? w : 0u;
    }
    const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
        q_plane + blk * (kStreamBlock * QB), 0, kStreamBlock * QB, 0x00020000);
#pragma unroll
    for (int d = 0; d < QB / 16; ++d)
        span_store(rq, lane * QB + d * 16, u32x4{q[4 * d], q[4 * d + 1], q[4 * d + 2], q[4 * d + 3]});
    if ((lane & 3) == 0) {   // the quad's scale: 16 per wave, 64 contiguous bytes
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            scales + blk * kPackScales, 0, kPackScales * 4, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(pk_bits(scale), rs, lane, 0, kAuxStore);
    }
}

template <class Ops, class Round>
DPWA_NO_PK_F32 __global__ __launch_bounds__(kStreamBlock) void k_pack(const char *__restrict__ payload, int64_t nbytes,
                                                       char *__restrict__ q_plane, float *__restrict__ scales,
                                                       Round round)
{
    pack_block<Ops>((int64_t)blockIdx.x, payload, nbytes, q_plane, scales, round);
}

// k_pack behind the reuse guard of a publish whose image the average wrote: the guard's fix-up, if there was
// one, left that image stale, and its verdict stays on the device.  Every wave returns at once unless the
// verdict word carries this publish's generation; a hit repacks the whole payload, a capped grid striding over
// the blocks as k_pull_unpack's, and a miss moves no payload byte.
template <class Ops, class Round>
DPWA_NO_PK_F32 __global__ __launch_bounds__(kStreamBlock) void k_pack_if(const char *__restrict__ payload, int64_t nbytes,
                                                          char *__restrict__ q_plane, float *__restrict__ scales,
                                                          int64_t nblocks, const int32_t *__restrict__ dirty,
                                                          int32_t gen, Round round)
{
    if (*dirty != gen) return;   // uniform
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x)
        pack_block<Ops>(b, payload, nbytes, q_plane, scales, round);
}

// The mirror image, shaped like k_pull: at most max_blocks one-wave workgroups stride over the blocks.
// The q bytes and the scale are the only reads that cross the link (`nt`: each is read once); workgroup
// 0 also copies the 256-byte header from the peer's slot, exactly.
template <class Ops>
DPWA_NO_PK_F32 __global__ __launch_bounds__(kStreamBlock) void k_pull_unpack(char *__restrict__ dst, int64_t nbytes,
                                                              const char *__restrict__ q_plane,
                                                              const float *__restrict__ scales, int64_t nblocks,
                                                              u32x4 *__restrict__ hdr_dst,
                                                              const u32x4 *__restrict__ hdr_src)
{
    constexpr int PER = Ops::PER;
    constexpr int QB = 4 * PER;
    const int lane = threadIdx.x;
    if (hdr_src && blockIdx.x == 0 && lane < 16) hdr_dst[lane] = __builtin_nontemporal_load(hdr_src + lane);
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int64_t off = b * kPackBlock;
        const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(q_plane + b * (kStreamBlock * QB)), 0, kStreamBlock * QB, 0x00020000);
        u32x4 w[QB / 16];
#pragma unroll
        for (int d = 0; d < QB / 16; ++d) w[d] = span_load<u32x4>(rq, lane * QB + d * 16);
        const float scale = __builtin_nontemporal_load(scales + b * kPackScales + (lane >> 2));
        const __amdgpu_buffer_rsrc_t r = span_rsrc<kPackBlock>(dst, off, nbytes & ~(int64_t)15);
        const Ragged rg = ragged_at(off, nbytes);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x[PER];
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                const int byte = j * PER + e;                        // of the lane's q bytes
                const uint32_t word = w[byte / 16][(byte / 4) % 4];
                const int qv = (int)(word << (24 - 8 * (byte % 4))) >> 24;   // the signed byte
                x[e] = (float)qv * scale;
            }
            const u32x4 out = pack_narrow(Ops{}, x);
            span_store(r, lane * kPackLane + j * 16, out);
            if (rg.lane == lane && rg.item == j) {
                uint16_t *p = reinterpret_cast<uint16_t *>(dst + (nbytes & ~(int64_t)15));
#pragma unroll
                for (int i = 0; i < 7; ++i)
                    if (2 * i < rg.bytes) p[i] = (uint16_t)(out[i / 2] >> (16 * (i & 1)));
            }
        }
    }
}

int64_t pack_blocks(int32_t dtype, int64_t n)
{
    const int64_t bytes = n * (int64_t)dtype_size(dtype);
    return bytes <= 0 ? 1 : (bytes + kPackBlock - 1) / kPackBlock;
}

int64_t pack_scale_offset(int32_t dtype, int64_t n)
{
    const int64_t q = pack_blocks(dtype, n) * (kPackBlock / (int64_t)dtype_size(dtype));
    return (q + 4095) / 4096 * 4096;
}

int64_t pack_image_bytes(int32_t dtype, int64_t n)
{
    return pack_scale_offset(dtype, n) + (pack_blocks(dtype, n) * kPackScales * 4 + 4095) / 4096 * 4096;
}

// A PackRounding as the policy object of the kernels above: f(RoundNearest{}) or f(RoundStochastic{nonce}).
template <class F> static hipError_t with_round(const PackRounding &rounding, F &&f)
{
    return rounding.stochastic ? f(RoundStochastic{rounding.nonce}) : f(RoundNearest{});
}

hipError_t launch_pack(int32_t dtype, const void *payload, int64_t n, void *image, hipStream_t s,
                       const LaunchTiming *timing, PackRounding rounding)
{
    if (!is_float_dtype(dtype) || n < 0 || !payload || !image || !aligned16(payload, image)) return hipErrorInvalidValue;
    const int64_t blocks = pack_blocks(dtype, n);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    return with_ops(dtype, [&](auto ops) {
        return with_round(rounding, [&](auto round) {
            return launch(k_pack<decltype(ops), decltype(round)>, dim3((uint32_t)blocks), dim3(kStreamBlock), s, timing,
                          payload, n * (int64_t)dtype_size(dtype), image, (char *)image + pack_scale_offset(dtype, n),
                          round);
        });
    });
}

hipError_t launch_pack_if(int32_t dtype, const void *payload, int64_t n, void *image, const int32_t *dirty, int32_t gen,
                          hipStream_t s, const LaunchTiming *timing, PackRounding rounding)
{
    if (!is_float_dtype(dtype) || n < 0 || !payload || !image || !dirty || !aligned16(payload, image))
        return hipErrorInvalidValue;
    const int64_t blocks = pack_blocks(dtype, n);
    return with_ops(dtype, [&](auto ops) {
        return with_round(rounding, [&](auto round) {
            return launch(k_pack_if<decltype(ops), decltype(round)>,
                          dim3((uint32_t)std::min<int64_t>(blocks, kPackIfBlocks)), dim3(kStreamBlock), s, timing,
                          payload, n * (int64_t)dtype_size(dtype), image, (char *)image + pack_scale_offset(dtype, n),
                          blocks, dirty, gen, round);
        });
    });
}

hipError_t launch_pull_unpack(int32_t dtype, void *payload_out, int64_t n, const void *image, void *header_out,
                              const void *header, int max_blocks, bool remote, hipStream_t s,
                              const LaunchTiming *timing)
{
    if (!is_float_dtype(dtype) || n < 0 || !payload_out || !image || !aligned16(payload_out, image, header_out, header) ||
        max_blocks < 1 || (!header) != (!header_out))
        return hipErrorInvalidValue;
    if (remote) hipLaunchKernelGGL(k_acquire_system, dim3(256), dim3(64), 0, s);
    const int64_t blocks = pack_blocks(dtype, n);
    return with_ops(dtype, [&](auto ops) {
        return launch(k_pull_unpack<decltype(ops)>, dim3((uint32_t)std::min<int64_t>(blocks, max_blocks)),
                      dim3(kStreamBlock), s, timing, payload_out, n * (int64_t)dtype_size(dtype), image,
                      (const char *)image + pack_scale_offset(dtype, n), blocks, header_out, header);
    });
}

// ---------------------------------------------------------------- the average straight from a packed image
// k_lerp's fused factor + lerp (lerp_span: one-wave workgroups over an exact grid of 1-KiB payload spans,
// a 16-byte item per lane, the parameter load and the two stores through descriptors ranged to the
// payload's whole items, the cache policy by size) with the peer operand dequantised in registers from the
// packed image instead of loaded from a contiguous payload: k_pull_unpack's store and k_lerp's load of the
// same bytes, 2 n s of HBM traffic, drop out of a DPWA_PULL_PACKED_AVG round.
//
// Lane l of span s owns the item at payload byte 1024 s + 16 l.  The q plane holds one byte per element
// in payload order, so its q bytes are the PER bytes at q-plane offset 64 PER s + PER l: one dword (fp32)
// or two (16-bit) per lane, one coalesced 256- or 512-byte `nt` read per wave.  A 256-byte group is 16
// lanes, so the wave needs scales[4 s .. 4 s + 3]: either every lane loads its own (four distinct
// addresses, one 16-byte request per wave), or -- USCALE, the default by measurement -- the four come
// through the wave's one uniform 16-byte load and three selects pick the lane's (DESIGN §3 has the timing
// of both).  No LDS memory.
// The image is padded to whole 4-KiB blocks, so neither plane is range-checked; the grid covers the
// payload's bytes and so never leaves the image.
//
// x' = (float)q * scale is one separately rounded fp32 multiply per element and a 16-bit type rounds it
// with pack_narrow, so the item is, to the bit, what k_pull_unpack would have stored; Ops::lerp is
// unchanged.  The ragged item of a payload that is no multiple of 16 bytes belongs to one lane, which has
// its q bytes and scale in registers anyway: it reads and writes the parameters' elements one by one
// (Ops::lerp_s) and nothing behind the payload's last byte.
template <class V> __device__ __forceinline__ float item_elem(OpsF32, V v, int i) { return v[i]; }
template <class Ops, class V> __device__ __forceinline__ uint16_t item_elem(Ops, V v, int i)
{
    return (uint16_t)(v[i / 2] >> (16 * (i & 1)));
}

// Where the peer's item of a span comes from (packed_span): a contiguous payload, loaded as k_lerp loads it, or
// a packed image, dequantised as above.  load() issues the lane's loads, item() is the lane's 16-byte item and
// ragged() element i of the payload's ragged item, for the lane that owns it.
struct PayloadPeer {
    const char *payload;
    template <class Ops> struct Raw {
        typename Ops::V q;
    };
    template <class Ops> __device__ __forceinline__ Raw<Ops> load(uint32_t span, int lane, int64_t vbytes) const
    {
        constexpr int SPAN = kStreamBlock * 16;
        return Raw<Ops>{span_load<typename Ops::V>(span_rsrc<SPAN>(payload, (int64_t)span * SPAN, vbytes), lane * 16)};
    }
    template <class Ops> __device__ __forceinline__ typename Ops::V item(const Raw<Ops> &raw, int) const { return raw.q; }
    template <class Ops>
    __device__ __forceinline__ typename Ops::S ragged(typename Ops::V, int64_t vbytes, int i) const
    {
        return reinterpret_cast<const typename Ops::S *>(payload + vbytes)[i];
    }
};

template <bool USCALE> struct ImagePeer {
    const char *q_plane;
    const float *scales;
    template <class Ops> struct Raw {
        uint32_t w[Ops::PER / 4];
        f32x4 s4;      // USCALE: the wave's four scales
        float scale;   // otherwise: the lane's own
    };
    template <class Ops> __device__ __forceinline__ Raw<Ops> load(uint32_t span, int lane, int64_t) const
    {
        constexpr int PER = Ops::PER;
        const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(q_plane + (int64_t)span * (kStreamBlock * PER)), 0, kStreamBlock * PER, 0x00020000);
        Raw<Ops> raw{};
        if constexpr (PER == 4) {
            raw.w[0] = __builtin_amdgcn_raw_buffer_load_b32(rq, lane * 4, 0, kAuxStream);
        } else {
            const auto w2 = __builtin_amdgcn_raw_buffer_load_b64(rq, lane * 8, 0, kAuxStream);
            raw.w[0] = w2[0], raw.w[1] = w2[1];
        }
        const float *const sc = scales + (int64_t)span * 4;
        if constexpr (USCALE)
            raw.s4 = *reinterpret_cast<const f32x4 *>(sc);   // uniform: the wave's one load
        else
            raw.scale = __builtin_nontemporal_load(sc + (lane >> 4));
        return raw;
    }
    template <class Ops> __device__ __forceinline__ typename Ops::V item(const Raw<Ops> &raw, int lane) const
    {
        float scale = raw.scale;
        if constexpr (USCALE) {
            const int g = lane >> 4;
            scale = g == 0 ? raw.s4.x : g == 1 ? raw.s4.y : g == 2 ? raw.s4.z : raw.s4.w;
        }
        float x[Ops::PER];
#pragma unroll
        for (int e = 0; e < Ops::PER; ++e) {
            const int qv = (int)(raw.w[e / 4] << (24 - 8 * (e % 4))) >> 24;   // the signed byte
            x[e] = (float)qv * scale;
        }
        return __builtin_bit_cast(typename Ops::V, pack_narrow(Ops{}, x));
    }
    template <class Ops> __device__ __forceinline__ typename Ops::S ragged(typename Ops::V q, int64_t, int i) const
    {
        return item_elem(Ops{}, q, i);
    }
};

// Element i of an item that is being put together (the ragged item of an emitting span), from zeros.
__device__ __forceinline__ void item_put(f32x4 &v, int i, float t) { v[i] = t; }
__device__ __forceinline__ void item_put(u32x4 &v, int i, uint16_t t) { v[i / 2] |= (uint32_t)t << (16 * (i & 1)); }

// The unsigned maximum over the 16 lanes of a DPP row, the same in all 16: lane ^ 1, lane ^ 2 (quad_perm), then
// row_half_mirror (lane -> 7 - lane within each 8) and row_mirror (lane -> 15 - lane), which pair every quad
// with the one it has not met.  Every lane of the wave is active where this is called.
__device__ __forceinline__ uint32_t row_umax(uint32_t v)
{
    v = quad_umax(v);
    uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);
    v = v > o ? v : o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);
    return v > o ? v : o;
}

// What an emitting span adds: the image bytes of the item this lane stored into the snapshot, by k_pack's
// arithmetic to the bit (the codec of include/dpwa_hip.h).  A 256-byte group is the 16 lanes of a row, so amax
// crosses lanes by row_umax alone: no LDS memory, no ds_bpermute, no barrier.  The lane's q bytes go to q-plane
// offset 64 PER span + PER lane (one coalesced 256- or 512-byte store per wave, where ImagePeer reads) and lane 0
// of each row stores the group's scale (scales[4 span ..], 16 bytes per wave); both `sc1`, as the snapshot's
// stores: a peer reads them next.  `item` is zeros in the lanes past the payload's end.  `noise` is the
// rounding policy's for the item's PER elements (emit_noise), taken by the caller behind its loads.
template <int PER, class Round> __device__ __forceinline__ auto emit_noise(const Round &round, uint32_t span, int lane)
{
    return round.template noise<PER>(((uint64_t)span * kStreamBlock + (uint32_t)lane) * PER);
}

template <class Ops, class Noise>
__device__ __forceinline__ void emit_item(u32x4 item, uint32_t span, int lane, char *__restrict__ q_out,
                                          float *__restrict__ scales_out, const Noise &noise)
{
    constexpr int PER = Ops::PER;
    float x[PER];
    pack_widen(Ops{}, item, x);
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const uint32_t a = pk_bits(x[e]) & 0x7fffffffu;
        m = m > a ? m : a;
    }
    m = row_umax(m);
    const bool nonfinite = m >= 0x7f800000u;
    const float amax = pk_float(m);
    const bool normal = !nonfinite && amax >= 0x1p-100f;
    const float den = normal ? amax : 1.0f;
    const float inv = 127.0f / den;                  // the two divisions, once per lane
    const float scale = nonfinite ? pk_float(0x7fc00000u) : normal ? den / 127.0f : 0.0f;
    uint32_t q[PER / 4];
#pragma unroll
    for (int d = 0; d < PER / 4; ++d) {
        const uint32_t w = noise.q(4 * d, x[4 * d], inv) | noise.q(4 * d + 1, x[4 * d + 1], inv) << 8 |
                           noise.q(4 * d + 2, x[4 * d + 2], inv) << 16 | noise.q(4 * d + 3, x[4 * d + 3], inv) << 24;
        q[d] = normal ? w : 0u;
    }
    const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
        q_out + (int64_t)span * (kStreamBlock * PER), 0, kStreamBlock * PER, 0x00020000);
    if constexpr (PER == 4)
        __builtin_amdgcn_raw_buffer_store_b32(q[0], rq, lane * 4, 0, kAuxStore);
    else
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{q[0], q[1]}, rq, lane * 8, 0, kAuxStore);
    if ((lane & 15) == 0) {
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(scales_out + (int64_t)span * 4, 0, 16, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(pk_bits(scale), rs, (lane >> 4) * 4, 0, kAuxStore);
    }
}

// One 1-KiB span of the fused average whose ragged item stays with its lane: k_lerp_packed's body, with the
// peer's item from `peer` (PayloadPeer / ImagePeer).  EMIT (with DUAL): the span also writes the image bytes of
// what it stored into args.snap -- the averaged item, or in a no-op round the unchanged parameters -- so the
// grid may reach past the payload (whole 4-KiB blocks): such spans have zero-range descriptors, touch neither
// operand and emit q = 0 and scale = +0.0f, whatever `round` is (a zero has no fraction to round).
template <class Ops, bool DUAL, bool OOP, int POLICY, class Peer, bool EMIT, class Round>
__device__ __forceinline__ void packed_span(typename Ops::V *__restrict__ param, const Peer &peer, int64_t n,
                                            const LerpArgs &args, char *__restrict__ q_out,
                                            float *__restrict__ scales_out, const Round &round)
{
    static_assert(!EMIT || DUAL, "the emitting forms are those that write a snapshot");
    using V = typename Ops::V;
    using S = typename Ops::S;
    using P = LerpPolicy<POLICY>;
    constexpr int PER = Ops::PER;
    constexpr int SPAN = kStreamBlock * 16;
    const int lane = threadIdx.x;
    const int lane_off = lane * 16;
    const int64_t nbytes = n * (int64_t)sizeof(S);
    const int64_t vbytes = nbytes & ~(int64_t)15;
    const int64_t span_off = (int64_t)blockIdx.x * SPAN;
    const __amdgpu_buffer_rsrc_t rp = span_rsrc<SPAN>(param, span_off, vbytes);
    // issue this lane's loads before anything else
    const V p = span_load<V, P::param_load>(rp, lane_off);
    const auto raw = peer.template load<Ops>(blockIdx.x, lane, vbytes);
    // EMIT: the rounding policy's noise for the item this lane will store, under the loads and the factor
    [[maybe_unused]] const auto noise = emit_noise<EMIT ? PER : 1>(round, blockIdx.x, lane);
    const bool ragged = (nbytes & 15) && span_off + lane_off == vbytes;   // this lane owns the partial item
    [[maybe_unused]] S *const ps = reinterpret_cast<S *>(reinterpret_cast<char *>(param) + vbytes);
    [[maybe_unused]] S *const ss = reinterpret_cast<S *>(reinterpret_cast<char *>(args.snap) + vbytes);
    const int rag = (int)(nbytes & 15) / (int)sizeof(S);
    [[maybe_unused]] V item{};   // EMIT: what this lane stored into the snapshot; zeros past the payload's end
    [[maybe_unused]] const bool whole = span_off + lane_off < vbytes;
    float a, b;
    if (!lerp_coef<COEF_FUSED>(args, blockIdx.x == 0, a, b)) {
        if (DUAL) {   // no-op round; a write-through snapshot still gets the parameters
            span_store<V, P::snap_store>(span_rsrc<SPAN>(args.snap, span_off, vbytes), lane_off, p);
            if constexpr (EMIT) item = p;   // (zeros out of range)
            if (ragged) {
#pragma unroll
                for (int i = 0; i < PER - 1; ++i)
                    if (i < rag) {
                        const S t = ps[i];
                        ss[i] = t;
                        if constexpr (EMIT) item_put(item, i, t);
                    }
            }
        }
        if constexpr (!EMIT) return;
    } else {
        const V q = peer.template item<Ops>(raw, lane);
        const V r = Ops::lerp(a, b, q, p);
        if (!OOP) span_store<V, P::store>(rp, lane_off, r);
        if (DUAL) span_store<V, P::snap_store>(span_rsrc<SPAN>(args.snap, span_off, vbytes), lane_off, r);
        if constexpr (EMIT)
            if (whole) item = r;
        if (ragged) {
#pragma unroll
            for (int i = 0; i < PER - 1; ++i)
                if (i < rag) {
                    const S t = Ops::lerp_s(a, b, peer.template ragged<Ops>(q, vbytes, i), ps[i]);
                    if (!OOP) ps[i] = t;
                    if (DUAL) ss[i] = t;
                    if constexpr (EMIT) item_put(item, i, t);
                }
        }
    }
    if constexpr (EMIT) emit_item<Ops>(__builtin_bit_cast(u32x4, item), blockIdx.x, lane, q_out, scales_out, noise);
}

template <class Ops, bool DUAL, bool OOP, int POLICY, bool USCALE>
__global__ __launch_bounds__(kStreamBlock) void k_lerp_packed(typename Ops::V *__restrict__ param,
                                                              const char *__restrict__ q_plane,
                                                              const float *__restrict__ scales, int64_t n,
                                                              LerpArgs args)
{
    packed_span<Ops, DUAL, OOP, POLICY, ImagePeer<USCALE>, false>(param, ImagePeer<USCALE>{q_plane, scales}, n, args,
                                                                  nullptr, nullptr, RoundNearest{});
}

// The emitting form of the fused write-through average (include/dpwa_hip.h dpwa_average_pack): one-wave
// workgroups over 4 pack_blocks spans, so that both planes of the image are written whole.  The next
// snapshot's image leaves from the registers that hold the snapshot: a round moves (3 + 0.27) n s bytes (fp32;
// 3 + 0.52 for a 16-bit type) plus the peer operand, in one launch, where the average followed by k_pack moved
// (3 + 1.27) n s in two.  There is no resident (OOP) form: resident parameters live in the slot and the step
// that follows the average writes them there, so their image can only be taken at the publish.
template <class Ops, int POLICY, class Peer, class Round>
__global__ __launch_bounds__(kStreamBlock) void k_lerp_emit(typename Ops::V *__restrict__ param, Peer peer, int64_t n,
                                                            LerpArgs args, char *__restrict__ q_out,
                                                            float *__restrict__ scales_out, Round round)
{
    packed_span<Ops, true, false, POLICY, Peer, true>(param, peer, n, args, q_out, scales_out, round);
}

// How the wave gets its four scales (k_lerp_packed): the wave's one uniform load, or with
// DPWA_PACKED_SCALES=lane every lane's own (A/B runs).  Measured write-through, interleaved on the same
// buffers (profiles/pack_avg_cost.json, pack_avg_cost_lane.json): 11.17M fp32 24.6 us against 32.5,
// 2^26 bf16 64.8 against 69.7.
constexpr int kPackedScalesUniform = 1;
static bool packed_scales_uniform()
{
    static const bool on = env_knob("DPWA_PACKED_SCALES", kPackedScalesUniform, [](const char *e) {
        return strcmp(e, "uniform") == 0 ? 1 : strcmp(e, "lane") == 0 ? 0 : kNoValue;
    }) != 0;
    return on;
}

hipError_t launch_average_packed(int32_t dtype, void *param, int64_t n, const void *image, const FusedArgs &fa,
                                 void *snap, hipStream_t s, const LaunchTiming *timing, bool oop)
{
    if (!is_float_dtype(dtype) || n < 0 || !image || (!param && n > 0) || (oop && !snap && n > 0) ||
        !aligned16(param, image, snap))
        return hipErrorInvalidValue;
    const int64_t nbytes = n * (int64_t)dtype_size(dtype);
    const int64_t grid = nbytes <= 0 ? 1 : (nbytes + kStreamBlock * 16 - 1) / (kStreamBlock * 16);
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    LerpArgs args{};
    args.fused = fa;
    args.snap = snap;
    const char *const q_plane = (const char *)image;
    const float *const scales = (const float *)(q_plane + pack_scale_offset(dtype, n));
    return with_ops(dtype, [&](auto ops) {
        using Ops = decltype(ops);
        using V = typename Ops::V;
        const auto run = [&](void (*kernel)(V *, const char *, const float *, int64_t, LerpArgs)) {
            return launch(kernel, dim3((uint32_t)grid), dim3(kStreamBlock), s, timing, param, q_plane, scales, n, args);
        };
        const auto forms = [&](auto uscale) {
            constexpr bool U = decltype(uscale)::value;
            // (resident: the product policy unless DPWA_LERP_POLICY forces the other, as k_lerp's resident form)
            return BySizePolicies::with(oop ? lerp_policy() : lerp_policy(nbytes), [&](auto policy) {
                constexpr int P = decltype(policy)::value;
                if (oop) return run(k_lerp_packed<Ops, true, true, P, U>);
                return snap ? run(k_lerp_packed<Ops, true, false, P, U>) : run(k_lerp_packed<Ops, false, false, P, U>);
            });
        };
        return packed_scales_uniform() ? forms(std::true_type{}) : forms(std::false_type{});
    });
}

// A write-through round of a pack-enabled learner emits the next snapshot's image from its average; DPWA_PACK_FUSED=0 keeps the average and the publish's k_pack as two launches (A/B runs).
// profiles/pack_emit_cost.json has both, interleaved on the same buffers.
bool pack_fused()
{
    static const bool on = env_knob("DPWA_PACK_FUSED", 1, [](const char *e) {
        return strcmp(e, "1") == 0 ? 1 : strcmp(e, "0") == 0 ? 0 : kNoValue;
    }) != 0;
    return on;
}

hipError_t launch_average_emit(int32_t dtype, void *param, int64_t n, const void *peer, const void *peer_image,
                               const FusedArgs &fa, void *snap, void *image_out, hipStream_t s,
                               const LaunchTiming *timing, PackRounding rounding)
{
    if (!is_float_dtype(dtype) || n < 0 || (!peer) == (!peer_image) || !param || !snap || !image_out ||
        snap == param || !aligned16(param, peer, peer_image) || !aligned16(snap, image_out))
        return hipErrorInvalidValue;
    const int64_t nbytes = n * (int64_t)dtype_size(dtype);
    const int64_t grid = 4 * pack_blocks(dtype, n);   // both planes whole
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    LerpArgs args{};
    args.fused = fa;
    args.snap = snap;
    const int64_t scale_off = pack_scale_offset(dtype, n);
    char *const q_out = (char *)image_out;
    float *const scales_out = (float *)(q_out + scale_off);
    return with_ops(dtype, [&](auto ops) {
        using Ops = decltype(ops);
        const auto from = [&](auto src) {
            using Peer = decltype(src);
            // (the policies of launch_average_packed)
            return BySizePolicies::with(lerp_policy(nbytes), [&](auto policy) {
                return with_round(rounding, [&](auto round) {
                    return launch(k_lerp_emit<Ops, decltype(policy)::value, Peer, decltype(round)>, dim3((uint32_t)grid),
                                  dim3(kStreamBlock), s, timing, param, src, n, args, q_out, scales_out, round);
                });
            });
        };
        if (peer) return from(PayloadPeer{(const char *)peer});
        const char *const q_plane = (const char *)peer_image;
        return from(ImagePeer<true>{q_plane, (const float *)(q_plane + scale_off)});
    });
}

}  // namespace dpwa
