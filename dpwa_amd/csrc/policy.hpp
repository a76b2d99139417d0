// policy.hpp -- which cache policy (kernels.hip LerpPolicy) an averaging launch takes, from the
// bytes it touches.  Host code with no HIP in it, so tests/native/policy_check.cpp runs it alone.
//
// Three cases decide it ("Cache policy by size"):
//   bare loop  bench.py's headline: the same learner averaged back to back.  Its next round
//              re-reads what this one stored, so parameters stored `nt` (policy 8) are fetched
//              from HBM again although they would have fitted the Infinity Cache.
//   trained    a writer (the optimizer) before the average and a reader (the forward pass) after
//              it, the peer's snapshot cold (tools/trained_regime.py).
//   cold       nobody touched the operands within the last 256 MB of traffic: true of payloads
//              far beyond the cache, never of a model that fits it several times over.
// A launch whose parameters and two snapshot slots (3 x payload) are at most kCacheFitBytes
// takes kFitPolicy; a larger one takes kProductPolicy, which wins cold by 1-3 %.
#pragma once

#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace dpwa {

// Parameters stored `nt`, the snapshot `sc1`: with the batched dispatch it lifts every cold
// averaging kernel by 1-3 % of peak (11.17M batched 0.78 -> 0.80-0.81, 7B bf16 full 0.81 -> 0.82,
// profiles/r03_policy_ab.log).  The policy of every launch above the cache-fit threshold and of
// the resident, pair, group and relay kernels.
constexpr int kProductPolicy = 8;
// Nothing stored `nt`: what was averaged stays in the Infinity Cache for whoever reads it next.
// At 11.17M fp32 in the trained regime (profiles/trained_regime.json, three repeats of 300 rounds
// per policy, fresh processes taking turns): the average 28.2-28.6 us against policy 8's 28.8-29.0
// (p10-p90 28.2-29.7), writer + average + reader 75.6-75.7 us a round against 79.9-80.2 (-5.6 %).
// Policy 1 (the parameters also loaded with the default policy) gives the same round (75.3-76.0 us)
// with a slower average (28.6-28.7 us), so it is 0.
constexpr int kFitPolicy = 0;

constexpr size_t kInfinityCacheBytes = (size_t)256 << 20;
// The largest 3 x payload that takes kFitPolicy.  bench.py's headline, never fit against always fit
// taking turns (profiles/fit_threshold.json): 3 x payload 67 MB +4.6 %, 134 MB (configs[1]) +1.4 %,
// 202 MB -0.2 % (a tie), 268 MB -1.0 %, 402 MB -8.5 %, 536 MB -12.5 %; so the threshold lies
// between the last size that won and the first that did not.  DPWA_CACHE_FIT_BYTES overrides it
// (A/B runs, tests); 0: never fit.
constexpr int64_t kCacheFitBytes = (int64_t)160 << 20;

constexpr int kNoPolicy = -1;

// DPWA_LERP_POLICY: 0..31 forces that policy on every launch; unset or out of range, kNoPolicy.
inline int parse_lerp_policy(const char *text)
{
    if (!text) return kNoPolicy;
    const int p = atoi(text);
    return p >= 0 && p <= 31 ? p : kNoPolicy;
}

// DPWA_CACHE_FIT_BYTES: a non-negative byte count; unset or anything else, `dflt`.
inline int64_t parse_cache_fit_bytes(const char *text, int64_t dflt = kCacheFitBytes)
{
    if (!text || !*text) return dflt;
    char *end = nullptr;
    errno = 0;
    const long long v = strtoll(text, &end, 10);
    return errno == 0 && end != text && *end == '\0' && v >= 0 ? (int64_t)v : dflt;
}

// The payload bytes of a dispatch: the sum over its `count` entries of n[i] elements of `elem` bytes.
inline int64_t payload_bytes(const int64_t *n, int count, int64_t elem)
{
    int64_t bytes = 0;
    for (int i = 0; i < count; ++i) bytes += n[i] * elem;
    return bytes;
}

// The policy requested of a launch that averages `payload` bytes: `forced` unless kNoPolicy,
// else kFitPolicy while the parameters and two slots fit `fit_bytes`, else kProductPolicy.
inline int policy_for_bytes(int forced, int64_t fit_bytes, int64_t payload)
{
    if (forced != kNoPolicy) return forced;
    // (payload <= fit_bytes / 3 would round; 3 x a payload of under 2^61 bytes does not overflow)
    return fit_bytes > 0 && payload >= 0 && payload <= INT64_MAX / 3 && 3 * payload <= fit_bytes ? kFitPolicy
                                                                                                  : kProductPolicy;
}

}  // namespace dpwa
