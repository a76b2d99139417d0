// policy_check.cpp -- dpwa_amd/csrc/policy.hpp (which cache policy an averaging launch takes, from
// the bytes it touches) on the host alone: the header has no HIP in it.  The rule on either side of
// the threshold and exactly on it, the sum over a batch's entries, the two overrides and their
// parsing, `0` meaning never fit, and byte counts near the top of int64.  Prints "policy check ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../dpwa_amd/csrc/policy.hpp"

using namespace dpwa;

static int failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

int main()
{
    static_assert(kFitPolicy != kProductPolicy, "the size would choose between one policy");
    static_assert(kFitPolicy >= 0 && kFitPolicy <= 31 && (kFitPolicy & 8) == 0, "the fit policy stores the parameters `nt`");
    static_assert(kProductPolicy == 8, "the product policy");
    static_assert(kCacheFitBytes > 0, "the built-in threshold is a byte count");

    // the rule: 3 x payload against the threshold, inclusive
    const int64_t T = 3 * 1028;
    CHECK(policy_for_bytes(kNoPolicy, T, 1027) == kFitPolicy);
    CHECK(policy_for_bytes(kNoPolicy, T, 1028) == kFitPolicy);      // exactly on it
    CHECK(policy_for_bytes(kNoPolicy, T, 1029) == kProductPolicy);
    CHECK(policy_for_bytes(kNoPolicy, T + 2, 1028) == kFitPolicy);  // a threshold that is no multiple of 3:
    CHECK(policy_for_bytes(kNoPolicy, T + 2, 1029) == kProductPolicy);   // 3 x 1029 = T + 3
    CHECK(policy_for_bytes(kNoPolicy, T - 1, 1028) == kProductPolicy);
    CHECK(policy_for_bytes(kNoPolicy, T, 0) == kFitPolicy);
    // configs[1] and the first north_star size above the cache, at the built-in threshold
    CHECK(policy_for_bytes(kNoPolicy, kCacheFitBytes, (int64_t)11173962 * 4) == kFitPolicy);
    CHECK(policy_for_bytes(kNoPolicy, kCacheFitBytes, (int64_t)100000000 * 4) == kProductPolicy);
    CHECK(policy_for_bytes(kNoPolicy, kCacheFitBytes, (int64_t)7000000000 * 2) == kProductPolicy);

    // 0: never fit, an empty launch included
    CHECK(policy_for_bytes(kNoPolicy, 0, 0) == kProductPolicy);
    CHECK(policy_for_bytes(kNoPolicy, 0, 1) == kProductPolicy);
    // byte counts whose triple does not fit int64, and the resident forms' "no size"
    CHECK(policy_for_bytes(kNoPolicy, INT64_MAX, INT64_MAX / 3) == kFitPolicy);
    CHECK(policy_for_bytes(kNoPolicy, INT64_MAX, INT64_MAX / 3 + 1) == kProductPolicy);
    CHECK(policy_for_bytes(kNoPolicy, INT64_MAX, INT64_MAX) == kProductPolicy);
    CHECK(policy_for_bytes(kNoPolicy, T, -1) == kProductPolicy);

    // a forced policy holds everywhere
    for (int forced = 0; forced <= 31; ++forced) {
        CHECK(policy_for_bytes(forced, T, 4) == forced);
        CHECK(policy_for_bytes(forced, T, 1 << 20) == forced);
        CHECK(policy_for_bytes(forced, 0, 4) == forced);
        CHECK(policy_for_bytes(forced, INT64_MAX, INT64_MAX) == forced);
    }

    // a batch goes by the sum of its entries
    const int64_t two[2] = {1, 255};
    CHECK(payload_bytes(two, 2, 4) == 1024);
    CHECK(payload_bytes(two, 1, 4) == 4);
    CHECK(payload_bytes(two, 0, 4) == 0);
    CHECK(policy_for_bytes(kNoPolicy, 3 * 1024, payload_bytes(two, 2, 4)) == kFitPolicy);       // exactly on it
    CHECK(policy_for_bytes(kNoPolicy, 3 * 1024 - 1, payload_bytes(two, 2, 4)) == kProductPolicy);
    CHECK(policy_for_bytes(kNoPolicy, 3 * 1024 - 1, 255 * 4) == kFitPolicy);                    // each entry alone would fit
    const int64_t eight[8] = {11173962, 11173962, 11173962, 11173962, 11173962, 11173962, 11173962, 11173962};
    CHECK(payload_bytes(eight, 8, 4) == (int64_t)8 * 11173962 * 4);
    CHECK(policy_for_bytes(kNoPolicy, kCacheFitBytes, payload_bytes(eight, 8, 4)) == kProductPolicy);   // 1.07 GB
    CHECK(policy_for_bytes(kNoPolicy, kCacheFitBytes, payload_bytes(eight, 1, 4)) == kFitPolicy);

    // DPWA_LERP_POLICY
    CHECK(parse_lerp_policy(nullptr) == kNoPolicy);
    CHECK(parse_lerp_policy("8") == 8);
    CHECK(parse_lerp_policy("0") == 0);
    CHECK(parse_lerp_policy("31") == 31);
    CHECK(parse_lerp_policy("32") == kNoPolicy);
    CHECK(parse_lerp_policy("-1") == kNoPolicy);

    // DPWA_CACHE_FIT_BYTES
    CHECK(parse_cache_fit_bytes(nullptr) == kCacheFitBytes);
    CHECK(parse_cache_fit_bytes("") == kCacheFitBytes);
    CHECK(parse_cache_fit_bytes("0") == 0);
    CHECK(parse_cache_fit_bytes("3084") == 3084);
    CHECK(parse_cache_fit_bytes("1099511627776") == (int64_t)1 << 40);
    CHECK(parse_cache_fit_bytes("9223372036854775807") == INT64_MAX);
    CHECK(parse_cache_fit_bytes("9223372036854775808") == kCacheFitBytes);   // out of range
    CHECK(parse_cache_fit_bytes("-5") == kCacheFitBytes);
    CHECK(parse_cache_fit_bytes("12k") == kCacheFitBytes);
    CHECK(parse_cache_fit_bytes("many") == kCacheFitBytes);
    CHECK(parse_cache_fit_bytes("7", 99) == 7);
    CHECK(parse_cache_fit_bytes("x", 99) == 99);

    if (failures) return 1;
    std::printf("policy check ok\n");
    return 0;
}
