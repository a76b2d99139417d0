// node_lerp_check.cpp -- TEST INFRASTRUCTURE: a node never fetches over a factor whose lerp was not issued.
// Over the host-only fake learner (fake_learner.cpp), which refuses such a fetch when it skips non-finite peers
// (fake_check), as learner.cpp's dpwa_learner_fetch does.  node.cpp's start_fetch abandons the factored fetch
// first, as dpwa_node_publish does: an eager gate after an update_wait without its lerp and without a publish goes
// through, with one cancel and one pull.
// Driven by tests/test_node_host.py.
#include <cstdint>
#include <cstdio>

#include "../../include/dpwa_hip.h"

extern "C" {
int fake_check(dpwa_learner *l, int on);
int fake_cancels(dpwa_learner *l, int *out);
int fake_counts(dpwa_learner *l, int *out);
}

#define CHECK(x)                                                                             \
    do {                                                                                     \
        const int rc_ = (x);                                                                 \
        if (rc_) {                                                                           \
            fprintf(stderr, "%s:%d %s = %d (%s)\n", __FILE__, __LINE__, #x, rc_, dpwa_last_error()); \
            return 2;                                                                        \
        }                                                                                    \
    } while (0)
#define EXPECT(c)                                                                            \
    do {                                                                                     \
        if (!(c)) {                                                                          \
            fprintf(stderr, "%s:%d expectation failed: %s\n", __FILE__, __LINE__, #c);      \
            return 3;                                                                        \
        }                                                                                    \
    } while (0)

struct Counts {
    int pulls, averages, cancels;
};

static int counts(dpwa_learner *l, Counts &c)
{
    int v[5];
    if (int rc = fake_counts(l, v)) return rc;
    c.pulls = v[0];
    c.averages = v[3];
    return fake_cancels(l, &c.cancels);
}

int main()
{
    const dpwa_interp cfg{DPWA_INTERP_CONSTANT, 0, 0.5, 0.0};
    dpwa_node *nodes[2] = {nullptr, nullptr};
    dpwa_learner *learners[2] = {nullptr, nullptr};
    for (int g = 0; g < 2; ++g) {
        const uint32_t key = 11 + (uint32_t)g;
        CHECK(dpwa_node_create(&nodes[g], 1, &key, 1, 1.0, &cfg));   // fetch probability 1: every gate grants
        CHECK(dpwa_node_bind(nodes[g], 0, 1000, DPWA_F32));
        CHECK(dpwa_node_handles(nodes[g], &learners[g], nullptr));
    }
    CHECK(dpwa_node_set_peer(nodes[0], 0, DPWA_NODE_PEER_LOCAL, nodes[1]));
    CHECK(dpwa_node_set_peer(nodes[1], 0, DPWA_NODE_PEER_LOCAL, nodes[0]));
    CHECK(fake_check(learners[0], 1));
    dpwa_node *n = nodes[0];
    dpwa_learner *l = learners[0];
    int fetching = 0, peer = -2;
    Counts a, b;

    // the loop's order first: a publish abandons the factor whose lerp never came
    CHECK(dpwa_node_update_send(nodes[1], nullptr, 1.0, nullptr, 0, nullptr, &fetching));
    CHECK(dpwa_node_update_send(n, nullptr, 1.0, nullptr, 0, nullptr, &fetching));
    CHECK(dpwa_node_update_wait(n, 1.0, nullptr, 0, nullptr, &peer));
    EXPECT(fetching == 1 && peer == 0);
    CHECK(counts(l, a));
    CHECK(dpwa_node_update_send(n, nullptr, 1.0, nullptr, 0, nullptr, &fetching));
    CHECK(counts(l, b));
    EXPECT(b.cancels == a.cancels + 1 && b.pulls == a.pulls);
    CHECK(dpwa_node_update_wait(n, 1.0, nullptr, 0, nullptr, &peer));
    EXPECT(peer == 0);

    // an eager gate with no publish in between: the factored fetch is abandoned, the new one issued
    CHECK(counts(l, a));
    CHECK(dpwa_node_gate(n, DPWA_FLAG_EAGER, nullptr, &fetching));
    CHECK(counts(l, b));
    EXPECT(fetching == 1 && b.cancels == a.cancels + 1 && b.pulls == a.pulls + 1);
    CHECK(dpwa_node_update_wait(n, 1.0, nullptr, 0, nullptr, &peer));
    EXPECT(peer == 0);
    CHECK(dpwa_node_lerp(n, nullptr, nullptr));
    CHECK(counts(l, a));
    EXPECT(a.averages == b.averages + 1 && a.cancels == b.cancels);

    // twice in a row, the second time with no lerp at all in between
    CHECK(dpwa_node_gate(n, DPWA_FLAG_EAGER, nullptr, &fetching));
    CHECK(dpwa_node_update_wait(n, 1.0, nullptr, 0, nullptr, &peer));   // factored, no lerp
    CHECK(counts(l, a));
    CHECK(dpwa_node_gate(n, DPWA_FLAG_EAGER, nullptr, &fetching));
    CHECK(counts(l, b));
    EXPECT(fetching == 1 && b.cancels == a.cancels + 1 && b.pulls == a.pulls + 1);
    CHECK(dpwa_node_update_wait(n, 1.0, nullptr, 0, nullptr, &peer));
    CHECK(dpwa_node_lerp(n, nullptr, nullptr));
    EXPECT(peer == 0);
    // (a gate that only grants starts no fetch before the next publish -- fetch_started is reset there -- so the
    // eager gate is the one way from a factor to a fetch without a publish)

    for (int g = 0; g < 2; ++g) CHECK(dpwa_node_destroy(nodes[g]));
    fprintf(stderr, "node lerp check ok\n");
    return 0;
}
