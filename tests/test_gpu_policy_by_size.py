"""The cache policy of an averaging launch follows the bytes it touches (dpwa_amd/csrc/policy.hpp:
the fit policy while 3 x payload is at most the threshold, the product policy above), and a policy
changes cache bits only: on either side of the threshold, and exactly on it, every form that chooses
by size -- plain, write-through, batched, tracked, mixed -- gives the host references' bits.

The threshold (DPWA_CACHE_FIT_BYTES) and DPWA_LERP_POLICY are read once per process, so each setting
runs tests/policy_worker.py in a fresh child process, one at a time.  The worker reports how many of its
launches fell below, on and above the threshold in force; the settings are chosen so that
  below      every launch is below it (the fit instantiation of every form)
  on         float32 n = 257 is exactly on it (3 x 1028 bytes): its lerp, plain, write-through and tracked
             launches; smaller shapes below, larger above
  on, batch  the batch of 1 and 255 float32 elements is exactly on it by the sum of its entries
             (3 x 1024 bytes), while n = 255 alone is below and n = 257 above
  on, mixed  the mixed layout of two 4-KiB segments is exactly on it (3 x 8192 bytes)
  above      every launch is above it (the product instantiation of every form)
and DPWA_LERP_POLICY=8 alone must give what the product gave before the policy went by size.
Which side a byte count falls on is checked on the host (tests/test_policy_host.py)."""
import os
import re
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120                    # a cap against a hang, not an expectation
ABNORMAL = (134, 139, 124, 137, 3)       # abort, segmentation fault, a time limit's two codes, a failed call
LAUNCHES = 44                            # 6 shapes x (2 lerps + 4 averages) + 3 batches x 2 + 2 mixed

# (name, environment, launches expected (below, on, above) or None without a threshold in the environment)
SETTINGS = [
    ("below", {"DPWA_CACHE_FIT_BYTES": str(1 << 40)}, (LAUNCHES, 0, 0)),
    ("on", {"DPWA_CACHE_FIT_BYTES": str(3 * 257 * 4)}, None),
    ("on, batch", {"DPWA_CACHE_FIT_BYTES": str(3 * (1 + 255) * 4)}, None),
    ("on, mixed", {"DPWA_CACHE_FIT_BYTES": str(3 * 2 * 4096)}, None),
    ("above", {"DPWA_CACHE_FIT_BYTES": "3"}, (0, 0, LAUNCHES)),
    ("policy 8 forced", {"DPWA_LERP_POLICY": "8"}, None),
]


_stopped = []      # the setting whose child ended abnormally: nothing more is started on the GPU after a fault


@pytest.mark.parametrize("name,env,want", SETTINGS, ids=[s[0].replace(", ", "-").replace(" ", "-") for s in SETTINGS])
def test_a_side_of_the_threshold_in_a_process_of_its_own(name, env, want):
    """A child that mismatches (exit 1) is an ordinary failure.  A child that ends abnormally -- a
    timeout, a signal, an abort, a failed call -- stops the walk: the settings after it fail unstarted."""
    if _stopped:
        pytest.fail("not started: the child of %r ended abnormally" % _stopped[0])
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.policy_worker"]
    base = {k: v for k, v in os.environ.items() if k not in ("DPWA_CACHE_FIT_BYTES", "DPWA_LERP_POLICY")}
    began = time.monotonic()
    try:
        child = subprocess.run(cmd, cwd=ROOT, env=dict(base, **env), stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        _stopped.append(name)
        out = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
        pytest.fail("%s: no end after %d s; the walk stops here\n%s" % (name, CHILD_TIMEOUT_S, out[-4000:]))
    print("%s: exit %d after %.1f s" % (name, child.returncode, time.monotonic() - began))
    if child.returncode < 0 or child.returncode in ABNORMAL:
        _stopped.append(name)
        pytest.fail("%s: ended abnormally (%d); the walk stops here\n%s" % (name, child.returncode, child.stdout[-4000:]))
    m = re.search(r"policy_worker: ok below=(\d+) on=(\d+) above=(\d+)", child.stdout)
    assert child.returncode == 0 and m, "%s: exit %d\n%s" % (name, child.returncode, child.stdout[-2000:])
    got = tuple(int(x) for x in m.groups())
    if "DPWA_CACHE_FIT_BYTES" in env:
        assert sum(got) == LAUNCHES, (name, got)
    if want is not None:
        assert got == want, (name, got)
    if name == "on":            # float32 n = 257: two lerps and four averages, and something on either side
        assert got[1] == 6 and got[0] > 0 and got[2] > 0, (name, got)
    if name in ("on, batch", "on, mixed"):     # plain and write-through
        assert got[1] == 2 and got[0] > 0 and got[2] > 0, (name, got)
