"""The kernel variants behind environment knobs.  kernels.hip instantiates the multi-wave form of
the averaging kernel (DPWA_LERP_BLOCK: wave 0 hands the factor over through LDS), its cache
policies (DPWA_LERP_POLICY), the batch's span orders (DPWA_BATCH_ORDER, DPWA_BATCH_SHARE=0,
DPWA_PAIR_FUSED=0) and the wider publish (DPWA_PUBLISH_BLOCK); A/B measurements switch between
them, and nothing else in the suite sets a knob.  The knobs are read once per process, so each
variant runs tests/forms_worker.py -- the plain, fused, batched and resident forms on hard values
with guard bands, for float32 and bfloat16 -- in a fresh child process, one at a time."""
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [
    ("DPWA_LERP_BLOCK", "128"),
    ("DPWA_LERP_BLOCK", "256"),
    ("DPWA_LERP_BLOCK", "512"),
    ("DPWA_LERP_POLICY", "0"),
    ("DPWA_PAIR_FUSED", "0"),
    ("DPWA_BATCH_SHARE", "0"),
    ("DPWA_BATCH_ORDER", "contiguous"),
    ("DPWA_BATCH_ORDER", "interleaved"),
    ("DPWA_PUBLISH_BLOCK", "128"),
    ("DPWA_PUBLISH_BLOCK", "256"),
]
CHILD_TIMEOUT_S = 120                    # a cap against a hang, not an expectation
ABNORMAL = (134, 139, 124, 137)          # abort, segmentation fault, a time limit's two codes


def test_every_variant_in_a_process_of_its_own():
    """A child that mismatches (exit 1) is an ordinary failure: the walk goes on and all such
    variants are reported together.  A child that ends abnormally -- a timeout, a signal, an abort
    -- stops the walk: nothing more is started on the GPU after a fault."""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.forms_worker"]
    failed = []
    for knob, value in VARIANTS:
        variant = "%s=%s" % (knob, value)
        began = time.monotonic()
        try:
            child = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, **{knob: value}), stdout=subprocess.PIPE,
                                   stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired as e:
            out = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
            pytest.fail("%s: no end after %d s; the walk stops here\n%s" % (variant, CHILD_TIMEOUT_S, out[-4000:]))
        print("%s: exit %d after %.1f s" % (variant, child.returncode, time.monotonic() - began))
        if child.returncode < 0 or child.returncode in ABNORMAL:
            pytest.fail("%s: ended abnormally (%d); the walk stops here\n%s"
                        % (variant, child.returncode, child.stdout[-4000:]))
        if child.returncode != 0 or "forms_worker: ok" not in child.stdout:
            failed.append("%s: exit %d\n%s" % (variant, child.returncode, child.stdout[-2000:]))
    assert not failed, "\n".join(failed)
