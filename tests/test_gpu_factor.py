"""The device factor on hard values through every kernel that runs it: k_factor, the 64-lane
averaging kernel (every lane evaluates it), the element-wise kernel for unaligned views, the mixed
and tracked kernels, the batch (once per entry), the pair and group kernels (one factor per entry in
registers), a learner's rounds with the status word and the written-ahead header, and -- in child
processes -- the multi-wave form that hands a, b and ok over through LDS and the batch's other
orders.

The cases are the table of tests/factor_ref.py: contraction-sensitive clocks, the double rounding
of b, the association of the threshold scaling, fp32 and fp64 edges, ZeroDivisionError in every
spelling, non-finite values and device-read losses.  Expected: ``oracle.policy.factor_and_clock``,
bit for bit (NaN payloads excepted); expected parameters: the host references of tests/forms_ref.py
at that factor.  tests/test_factor_host.py shows on the CPU that each form's cases tell every
plausible wrong factor_math from the reference.  The forms are the functions of
tests/factor_worker.py.

Shapes: 2 * 64 * PER + 1 elements (a committing workgroup, one that only consumes a and b, the
ragged-tail lane) and 1 element (the tail alone)."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from dpwa_amd import _lib
from tests import factor_ref as fr
from tests import factor_worker as forms
from tests import forms_ref as ref
from tests.forms_ref import CODE
from tests.test_gpu_kernels import ptr
from tests.test_gpu_variants import ABNORMAL, CHILD_TIMEOUT_S, ROOT

pytestmark = pytest.mark.gpu

DEV = forms.DEV
UNALIGNED = (1, 3)             # (parameters, snapshot) in elements off the 16-byte alignment


# ---------------------------------------------------------------- 1. dpwa_factor
@pytest.mark.parametrize("device_loss", [False, True], ids=["host-loss", "device-f64-loss"])
def test_factor_kernel(device_loss):
    """Every case through k_factor alone: dpwa_coef and the clock (moved in place; kept by a zero
    division) bit for bit, nothing else inside the 0xA5 bytes around them written."""
    for case in fr.CASES:
        forms.run_factor(case, device_loss)


# ---------------------------------------------------------------- 2. dpwa_average
@pytest.mark.parametrize("write_through", [False, True], ids=["plain", "write-through"])
def test_average_f32(write_through):
    """Every case through the fused kernel at both sizes: the committed factor, the clock written
    behind the untouched clock read, and every parameter (and snapshot) bit."""
    for n in forms.sizes("f32"):
        for case in fr.CASES:
            forms.run_average("f32", n, case, write_through)


@pytest.mark.parametrize("write_through", [False, True], ids=["plain", "write-through"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_average_16_bit(dtype, write_through):
    for n in forms.sizes(dtype):
        for case in fr.CATCHING:
            forms.run_average(dtype, n, case, write_through)


@pytest.mark.parametrize("write_through", [False, True], ids=["plain", "write-through"])
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_average_unaligned(dtype, write_through):
    """Parameters one element and the snapshot three elements off the alignment: k_lerp_unaligned."""
    for case in fr.CATCHING:
        forms.run_average(dtype, forms.big(dtype), case, write_through, offsets=UNALIGNED)


@pytest.mark.parametrize("write_through", [False, True], ids=["plain", "write-through"])
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_average_tracked_kernel(dtype, write_through):
    """dpwa_average_tracked (k_lerp_tracked): coef, clock and parameters are dpwa_average's.  (What
    the distance record holds after a NaN or zero-division round is tests/test_gpu_distance.py's.)"""
    for n in forms.sizes(dtype):
        for case in fr.CATCHING:
            forms.run_average(dtype, n, case, write_through, tracked=True)


# ---------------------------------------------------------------- 3. dpwa_average_mixed
@pytest.mark.parametrize("write_through", [False, True], ids=["plain", "write-through"])
def test_average_mixed(write_through):
    for case in fr.CATCHING:
        forms.run_mixed(case, write_through)


# ---------------------------------------------------------------- 4. dpwa_average_many
@pytest.mark.parametrize("write_through", [False, True], ids=["plain", "write-through"])
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_average_many(dtype, write_through):
    """Each entry its own case of one cfg: unequal sizes (the begin[] scan), equal sizes (the
    round-robin order), 8 entries, and a zero-division and a NaN-factor entry between finite ones,
    whose neighbours must be exactly their own references."""
    for name, pattern, cases in fr.many_dispatches():
        forms.run_many(dtype, name, pattern, cases, write_through)


# ---------------------------------------------------------------- 5. dpwa_average_many_resident
@pytest.mark.parametrize("name", list(fr.TOPOLOGIES))
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_average_many_resident(dtype, name):
    """The mutual pair (k_lerp_pair), a 3-cycle and four pairs (k_lerp_group with 3 and 8 buffers),
    two entries apart (k_lerp_batch) and eleven buffers (the XCD-grouped batch): one factor per
    entry, none leaking into a neighbour."""
    forms.run_resident_all(dtype, name, forms.big(dtype))
    if name == "mutual-pair":
        forms.run_resident_all(dtype, name, 1)


# ---------------------------------------------------------------- 6. through a learner
def by_cfg(cases):
    out = {}
    for case in cases:
        out.setdefault(fr.cfg_of(case), []).append(case)
    return list(out.values())


@pytest.mark.parametrize("write_through", [False, True], ids=["plain", "write-through"])
def test_learner_tracked(write_through):
    """A learner with the distance on runs the tracked kernel: coef, clock and parameters."""
    for cases in by_cfg(fr.LEARNER_CATCHING):
        pair = forms.Pair("f32", forms.big("f32"), cases[0], track=True)
        try:
            for case in cases:
                pair.round(case, write_through)
        finally:
            pair.close()


def test_learner_device_loss():
    """The same loss as a host double, a device float64 and a device float32 (read in place and
    widened exactly: an fp32-subnormal loss is not flushed)."""
    cases = fr.device_loss_cases()
    pair = forms.Pair("f32", forms.big("f32"), cases[0])
    try:
        for case in cases:
            assert float(np.float32(case[5])) == case[5]
            for loss in (case[5], torch.tensor(case[5], dtype=torch.float64, device=DEV),
                         torch.tensor(np.float32(case[5]), dtype=torch.float32, device=DEV)):
                pair.round(case, loss=loss)
    finally:
        pair.close()


def test_learner_status_is_reported_once():
    """OK, zero division, OK: the status word keeps the zero division through the OK round that
    follows, reports it once and is OK again (dpwa_learner_poll_status, and the word read directly
    as Learner.take_status does); the dpwa_coef of each round holds that round's own status."""
    ok = fr.family("contraction")[1]                         # clock interpolation; a contracted clock and
    zd = ok[:3] + (-ok[4],) + ok[4:]                         # b = 1f - a both show on it.  zd: c == -pc
    assert fr.kind(ok) == "finite" and fr.kind(zd) == "zd"
    assert all(fr.catches(ok, m) for m in ("contract-first-product", "contract-second-product", "b-from-a"))
    pair = forms.Pair("f32", forms.big("f32"), ok)
    try:
        pair.round(ok)
        assert pair.me.take_status() == _lib.STATUS_OK
        pair.round(zd)
        pair.round(ok)                                       # (its dpwa_coef is OK: checked in round)
        assert pair.me.poll_status()[1] == _lib.STATUS_ZERO_DIVISION
        assert pair.me.poll_status()[1] == _lib.STATUS_OK
        pair.round(zd, write_through=True)
        assert pair.me.take_status() == _lib.STATUS_ZERO_DIVISION
        assert pair.me.take_status() == _lib.STATUS_OK and pair.me.poll_status()[1] == _lib.STATUS_OK
    finally:
        pair.close()


def test_learner_written_ahead_header():
    """A write-through round writes the next publish's header ahead; after that publish the served
    header holds new_clock + 1.0 in Python arithmetic -- 2^53 stays 2^53 -- and the publish's
    version, n and dtype; the served payload is the averaged parameters."""
    fp64 = fr.family("fp64")
    cases = [fp64[6], fp64[4], fr.family("contraction")[0], fp64[5], fr.family("contraction")[2]]
    assert fr.evaluate(fp64[4])[1] == fr.evaluate(fp64[5])[1] == 2.0 ** 53 == 2.0 ** 53 + 1.0
    n = forms.big("f32")
    for group in by_cfg(cases):
        pair = forms.Pair("f32", n, group[0])
        try:
            for k, case in enumerate(group):
                flat, check = pair.round(case, write_through=True)
                s = torch.cuda.current_stream()
                _lib.call("dpwa_learner_publish_reuse", pair.me.handle, ptr(flat), 2.5, None,
                          ctypes.c_void_p(s.cuda_stream))
                torch.cuda.synchronize()
                h, payload, version = pair.snapshot(pair.me)
                want = fr.evaluate(case)[1] + 1.0
                assert fr.bits64(h.clock) == fr.bits64(want), (fr.to_literal(case), h.clock.hex(), want.hex())
                assert version == h.version == k + 1 == pair.me.native_version(), (case, version, h.version)
                assert h.n == n and h.dtype == CODE["f32"], (case, h.n, h.dtype)
                assert np.array_equal(payload, forms.tensor_bits(flat)), (case, "the served payload")
                assert pair.me.read_clock() == want, case
                check(case)
        finally:
            pair.close()


# ---------------------------------------------------------------- 7. the kernel variants
VARIANTS = [
    ("DPWA_LERP_BLOCK", "128"),
    ("DPWA_LERP_BLOCK", "256"),
    ("DPWA_LERP_BLOCK", "512"),
    ("DPWA_PAIR_FUSED", "0"),
    ("DPWA_BATCH_SHARE", "0"),
    ("DPWA_BATCH_ORDER", "contiguous"),
    ("DPWA_BATCH_ORDER", "interleaved"),
]


def test_every_variant_in_a_process_of_its_own():
    """tests/factor_worker.py once per knob, one child at a time, as tests/test_gpu_variants.py
    starts tests/forms_worker.py: a mismatch (exit 1) is an ordinary failure and the walk goes on;
    a child that ends abnormally, or with the worker's code for anything but a mismatch (a HIP
    error among them), stops the walk -- nothing more is started after a fault."""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.factor_worker"]
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
        if child.returncode < 0 or child.returncode in ABNORMAL or child.returncode == forms.EXIT_ERROR:
            pytest.fail("%s: ended abnormally (%d); the walk stops here\n%s"
                        % (variant, child.returncode, child.stdout[-4000:]))
        if child.returncode != 0 or "factor_worker: ok" not in child.stdout:
            failed.append("%s: exit %d\n%s" % (variant, child.returncode, child.stdout[-2000:]))
    assert not failed, "\n".join(failed)
