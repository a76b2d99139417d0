"""The averaging forms whose cache policy follows the bytes of the launch (kernels.hip lerp_policy:
k_lerp plain and write-through, k_lerp_batch, k_lerp_tracked, k_lerp_mixed -- none of them resident),
at span edges, in a process of its own: DPWA_CACHE_FIT_BYTES and DPWA_LERP_POLICY are read once per
process, so tests/test_gpu_policy_by_size.py starts one worker per setting.  A policy is cache bits on
the same loads and stores, so every setting must give the host references' bits (oracle.lerp through
forms_ref.lerp, oracle.policy through factor_ref.evaluate).

Shapes: float32 n in {1, 255, 257, 4099} (the tail alone; one element short of a one-wave span of 256;
one over it; 17 spans and a tail), bfloat16 n in {9, 2053} (one item and a tail; five spans and a
tail), batches of two such entries, one mixed layout of two 4-KiB segments.

Run as ``python -m tests.policy_worker``: exits 0 after printing how many launches fell below, on and
above the threshold in force (3 x payload bytes against DPWA_CACHE_FIT_BYTES), 1 with the first
mismatch printed, 3 after any other exception."""
import ctypes
import os
import sys

import numpy as np
import torch

from dpwa_amd import _lib
from dpwa_amd.flat import c_layout
from tests import factor_ref as fr
from tests import factor_worker as fw
from tests import forms_ref as ref
from tests import mixed_ref
from tests.forms_ref import CODE, SIZE, TORCH
from tests.forms_worker import DEV, OFF, bands, dest, expect, lerp_call, slot_of, source, unchanged
from tests.test_gpu_kernels import header_bytes, ptr, stream

SHAPES = [("f32", 1), ("f32", 255), ("f32", 257), ("f32", 4099), ("bf16", 9), ("bf16", 2053)]
BATCHES = [("f32", (1, 255)), ("f32", (257, 4099)), ("bf16", (9, 2053))]
MIXED_SPEC = [("f32", 5), ("bf16", 9)]          # two segments of one 4-KiB block each
CASE = ("clock", None, 0.0, 3.0, 7.0, 1.0, 1.0)  # clock interpolation, 3 meets 7
FACTOR = 0.3
SEED = fw.SEED
EXIT_ERROR = 3

TALLY = {"below": 0, "on": 0, "above": 0}


def note(payload_bytes):
    """Which side of the threshold in force a launch of `payload_bytes` falls on."""
    fit = int(os.environ.get("DPWA_CACHE_FIT_BYTES", "-1"))
    if fit < 0:
        return
    TALLY["below" if 3 * payload_bytes < fit else "on" if 3 * payload_bytes == fit else "above"] += 1


def run_lerp(dtype, n):
    """dpwa_lerp_* with a host factor and a device coefficient block (k_lerp, COEF_HOST / COEF_DEV)."""
    p_bits, q_bits = ref.operands(dtype, n, SEED)
    want = ref.lerp(dtype, p_bits, q_bits, FACTOR)
    q = source(dtype, q_bits)
    for mode in ("host", "device"):
        what = ("lerp", dtype, n, mode)
        p, check = dest(dtype, p_bits)
        lerp_call(dtype, mode, p, q, FACTOR)
        note(n * SIZE[dtype])
        bands(what, check)
        expect(dtype, p, want, what)
    unchanged(q, q_bits, ("lerp: the peer", dtype, n))


def run_average(dtype, n, write_through, tracked):
    fw.run_average(dtype, n, CASE, write_through, tracked=tracked)
    note(n * SIZE[dtype])


def run_batch(dtype, sizes, write_through):
    """One dpwa_average_many of two entries: the policy goes by the sum of their bytes."""
    ents = []
    for i, n in enumerate(sizes):
        p_bits, q_bits = ref.operands(dtype, n, SEED + i)
        p, check = dest(dtype, p_bits)
        snap, check_snap = dest(dtype, n=n) if write_through else (None, None)
        ents.append(dict(n=n, i=i, p_bits=p_bits, q_bits=q_bits, p=p, check=check, snap=snap, check_snap=check_snap,
                         slot=slot_of(dtype, q_bits, CASE[4], CASE[6])))
    ctl = fw.Ctl([CASE[3]] * len(ents))
    d = (_lib.AverageDesc * len(ents))()
    for j, e in enumerate(ents):
        d[j] = _lib.AverageDesc(e["p"].data_ptr(), e["slot"].data_ptr(), e["n"], ctl.clock_ptr(j), CASE[5],
                                ctl.coef_ptr(j), e["snap"].data_ptr() if write_through else None)
    cfg = fw.interp(CASE)
    _lib.call("dpwa_average_many", CODE[dtype], d, len(ents), ctypes.byref(cfg), stream(), None, None)
    torch.cuda.synchronize()
    note(sum(sizes) * SIZE[dtype])
    for e in ents:
        bands(("average_many", dtype, sizes, write_through, "entry %d" % e["i"]), e["check"], e["check_snap"])
    for e in ents:
        what = ("average_many", dtype, sizes, write_through, "entry %d" % e["i"])
        fw.check_result(*ctl.read(e["i"], what), CASE, what)
        fw.check_params(dtype, e["p"], e["snap"], CASE, e["p_bits"], SEED + e["i"], what)
        unchanged(e["slot"][OFF:].view(TORCH[dtype]), e["q_bits"], (what, "the peer's slot"))


def run_mixed(write_through):
    """dpwa_average_mixed over a float32 and a bfloat16 segment of one block each: every segment, its
    zero padding included, against its dtype's reference."""
    what = ("average_mixed", write_through)
    segs, total = mixed_ref.segments(MIXED_SPEC)
    assert [length for _, _, length, _ in segs] == [mixed_ref.BLOCK] * 2
    lay = tuple((mixed_ref.TORCH[d], off, length) for d, off, length, _ in segs)
    p_h, q_h = mixed_ref.sample(MIXED_SPEC, 31)
    p, check = ref.guarded(total)
    p.copy_(torch.from_numpy(np.array(p_h)))
    slot = torch.zeros(OFF + total + ref.GUARD, dtype=torch.uint8, device=DEV)[:OFF + total]
    slot[:256].copy_(torch.frombuffer(bytearray(header_bytes(CASE[4], CASE[6])), dtype=torch.uint8))
    slot[OFF:].copy_(torch.from_numpy(np.array(q_h)))
    snap, check_snap = ref.guarded(total) if write_through else (None, None)
    ctl = fw.Ctl([CASE[3]])
    cfg = fw.interp(CASE)
    _lib.call("dpwa_average_mixed", ctypes.byref(c_layout(lay)), ptr(p), ptr(slot), ctypes.byref(cfg),
              ctypes.c_void_p(ctl.clock_ptr(0)), float(CASE[5]), ctypes.c_void_p(ctl.coef_ptr(0)),
              ptr(snap) if write_through else None, stream(), None, None)
    torch.cuda.synchronize()
    note(total)
    bands(what, check, check_snap)
    fw.check_result(*ctl.read(0, what), CASE, what)
    got, f = p.cpu().numpy(), fr.evaluate(CASE)[0]
    for d, off, length, _ in segs:
        view = lambda a: np.ascontiguousarray(a[off:off + length]).view(ref.NUMPY[d])       # noqa: E731
        w = ref.lerp(d, view(p_h), view(q_h), f)
        assert ref.same(d, view(got), w), (what, d, ref.mismatches(d, view(got), w))
    if write_through:
        assert torch.equal(snap, p), (what, "the snapshot is not the parameters")
    assert np.array_equal(slot[OFF:].cpu().numpy(), q_h), (what, "the peer's slot")


def main():
    for dtype, n in SHAPES:
        run_lerp(dtype, n)
        for write_through in (False, True):
            for tracked in (False, True):
                run_average(dtype, n, write_through, tracked)
    for dtype, sizes in BATCHES:
        for write_through in (False, True):
            run_batch(dtype, sizes, write_through)
    for write_through in (False, True):
        run_mixed(write_through)
    print("policy_worker: ok below=%(below)d on=%(on)d above=%(above)d" % TALLY)


if __name__ == "__main__":
    try:
        main()
    except AssertionError as e:
        print("policy_worker: MISMATCH %s" % (e,), flush=True)
        sys.exit(1)
    except Exception as e:                 # a failed call, a HIP error: not a mismatch -- the walk stops
        print("policy_worker: ERROR %r" % (e,), flush=True)
        sys.exit(EXIT_ERROR)
