"""The forms of the averaging kernel on hard values with guard bands, as functions that run one
form and raise AssertionError on the first mismatch -- used by tests/test_gpu_forms.py -- and, run
as ``python -m tests.forms_worker``, a compact subset of them for float32 and bfloat16 in a
process of its own: the kernel variants behind environment knobs (DPWA_LERP_BLOCK,
DPWA_LERP_POLICY, DPWA_PAIR_FUSED, DPWA_BATCH_SHARE, DPWA_BATCH_ORDER, DPWA_PUBLISH_BLOCK) are
read once per process, so tests/test_gpu_variants.py starts one worker per variant.  The worker
exits 0, or 1 with the first mismatch printed.

Every destination (parameters, write-through snapshot, next slot) lies between two 8-KiB guard
bands (forms_ref.guarded) that are checked after the call; every source is compared with its host
copy afterwards.  Operands and expected values come from forms_ref.case -- host references only."""
import ctypes
import os
import sys

import numpy as np
import torch

from dpwa_amd import _lib
from dpwa_amd.learner import Learner
from tests import forms_ref as ref
from tests.forms_ref import CODE, SIZE, TORCH, tensor_bits
from tests.test_gpu_f16 import FUSED, average
from tests.test_gpu_kernels import average_slot, coef_block, ptr, stream

DEV = torch.device("cuda", 0)
OFF = _lib.SLOT_PAYLOAD_OFFSET
LERP = {"f32": "dpwa_lerp_f32", "bf16": "dpwa_lerp_bf16", "f16": "dpwa_lerp_f16"}


def raw(bits):
    """A CPU uint8 tensor over a copy of the bit patterns (the shared arrays are read-only)."""
    return torch.from_numpy(np.array(bits).view(np.uint8))


def source(dtype, bits):
    """A buffer the kernels only read (with a guard band's room behind it, so that a span read past
    the end stays inside the allocation)."""
    whole = torch.zeros(len(bits) * SIZE[dtype] + ref.GUARD, dtype=torch.uint8, device=DEV)
    whole[:len(bits) * SIZE[dtype]].copy_(raw(bits))
    return whole[:len(bits) * SIZE[dtype]].view(TORCH[dtype])


def slot_of(dtype, bits, clock, loss):
    """A peer's published slot holding `bits` (test_gpu_kernels.average_slot), with the same room
    behind it."""
    nbytes = OFF + len(bits) * SIZE[dtype]
    whole = torch.zeros(nbytes + ref.GUARD, dtype=torch.uint8, device=DEV)
    whole[:nbytes].copy_(average_slot(raw(bits).to(DEV).view(TORCH[dtype]), clock, loss))
    return whole[:nbytes]


def dest(dtype, bits=None, n=None, offset=0):
    """(tensor, check) of a guarded destination `offset` elements off the 16-byte alignment,
    holding `bits`, or n elements of 0xA5 bytes."""
    n = len(bits) if bits is not None else n
    payload, check = ref.guarded(n * SIZE[dtype], offset * SIZE[dtype])
    if bits is not None:
        payload.copy_(raw(bits))
    return payload.view(TORCH[dtype]), check


def bands(what, *checks):
    """The guard bands of every destination of a call, looked at before any value: an overrun is
    the plainer finding, and it spoils values too (the tail is averaged twice)."""
    for check in checks:
        if check is not None:
            check(what)


def expect(dtype, got, want, what):
    got = tensor_bits(got) if isinstance(got, torch.Tensor) else got
    assert ref.same(dtype, got, want), (what, ref.mismatches(dtype, got, want))


def unchanged(t, bits, what):
    """Byte for byte (a source that is only read, parameters after a no-op round)."""
    assert np.array_equal(tensor_bits(t), bits), (what, "changed")


def lerp_call(dtype, mode, p, q, f):
    if mode == "host":
        _lib.call(LERP[dtype] + "_host", ptr(p), ptr(q), p.numel(), float(f), stream())
    else:
        coef = coef_block(f)
        _lib.call(LERP[dtype], ptr(p), ptr(q), p.numel(), ptr(coef), stream())
    torch.cuda.synchronize()


def read_coef(t):
    return _lib.Coef.from_buffer_copy(t.cpu().numpy().tobytes())


def check_coef(c, f, new_clock, got_clock, what):
    assert c.status == 0 and c.factor == f, (what, c.status, c.factor, f)
    assert c.a == np.float32(f) and c.b == np.float32(1.0 - f), (what, c.a, c.b)
    assert got_clock == new_clock == c.new_clock, (what, got_clock, new_clock, c.new_clock)     # dpwa.py:150


# ---------------------------------------------------------------- 1. every bf16 bit pattern
def run_every_bf16_pattern(f):
    want = ref.every_bf16_pattern_expected(f)
    q = source("bf16", ref.PATTERNS_BF16)
    for mode in ("host", "device"):
        p, check = dest("bf16", ref.PERM_BF16)
        lerp_call("bf16", mode, p, q, f)
        bands((f, mode), check)
        expect("bf16", p, want, (f, mode))
    unchanged(q, ref.PATTERNS_BF16, "the peer")


# ---------------------------------------------------------------- 2. plain lerp
def run_plain(dtype, n, f):
    p_bits, q_bits, want = ref.case(dtype, n, ref.seed_of(dtype, n), f)
    q = source(dtype, q_bits)
    for mode in ("host", "device"):
        what = ("lerp", dtype, n, f, mode)
        p, check = dest(dtype, p_bits)
        lerp_call(dtype, mode, p, q, f)
        bands(what, check)
        expect(dtype, p, want, what)
    unchanged(q, q_bits, ("lerp: the peer", dtype, n, f))


# ---------------------------------------------------------------- 3. unaligned views
def run_unaligned(dtype, k):
    """Offset pair k: plain lerp with the parameters off_p and the peer off_q elements off the
    alignment; dpwa_average with the parameters off_p off it (the peer's slot stays aligned: its
    header is read as doubles), without a snapshot and with one off_q off it; and the zero-division
    branch of that, which copies the parameters to the snapshot."""
    n = ref.UNALIGNED_N
    off_p, off_q = ref.UNALIGNED_OFFSETS[k]
    seed = ref.seed_of(dtype, n, k)
    p_bits, q_bits, want = ref.case(dtype, n, seed, 0.3)
    for mode in ("host", "device"):
        what = ("unaligned lerp", dtype, off_p, off_q, mode)
        p, check = dest(dtype, p_bits, offset=off_p)
        q, check_q = dest(dtype, q_bits, offset=off_q)
        lerp_call(dtype, mode, p, q, 0.3)
        bands(what, check, check_q)
        expect(dtype, p, want, what)
        unchanged(q, q_bits, what)
    for case in (ref.UNALIGNED_CASE, ref.ZERO_DIVISION):
        for write_through in (False, True):
            what = ("unaligned average", dtype, off_p, off_q, case, write_through)
            p, check = dest(dtype, p_bits, offset=off_p)
            slot = slot_of(dtype, q_bits, case[4], case[6])
            snap, check_snap = dest(dtype, n=n, offset=off_q) if write_through else (None, None)
            c, got_clock = average(CODE[dtype], p, slot, n, case, snap)
            bands(what, check, check_snap)
            if case is ref.ZERO_DIVISION:
                assert c.status == _lib.STATUS_ZERO_DIVISION and got_clock == case[3], what
                unchanged(p, p_bits, what)
            else:
                f, new_clock = ref.fused_factor(case)
                expect(dtype, p, ref.case(dtype, n, seed, f)[2], what)
                check_coef(c, f, new_clock, got_clock, what)
            if write_through:
                unchanged(snap, tensor_bits(p), (what, "the snapshot is not the parameters"))
            unchanged(slot[OFF:].view(TORCH[dtype]), q_bits, (what, "the peer's slot"))


# ---------------------------------------------------------------- 4. dpwa_average
def run_average(dtype, n, write_through):
    """The five policy cases and the zero-division no-op, plain or write-through."""
    seed = ref.seed_of(dtype, n)
    for case in FUSED + [ref.ZERO_DIVISION]:
        what = ("average", dtype, n, case, write_through)
        p_bits, q_bits = ref.operands(dtype, n, seed)
        p, check = dest(dtype, p_bits)
        slot = slot_of(dtype, q_bits, case[4], case[6])
        snap, check_snap = dest(dtype, n=n) if write_through else (None, None)
        c, got_clock = average(CODE[dtype], p, slot, n, case, snap)
        bands(what, check, check_snap)
        if case is ref.ZERO_DIVISION:
            assert c.status == _lib.STATUS_ZERO_DIVISION and got_clock == case[3], what
            unchanged(p, p_bits, what)
        else:
            f, new_clock = ref.fused_factor(case)
            expect(dtype, p, ref.case(dtype, n, seed, f)[2], what)
            check_coef(c, f, new_clock, got_clock, what)
        if write_through:
            unchanged(snap, tensor_bits(p), (what, "the snapshot is not the parameters"))
        unchanged(slot[OFF:].view(TORCH[dtype]), q_bits, (what, "the peer's slot"))


# ---------------------------------------------------------------- 5. dpwa_average_many
def run_many(dtype, group, write_through, zero_division=False):
    """One dispatch over the entries of forms_ref.many_sizes(dtype)[group]; with `zero_division`
    entry 0 has both clocks 0 and must stay as it is while the others average."""
    ents = []
    for i, n in enumerate(ref.many_sizes(dtype)[group]):
        case = ref.many_case(i)
        if zero_division and i == 0:
            case = case[:3] + (0.0, 0.0) + case[5:]
        p_bits, q_bits = ref.operands(dtype, n, ref.seed_of(dtype, n, i))
        p, check = dest(dtype, p_bits)
        snap, check_snap = dest(dtype, n=n) if write_through else (None, None)
        ents.append(dict(n=n, i=i, case=case, p_bits=p_bits, q_bits=q_bits, p=p, check=check, snap=snap,
                         check_snap=check_snap, slot=slot_of(dtype, q_bits, case[4], case[6]),
                         clock=torch.tensor([case[3], -1.0], dtype=torch.float64, device=DEV),
                         coef=torch.zeros(32, dtype=torch.uint8, device=DEV)))
    d = (_lib.AverageDesc * len(ents))()
    for j, e in enumerate(ents):
        d[j] = _lib.AverageDesc(e["p"].data_ptr(), e["slot"].data_ptr(), e["n"], e["clock"].data_ptr(), e["case"][5],
                                e["coef"].data_ptr(), e["snap"].data_ptr() if write_through else None)
    cfg = _lib.Interp(_lib.INTERP_CLOCK, 0, 0.0, 0.0)
    _lib.call("dpwa_average_many", CODE[dtype], d, len(ents), ctypes.byref(cfg), stream(), None, None)
    torch.cuda.synchronize()
    for e in ents:
        bands(("average_many", dtype, group, write_through, zero_division, "entry %d" % e["i"]), e["check"],
              e["check_snap"])
    for e in ents:
        what = ("average_many", dtype, group, write_through, zero_division, "entry %d" % e["i"])
        c, got_clock = read_coef(e["coef"]), e["clock"][1].item()
        if zero_division and e["i"] == 0:
            assert c.status == _lib.STATUS_ZERO_DIVISION and got_clock == 0.0, what
            unchanged(e["p"], e["p_bits"], what)
        else:
            f, new_clock = ref.fused_factor(e["case"])
            expect(dtype, e["p"], ref.case(dtype, e["n"], ref.seed_of(dtype, e["n"], e["i"]), f)[2], what)
            check_coef(c, f, new_clock, got_clock, what)
        if write_through:
            unchanged(e["snap"], tensor_bits(e["p"]), (what, "the snapshot is not the parameters"))
        unchanged(e["slot"][OFF:].view(TORCH[dtype]), e["q_bits"], (what, "the peer's slot"))


# ---------------------------------------------------------------- 6. dpwa_average_many_resident
def run_resident(dtype, name, n):
    """One dispatch of the topology forms_ref.RESIDENT[name]: every average lands in its entry's
    guarded next slot, equal to the reference and to the same average done alone through
    dpwa_average; the published slots are only read; a zero-dividing entry's next slot receives its
    parameters and its clock stays."""
    picks = ref.RESIDENT[name]
    count = 1 + max(max(a, b) for a, b in picks)
    base = ref.seed_of(dtype, n)
    ls = []
    for i in range(count):
        clock, loss = ref.resident_learner(i, name)
        bits = ref.operands(dtype, n, (base + i, base + i))[0]
        nxt, check = dest(dtype, n=n)
        ls.append(dict(bits=bits, clock_val=clock, loss=loss, slot=slot_of(dtype, bits, clock, loss),
                       next=nxt, check=check, clock=torch.tensor([clock, -1.0], dtype=torch.float64, device=DEV),
                       coef=torch.zeros(32, dtype=torch.uint8, device=DEV)))
    d = (_lib.AverageDesc * len(picks))()
    for j, (a, b) in enumerate(picks):
        me, peer = ls[a], ls[b]
        d[j] = _lib.AverageDesc(me["slot"].data_ptr() + OFF, peer["slot"].data_ptr(), n, me["clock"].data_ptr(),
                                ref.resident_entry(name, j)[1], me["coef"].data_ptr(), me["next"].data_ptr())
    before = [lr["slot"].clone() for lr in ls]
    method = ref.resident_entry(name, 0)[0]
    cfg = _lib.Interp(_lib.INTERP_CLOCK if method == "clock" else _lib.INTERP_LOSS, 0, 0.0, 0.0)
    _lib.call("dpwa_average_many_resident", CODE[dtype], d, len(picks), ctypes.byref(cfg), stream(), None, None)
    torch.cuda.synchronize()
    for i, (lr, b) in enumerate(zip(ls, before)):
        assert torch.equal(lr["slot"], b), ("resident", dtype, name, n, "published slot %d changed" % i)
        lr["check"](("resident", dtype, name, n, "next slot %d" % i))
    for j, (a, b) in enumerate(picks):
        what = ("resident", dtype, name, n, "entry %d: %d with %d" % (j, a, b))
        me, peer = ls[a], ls[b]
        res = ref.resident_factor(name, j)
        c, got_clock = read_coef(me["coef"]), me["clock"][1].item()
        if res is None:
            assert c.status == _lib.STATUS_ZERO_DIVISION and got_clock == me["clock_val"], what
            unchanged(me["next"], me["bits"], what)
            continue
        f, new_clock = res
        expect(dtype, me["next"], ref.case(dtype, n, (base + a, base + b), f)[2], what)
        check_coef(c, f, new_clock, got_clock, what)
        alone = source(dtype, me["bits"])
        case = (method, None, 0.0, me["clock_val"], peer["clock_val"], ref.resident_entry(name, j)[1], peer["loss"])
        average(CODE[dtype], alone, peer["slot"], n, case, None)
        expect(dtype, me["next"], tensor_bits(alone), (what, "differs from the same average done alone"))
    mine = {a for a, _ in picks}
    for i, lr in enumerate(ls):
        if i not in mine:           # a peer outside the dispatch has no output
            assert bool((lr["next"].view(torch.uint8) == ref.GUARD_BYTE).all()), ("resident", dtype, name, n, i)


# ---------------------------------------------------------------- publish (DPWA_PUBLISH_BLOCK)
def run_publish(dtype, n):
    """One Learner.publish of a ragged payload (bytes & 15 != 0), read back with read_snapshot."""
    assert (n * SIZE[dtype]) & 15
    bits = ref.operands(dtype, n, ref.SEEDS.get((dtype, n), 1))[0]
    flat = source(dtype, bits)
    lr = Learner(DEV, n, TORCH[dtype], _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0))
    try:
        lr.publish(flat, 1.25, torch.cuda.current_stream())
        torch.cuda.synchronize()
        out = np.zeros(n, ref.NUMPY[dtype])
        hdr, v = ctypes.create_string_buffer(256), ctypes.c_uint64()
        _lib.call("dpwa_learner_read_snapshot", lr.handle, hdr, ctypes.c_void_p(out.ctypes.data), out.nbytes,
                  ctypes.byref(v))
        h = _lib.Header.from_buffer_copy(hdr.raw)
        what = ("publish", dtype, n)
        assert v.value == 1 and h.version == 1 and h.n == n and h.dtype == CODE[dtype] and h.loss == 1.25, what
        assert h.clock == 1.0, what                                   # dpwa.py:112
        assert np.array_equal(out, bits), (what, "the snapshot is not the payload",
                                           np.flatnonzero(out != bits)[:5].tolist())
        unchanged(flat, bits, what)
    finally:
        lr.close()


# ---------------------------------------------------------------- the worker
def main():
    wide = os.environ.get("DPWA_LERP_BLOCK") == "512"
    for dtype in ("f32", "bf16"):
        for n in ref.worker_sizes(dtype, wide):
            for f in ref.PLAIN_FACTORS:
                run_plain(dtype, n, f)
            for write_through in (False, True):
                run_average(dtype, n, write_through)
        for write_through in (False, True):
            run_many(dtype, "equal", write_through)
            run_many(dtype, "nine", write_through, zero_division=write_through)
        for name in ref.RESIDENT:
            for n in ref.worker_sizes(dtype):
                run_resident(dtype, name, n)
        if os.environ.get("DPWA_PUBLISH_BLOCK"):
            for n in [ref.worker_sizes(dtype)[1]] + ref.ragged_publish_elements(dtype):
                run_publish(dtype, n)
    print("forms_worker: ok")


if __name__ == "__main__":
    try:
        main()
    except AssertionError as e:
        print("forms_worker: MISMATCH %s" % (e,), flush=True)
        sys.exit(1)
