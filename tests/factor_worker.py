"""The device factor on the hard values of tests/factor_ref.py through every kernel that runs it, as
functions that run one form and raise AssertionError on the first mismatch -- used by
tests/test_gpu_factor.py -- and, run as ``python -m tests.factor_worker``, the catching subset
through dpwa_average, dpwa_average_many and dpwa_average_many_resident in a process of its own: the
kernel variants behind DPWA_LERP_BLOCK (wave 0 hands a, b and ok over through LDS),
DPWA_PAIR_FUSED, DPWA_BATCH_SHARE and DPWA_BATCH_ORDER are read once per process.  The worker
exits 0, 1 with the first mismatch printed, or 3 after any other exception (the walk then stops).

Every factor is compared with ``factor_ref.evaluate`` (oracle.policy.factor_and_clock) bit for bit,
NaN payloads excepted.  Operands come from forms_ref.operands, expected parameters from
forms_ref.lerp at the reference factor; destinations lie in forms_ref.guarded bands; every dpwa_coef
and clock pair lies inside 0xA5 bytes (``Ctl``) of which a commit may change the 32 + 8 it owns.

Sizes: 2 * 64 * PER + 1 elements -- a workgroup that commits, a second that only consumes a and b,
and the ragged-tail lane -- and 1 element, the tail alone (the worker: 2 * block * PER + 1 at the
block size under test)."""
import ctypes
import functools
import os
import struct
import sys

import numpy as np
import torch

from dpwa_amd import _lib
from dpwa_amd.flat import c_layout
from dpwa_amd.learner import Learner
from oracle import policy as opolicy
from tests import factor_ref as fr
from tests import forms_ref as ref
from tests import mixed_ref
from tests.forms_ref import CODE, TORCH, tensor_bits
from tests.forms_worker import DEV, OFF, bands, dest, expect, slot_of, source, unchanged
from tests.test_gpu_kernels import header_bytes, ptr, stream

EXIT_ERROR = 3                 # the worker's exit code for anything but a mismatch
SEED = 1                       # forms_ref.operands seeds: entry or learner i uses SEED + i
MIXED_SPEC = [("f32", 5), ("bf16", 9), ("f16", 7)]      # three segments of one 4-KiB block each


def big(dtype, block=64):
    return 2 * block * ref.PER[dtype] + 1


def sizes(dtype):
    return [big(dtype), 1]


@functools.lru_cache(maxsize=None)
def _expected(dtype, n, seed, f_bits):
    p, q = ref.operands(dtype, n, seed)
    want = ref.lerp(dtype, p, q, struct.unpack("<d", struct.pack("<Q", f_bits))[0])
    want.setflags(write=False)
    return want


def expected(dtype, n, seed, f):
    """forms_ref.lerp of the operands of `seed` at the reference factor, computed once."""
    return _expected(dtype, n, seed, fr.bits64(f))


def interp(case):
    method, value, thr = case[:3]
    return _lib.Interp(opolicy.METHODS[method], 0, float(value or 0.0), float(thr))


# ---------------------------------------------------------------- coefficient blocks and clocks
class Ctl:
    """The dpwa_coef (32 B) and the clock pair (16 B) of `count` entries in one allocation of 0xA5
    bytes, 1 KiB per entry: clock[0] holds the entry's clock, everything else is 0xA5 until
    written.  read(i) fetches the bytes back and asserts that only the 32 bytes of the coefficient
    block and the 8 bytes of the clock that the commit owns differ from what was uploaded."""
    STRIDE, COEF, CLOCK = 1024, 256, 640

    def __init__(self, clocks, in_place=False):
        self.in_place = in_place
        self.before = np.full(len(clocks) * self.STRIDE, ref.GUARD_BYTE, np.uint8)
        for i, c in enumerate(clocks):
            at = i * self.STRIDE + self.CLOCK
            self.before[at:at + 8] = np.frombuffer(np.float64(c).tobytes(), np.uint8)
        self.dev = torch.from_numpy(self.before.copy()).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        self.after = None

    def coef_ptr(self, i):
        return self.dev.data_ptr() + i * self.STRIDE + self.COEF

    def clock_ptr(self, i):
        return self.dev.data_ptr() + i * self.STRIDE + self.CLOCK

    def read(self, i, what):
        """(dpwa_coef, the clock written) of entry i."""
        if self.after is None:
            self.after = self.dev.cpu().numpy()
        base = i * self.STRIDE
        own = np.zeros(self.STRIDE, bool)
        own[self.COEF:self.COEF + 32] = True
        out = self.CLOCK if self.in_place else self.CLOCK + 8
        own[out:out + 8] = True
        got, was = self.after[base:base + self.STRIDE], self.before[base:base + self.STRIDE]
        stray = np.flatnonzero((got != was) & ~own)
        assert stray.size == 0, (what, "bytes outside the coefficient block and the clock written changed", stray[:8].tolist())
        coef = _lib.Coef.from_buffer_copy(got[self.COEF:self.COEF + 32].tobytes())
        return coef, np.frombuffer(got[out:out + 8].tobytes(), np.float64)[0].item()


    def untouched(self, i, what):
        """Entry i took no part: its coefficient block and clock pair are as uploaded, all of them."""
        if self.after is None:
            self.after = self.dev.cpu().numpy()
        base = i * self.STRIDE
        stray = np.flatnonzero(self.after[base:base + self.STRIDE] != self.before[base:base + self.STRIDE])
        assert stray.size == 0, (what, "bytes of a learner without an entry changed", stray[:8].tolist())


def check_result(coef, got_clock, case, what):
    """Status, factor, new clock, a and b -- and the clock written -- against the reference."""
    want = fr.evaluate(case)
    assert coef.reserved == 0, (what, coef.reserved)
    if want == fr.ZD:
        assert coef.status == _lib.STATUS_ZERO_DIVISION, (what, coef.status)
        got = (coef.factor, coef.new_clock, coef.a, coef.b)
        assert fr.same_result(got, (0.0, case[3], np.float32(0.0), np.float32(1.0))), (what, got)
        assert fr.bits64(got_clock) == fr.bits64(case[3]), (what, "the clock moved", got_clock.hex(), case[3].hex())
        return
    assert coef.status == _lib.STATUS_OK, (what, coef.status, "reference: %r" % (want,))
    got = (coef.factor, coef.new_clock, coef.a, coef.b)
    assert fr.same_result(got, want), (what, "got %s" % ([float(x).hex() for x in got],),
                                       "want %s" % ([float(x).hex() for x in want],))
    assert fr.same_result((0.0, got_clock, want[2], want[3]), (0.0, want[1], want[2], want[3])), \
        (what, "the clock written", got_clock.hex(), want[1].hex())


def check_params(dtype, p, snap, case, p_bits, seed, what):
    """Zero division: parameters byte-identical; otherwise the reference lerp at the reference
    factor (NaN where it is NaN, bit-equal elsewhere).  A snapshot equals the parameters."""
    want = fr.evaluate(case)
    if want == fr.ZD:
        unchanged(p, p_bits, what)
    else:
        expect(dtype, p, expected(dtype, len(p_bits), seed, want[0]), what)
    if snap is not None:
        unchanged(snap, tensor_bits(p), (what, "the snapshot is not the parameters"))


# ---------------------------------------------------------------- 1. dpwa_factor
def run_factor(case, device_loss):
    """k_factor alone: the clock moves in place; host loss or a device float64."""
    what = ("factor", fr.to_literal(case), device_loss)
    ctl = Ctl([case[3]], in_place=True)
    hdr_h = np.frombuffer(header_bytes(case[4], case[6]), np.uint8)
    hdr = torch.from_numpy(hdr_h.copy()).to(DEV)
    loss_d = torch.tensor([case[5]], dtype=torch.float64, device=DEV) if device_loss else None
    cfg = interp(case)
    _lib.call("dpwa_factor", ctypes.byref(cfg), ctypes.c_void_p(ctl.clock_ptr(0)), ptr(hdr),
              0.0 if device_loss else float(case[5]), ptr(loss_d) if device_loss else None,
              ctypes.c_void_p(ctl.coef_ptr(0)), stream())
    torch.cuda.synchronize()
    check_result(*ctl.read(0, what), case, what)
    assert np.array_equal(hdr.cpu().numpy(), hdr_h), (what, "the peer's header is only read")


# ---------------------------------------------------------------- 2. dpwa_average
def run_average(dtype, n, case, write_through, offsets=(0, 0), tracked=False):
    """One dpwa_average (or dpwa_average_tracked): `offsets` = (parameters, snapshot) in elements
    off the 16-byte alignment -- off it the element-wise kernel runs."""
    what = ("average_tracked" if tracked else "average", dtype, n, fr.to_literal(case), write_through, offsets)
    p_bits, q_bits = ref.operands(dtype, n, SEED)
    p, check = dest(dtype, p_bits, offset=offsets[0])
    slot = slot_of(dtype, q_bits, case[4], case[6])
    snap, check_snap = dest(dtype, n=n, offset=offsets[1]) if write_through else (None, None)
    ctl = Ctl([case[3]])
    cfg = interp(case)
    args = [CODE[dtype], ptr(p), ptr(slot), n, ctypes.byref(cfg), ctypes.c_void_p(ctl.clock_ptr(0)), float(case[5]),
            ctypes.c_void_p(ctl.coef_ptr(0)), ptr(snap) if write_through else None]
    if tracked:
        ws_bytes = ctypes.c_int64()
        _lib.call("dpwa_distance_workspace", ctypes.byref(ws_bytes))
        ws = torch.zeros(ws_bytes.value, dtype=torch.uint8, device=DEV)
        rec = torch.zeros(32, dtype=torch.uint8, device=DEV)
        _lib.call("dpwa_average_tracked", *args, ptr(ws), ptr(rec), stream(), None, None)
    else:
        _lib.call("dpwa_average", *args, stream(), None, None)
    torch.cuda.synchronize()
    bands(what, check, check_snap)
    check_result(*ctl.read(0, what), case, what)
    check_params(dtype, p, snap, case, p_bits, SEED, what)
    unchanged(slot[OFF:].view(TORCH[dtype]), q_bits, (what, "the peer's slot"))
    assert bytes(slot[:256].cpu().numpy()) == header_bytes(case[4], case[6]), (what, "the peer's header")


# ---------------------------------------------------------------- 3. dpwa_average_mixed
@functools.lru_cache(maxsize=None)
def mixed_payloads():
    p, q = mixed_ref.sample(MIXED_SPEC, 29)
    p.setflags(write=False)
    q.setflags(write=False)
    return p, q


def run_mixed(case, write_through):
    """Three segments of one block each.  Every segment, its zero padding included (0 * a + 0 * b:
    zeros at a finite factor, NaN at a NaN one), against its dtype's reference."""
    what = ("average_mixed", fr.to_literal(case), write_through)
    segs, total = mixed_ref.segments(MIXED_SPEC)
    assert [length for _, _, length, _ in segs] == [mixed_ref.BLOCK] * 3
    lay = tuple((mixed_ref.TORCH[d], off, length) for d, off, length, _ in segs)
    p_h, q_h = mixed_payloads()
    p, check = ref.guarded(total)
    p.copy_(torch.from_numpy(np.array(p_h)))
    slot = torch.zeros(OFF + total + ref.GUARD, dtype=torch.uint8, device=DEV)[:OFF + total]
    slot[:256].copy_(torch.frombuffer(bytearray(header_bytes(case[4], case[6])), dtype=torch.uint8))
    slot[OFF:].copy_(torch.from_numpy(np.array(q_h)))
    snap, check_snap = ref.guarded(total) if write_through else (None, None)
    ctl = Ctl([case[3]])
    cfg = interp(case)
    _lib.call("dpwa_average_mixed", ctypes.byref(c_layout(lay)), ptr(p), ptr(slot), ctypes.byref(cfg),
              ctypes.c_void_p(ctl.clock_ptr(0)), float(case[5]), ctypes.c_void_p(ctl.coef_ptr(0)),
              ptr(snap) if write_through else None, stream(), None, None)
    torch.cuda.synchronize()
    bands(what, check, check_snap)
    check_result(*ctl.read(0, what), case, what)
    got, want = p.cpu().numpy(), fr.evaluate(case)
    if want == fr.ZD:
        assert np.array_equal(got, p_h), (what, "changed")
    else:
        for d, off, length, _ in segs:
            view = lambda a: np.ascontiguousarray(a[off:off + length]).view(ref.NUMPY[d])       # noqa: E731
            w = ref.lerp(d, view(p_h), view(q_h), want[0])
            assert ref.same(d, view(got), w), (what, d, ref.mismatches(d, view(got), w))
    if write_through:
        assert torch.equal(snap, p), (what, "the snapshot is not the parameters")
    assert np.array_equal(slot[OFF:].cpu().numpy(), q_h), (what, "the peer's slot")


# ---------------------------------------------------------------- 4. dpwa_average_many
def run_many(dtype, name, pattern, cases, write_through, block=64):
    """One dispatch, one case per entry: every entry exactly its own reference, whatever its
    neighbours do (a zero division that does not average, a NaN factor)."""
    ents = []
    for i, case in enumerate(cases):
        n = 1 if pattern == "unequal" and i % 2 else big(dtype, block)
        p_bits, q_bits = ref.operands(dtype, n, SEED + i)
        p, check = dest(dtype, p_bits)
        snap, check_snap = dest(dtype, n=n) if write_through else (None, None)
        ents.append(dict(n=n, i=i, case=case, p_bits=p_bits, q_bits=q_bits, p=p, check=check, snap=snap,
                         check_snap=check_snap, slot=slot_of(dtype, q_bits, case[4], case[6])))
    ctl = Ctl([c[3] for c in cases])
    d = (_lib.AverageDesc * len(ents))()
    for j, e in enumerate(ents):
        d[j] = _lib.AverageDesc(e["p"].data_ptr(), e["slot"].data_ptr(), e["n"], ctl.clock_ptr(j), e["case"][5],
                                ctl.coef_ptr(j), e["snap"].data_ptr() if write_through else None)
    cfg = interp(cases[0])
    _lib.call("dpwa_average_many", CODE[dtype], d, len(ents), ctypes.byref(cfg), stream(), None, None)
    torch.cuda.synchronize()
    for e in ents:
        what = ("average_many", dtype, name, write_through, "entry %d" % e["i"], fr.to_literal(e["case"]))
        bands(what, e["check"], e["check_snap"])
    for e in ents:
        what = ("average_many", dtype, name, write_through, "entry %d" % e["i"], fr.to_literal(e["case"]))
        check_result(*ctl.read(e["i"], what), e["case"], what)
        check_params(dtype, e["p"], e["snap"], e["case"], e["p_bits"], SEED + e["i"], what)
        unchanged(e["slot"][OFF:].view(TORCH[dtype]), e["q_bits"], (what, "the peer's slot"))


# ---------------------------------------------------------------- 5. dpwa_average_many_resident
def run_resident(dtype, n, label, learners, entries, cases):
    """One dispatch of a factor_ref.resident_dispatches row: learner i has one clock and one
    published slot; every entry's average lands in its learner's guarded next slot."""
    ls = []
    for i, (clock, loss) in enumerate(learners):
        bits = ref.operands(dtype, n, (SEED + i, SEED + i))[0]
        nxt, check = dest(dtype, n=n)
        ls.append(dict(bits=bits, slot=slot_of(dtype, bits, clock, loss), next=nxt, check=check))
    ctl = Ctl([clock for clock, _ in learners])
    d = (_lib.AverageDesc * len(entries))()
    for j, (a, b, loss) in enumerate(entries):
        d[j] = _lib.AverageDesc(ls[a]["slot"].data_ptr() + OFF, ls[b]["slot"].data_ptr(), n, ctl.clock_ptr(a), loss,
                                ctl.coef_ptr(a), ls[a]["next"].data_ptr())
    before = [lr["slot"].clone() for lr in ls]
    cfg = interp(cases[0])
    _lib.call("dpwa_average_many_resident", CODE[dtype], d, len(entries), ctypes.byref(cfg), stream(), None, None)
    torch.cuda.synchronize()
    for i, (lr, b) in enumerate(zip(ls, before)):
        assert torch.equal(lr["slot"], b), ("resident", dtype, label, "published slot %d changed" % i)
        lr["check"](("resident", dtype, label, "next slot %d" % i))
    for j, ((a, b, _), case) in enumerate(zip(entries, cases)):
        what = ("resident", dtype, n, label, "entry %d: %d with %d" % (j, a, b), fr.to_literal(case))
        check_result(*ctl.read(a, what), case, what)
        want = fr.evaluate(case)
        if want == fr.ZD:
            unchanged(ls[a]["next"], ls[a]["bits"], what)         # the parameters move on as they are
        else:
            expect(dtype, ls[a]["next"], expected(dtype, n, (SEED + a, SEED + b), want[0]), what)
    mine = {a for a, _, _ in entries}
    for i, lr in enumerate(ls):
        if i not in mine:                                          # a peer outside the dispatch has no output
            assert bool((lr["next"].view(torch.uint8) == ref.GUARD_BYTE).all()), ("resident", dtype, label, i)
            ctl.untouched(i, ("resident", dtype, label, "learner %d has no entry" % i))


def run_resident_all(dtype, name, n):
    for label, learners, entries, cases in fr.resident_dispatches(name):
        run_resident(dtype, n, label, learners, entries, cases)


# ---------------------------------------------------------------- 6. through a learner
class Pair:
    """A learner of `cfg_case`'s (method, value, threshold) and the peer it averages with.  The
    peer's publish writes clock + 1.0 into its header, so its clock is set to pc - 1.0 first
    (factor_ref.learner_ok: that gives pc back exactly)."""

    def __init__(self, dtype, n, cfg_case, track=False):
        self.dtype, self.n, self.cfg = dtype, n, fr.cfg_of(cfg_case)
        cfg = interp(cfg_case)
        self.me, self.peer = Learner(DEV, n, TORCH[dtype], cfg), Learner(DEV, n, TORCH[dtype], cfg)
        if track:
            _lib.call("dpwa_learner_set_distance", self.me.handle, 1)
        self.me.attach_local(0, self.peer)
        self.p_bits, self.q_bits = ref.operands(dtype, n, SEED)
        self.q = source(dtype, self.q_bits)

    def close(self):
        self.me.close()
        self.peer.close()

    def round(self, case, write_through=False, loss=None):
        """One average of fresh parameters with the peer's fresh snapshot; `loss`: what to give as
        the loss (a number or a device tensor), case[5] by default.  Returns (parameters, band
        check); the factor, clock and parameters have been compared with the reference."""
        assert fr.learner_ok(case) and fr.cfg_of(case) == self.cfg, case
        what = ("learner", self.dtype, self.n, fr.to_literal(case), write_through, str(getattr(loss, "dtype", "host")))
        s = torch.cuda.current_stream()
        self.peer.write_clock(case[4] - 1.0)
        self.peer.publish(self.q, case[6], s)
        flat, check = dest(self.dtype, self.p_bits)
        self.me.write_clock(case[3])
        self.me.fetch(0, self.peer.version, True, s)
        h, d, keep = self.me.loss_args(case[5] if loss is None else loss)
        _lib.call("dpwa_learner_average_through" if write_through else "dpwa_learner_average", self.me.handle,
                  ptr(flat), h, d, ctypes.c_void_p(s.cuda_stream))
        torch.cuda.synchronize()
        del keep
        bands(what, check)
        check_result(self.me.read_coef(), self.me.read_clock(), case, what)
        check_params(self.dtype, flat, None, case, self.p_bits, SEED, what)
        unchanged(self.q, self.q_bits, (what, "the peer's parameters"))
        return flat, check

    def snapshot(self, learner):
        out = np.zeros(self.n, ref.NUMPY[self.dtype])
        hdr, v = ctypes.create_string_buffer(256), ctypes.c_uint64()
        _lib.call("dpwa_learner_read_snapshot", learner.handle, hdr, ctypes.c_void_p(out.ctypes.data), out.nbytes,
                  ctypes.byref(v))
        return _lib.Header.from_buffer_copy(hdr.raw), out, v.value


# ---------------------------------------------------------------- the worker
def main():
    block = int(os.environ.get("DPWA_LERP_BLOCK", "64"))
    for dtype in ("f32", "bf16"):
        for case in fr.CATCHING:
            for write_through in (False, True):
                run_average(dtype, big(dtype, block), case, write_through)
    for k, (name, pattern, cases) in enumerate(fr.many_dispatches()):
        run_many("f32", name, pattern, cases, write_through=bool(k % 2), block=block)
    for name in fr.TOPOLOGIES:
        run_resident_all("f32", name, big("f32", block))
    print("factor_worker: ok")


if __name__ == "__main__":
    try:
        main()
    except AssertionError as e:
        print("factor_worker: MISMATCH %s" % (e,), flush=True)
        sys.exit(1)
    except Exception as e:                 # a failed call, a HIP error: not a mismatch -- the walk stops
        print("factor_worker: ERROR %s: %s" % (type(e).__name__, e), flush=True)
        sys.exit(EXIT_ERROR)
