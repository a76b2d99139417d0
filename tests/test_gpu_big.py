"""Every streaming kernel of dpwa_amd/csrc/kernels.hip on payloads that cross element 2^31 and byte
2^32, against the host model of tests/big_ref.py (tests/test_big_host.py shows without a GPU that
these checks tell the model from every slip of big_ref.MUTANTS).  Everything but the relay case runs in
this process through the C ABI (dpwa_amd._lib) and dpwa_amd.learner.Learner.

Operands are a constant bit pattern with 4-KiB windows of seeded values at byte 0, around bytes 2^31 and
2^32, over the ragged end and around every segment or tensor border.  Every destination lies between
forms_ref.guarded bands; its windows are copied back and compared with the host reference (NaN
positions coincide, every other element bit-equal; byte-equal for the byte movers); every other
element is compared on the device, in chunks of 2^28 elements, with the host-computed constant by an
integer != and nonzero, and every position listed must lie in a window; every source is checked the
same way afterwards.  The sums are compared with == (the exact family of big_ref).  Nothing here reads
out of range on purpose.  After a DPWA_ERR_HIP or a HIP error from torch every later test of the module
fails at once without touching the GPU.

Which case runs which kernel beyond 2^32 bytes:
  k_lerp (COEF_HOST, COEF_DEV)          test_lerp (bf16, f32, f16)
  k_lerp (COEF_FUSED, plain and DUAL)   test_average (bf16, f32; plain and write-through)
  k_lerp (out of place)                 test_resident[one]
  k_lerp_unaligned                      test_average_unaligned
  k_lerp_tracked, k_distance_finish     test_average_tracked (bf16, f32)
  k_lerp_mixed (plain and DUAL)         test_average_mixed
  k_lerp_pair                           test_resident[mutual-pair]
  k_lerp_group                          test_resident[U3]
  k_distance, k_distance_unaligned      test_distance (bf16, f32; aligned and one element on)
  k_distance_mixed                      test_distance_mixed
  k_param_distance, _finish             test_param_distance
  k_peer_finite, k_peer_finite_unaligned  test_check_finite (bf16, f32, f16; aligned and one element on)
  k_peer_finite_mixed                   test_check_finite_mixed
  k_publish<true>, k_publish<false>     test_publish (aligned, 2 bytes off)
  k_copy_payload                        test_relocation
  k_pull                                test_pull (max_blocks 512)
  k_guard_publish, _bytes               test_reuse_guard (aligned, 4 bytes off)
  k_window_roll                         test_window_guard
  k_relay_phase1, k_relay_phase2        test_relay (form "gather"; world 2, one process per rank)
  k_lerp_relay (StripeSrc)              test_relay (form "fused")
Left out: k_factor, k_publish_header, k_store_u64 and the fence kernels (k_acquire_system,
k_release_system) touch no payload; k_stream_mix is the benchmark's.  k_lerp_batch runs beyond 2^32
bytes in tests/test_gpu_batch.py::test_average_many_beyond_4gib_offsets only.

Wall time on one MI355X, same run and machine: tests/test_gpu_batch.py::
test_average_many_beyond_4gib_offsets 0.25 s; the slowest test here, test_reuse_guard[byte-form], 6.03 s.
The issue's bar of three times the parent's time is NOT met: in every run two to four tests take 2 to 6 s
where they otherwise take 0.03 to 0.25 s (test_relay, which starts two processes, 2.4 to 4.2 s).
test_wall_times_are_reported prints every in-process test's wall time and its share spent allocating and
freeing device memory; that share explains some of them (test_resident[U3]: 5.73 of 5.86 s) and not others
(test_reuse_guard[byte-form]: 0.01 of 6.03 s, whose byte-wise chunk copy runs in one thread; 0.17 s in
another run), whose cause is not known.
"""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

from dpwa_amd import _lib
from dpwa_amd.devview import device_tensor
from dpwa_amd.learner import Learner
from oracle import policy as opolicy
from tests import big_ref as ref
from tests import finite_ref
from tests import forms_ref as fref
from tests import moves_ref as mref
from tests.mixed_ref import CODE, NUMPY, SIZE, TORCH
from tests.test_gpu_kernels import coef_block, header_bytes, ptr, stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
BROKEN = []
SPENT = {"allocating": 0.0}        # seconds of the running test that went to allocating and freeing device memory
WALL = {}                          # test -> (wall seconds, of which allocating and freeing)
INT = {2: torch.int16, 4: torch.int32}
OFF = _lib.SLOT_PAYLOAD_OFFSET
CFG = _lib.Interp(_lib.INTERP_CONSTANT, 0, ref.FACTOR, 0.0)
MY_CLOCK, PEER_CLOCK, LOSS, PEER_LOSS = 3.0, 7.0, 0.5, 0.25


def latched(fn):
    @functools.wraps(fn)
    def run(*args, **kwargs):
        if BROKEN:
            pytest.fail("not run: an earlier test of this module met a HIP error (%s)" % BROKEN[0])
        began, SPENT["allocating"] = time.monotonic(), 0.0
        try:
            fn(*args, **kwargs)
            torch.cuda.synchronize()
        except _lib.DpwaError as e:
            if e.code == _lib.ERR_HIP:
                BROKEN.append(str(e))
            raise
        except RuntimeError as e:          # torch's HIP errors
            BROKEN.append("%s: %s" % (type(e).__name__, e))
            raise
        finally:
            if not BROKEN:
                with allocating():
                    torch.cuda.empty_cache()
            WALL[(fn.__name__,) + args + tuple(kwargs.values())] = (time.monotonic() - began, SPENT["allocating"])
    return run


class allocating:
    """Adds the block's wall time, up to the device's having finished it, to SPENT."""

    def __enter__(self):
        self.began = time.monotonic()

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        SPENT["allocating"] += time.monotonic() - self.began
        return False


# ---------------------------------------------------------------- device buffers
def signed(dtype, bits):
    return int(np.array([bits], dtype=NUMPY[dtype]).view({2: np.int16, 4: np.int32}[SIZE[dtype]])[0])


class Buffer:
    """A payload's bytes on the device between guard bands: an Operand's constants and windows, or the
    bands' fill (a destination).  slot: the payload lies DPWA_SLOT_PAYLOAD_OFFSET behind a dpwa_header
    (a peer's snapshot slot); offset: bytes behind a 16-byte boundary."""

    def __init__(self, pl, op=None, offset=0, slot=None):
        assert not (slot and offset)
        self.pl, self.op = pl, op
        with allocating():
            raw, self.check = fref.guarded((OFF if slot else 0) + pl.nbytes, offset)
        self.raw = raw
        self.bytes = raw[OFF:] if slot else raw
        if slot:
            raw[:256].copy_(torch.frombuffer(bytearray(header_bytes(*slot)), dtype=torch.uint8))
        if op is not None:
            fill(self.bytes, pl, op)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.bytes.data_ptr())

    @property
    def slot_ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr())


def fill(view, pl, op):
    for d, a, b in pl.segs:
        view[a:b].view(INT[SIZE[d]]).fill_(signed(d, op.const[d]))
    for (lo, hi), w in zip(pl.wins, op.data):
        view[lo:hi].copy_(torch.from_numpy(w))


def outcome(view, pl, const):
    """big_ref.Outcome of device bytes: the windows copied back, and the constant-region elements that
    differ from const[dtype], listed on the device chunk by chunk."""
    wins = [(lo, hi, view[lo:hi].cpu().numpy()) for lo, hi in pl.wins]
    lows = np.array([w[0] for w in pl.wins], dtype=np.int64)
    highs = np.array([w[1] for w in pl.wins], dtype=np.int64)
    stray, first = 0, []
    for d, a, b in pl.segs:
        s = SIZE[d]
        elems = view[a:b].view(INT[s])
        want = signed(d, const[d])
        for c in range(0, elems.numel(), ref.CHUNK):
            differ = elems[c:c + ref.CHUNK] != want
            count = int(differ.sum())
            if count > (1 << 20):                          # far more than the windows hold
                stray += count
                first = first or [("chunk at element %d" % c, count)]
                continue
            at = a + (torch.nonzero(differ).reshape(-1).cpu().numpy() + c) * s
            k = np.searchsorted(lows, at, side="right") - 1
            out = at[~((k >= 0) & (at < highs[np.maximum(k, 0)]))]
            stray += out.size
            first = first or out[:5].tolist()
            del differ
    return ref.Outcome(windows=wins, stray=stray), first


def expect(buf, want, what, exact_bytes=False, const=None):
    """The destination `buf` against the model's Outcome, and its guard bands."""
    got, first = outcome(buf.bytes, buf.pl, const)
    failed = ref.failures(buf.pl, got, want, exact_bytes)
    detail = []
    if "windows" in failed:
        for (lo, hi, g), (_, _, w) in zip(got.windows, want.windows):
            bad = np.flatnonzero(g != w)
            if bad.size:
                detail.append((lo, "%d bytes differ, the first at payload byte %d" % (bad.size, lo + int(bad[0])),
                               g[bad[:8]].tolist(), w[bad[:8]].tolist()))
    assert not failed, (what, failed, "stray elements: %d, first at bytes %s" % (got.stray, first), detail)
    buf.check(what)


def unchanged(buf, what):
    """A source still holds its operand: windows byte for byte, every other element the constant."""
    pl, op = buf.pl, buf.op
    want = ref.Outcome(windows=[(lo, hi, w) for (lo, hi), w in zip(pl.wins, op.data)], stray=0)
    expect(buf, want, (what, "a source changed"), exact_bytes=True, const=op.const)


def clock_block(clock=MY_CLOCK):
    return torch.tensor([clock, -1.0], dtype=torch.float64, device=DEV)


def new_clock():
    f, c = opolicy.factor_and_clock("constant", ref.FACTOR, 0.0, MY_CLOCK, PEER_CLOCK, LOSS, PEER_LOSS)
    assert f == ref.FACTOR
    return c


def c_layout(pl):
    lay = _lib.Layout()
    lay.count = len(pl.segs)
    for i, (d, a, b) in enumerate(pl.segs):
        lay.seg[i] = _lib.Segment(CODE[d], 0, a, b - a)
    return lay


def workspace():
    ws = ctypes.c_int64()
    _lib.call("dpwa_distance_workspace", ctypes.byref(ws))
    return torch.zeros(ws.value, dtype=torch.uint8, device=DEV)


def read_distance(rec, n, clock):
    d2, n2, c = np.frombuffer(rec.cpu().numpy().tobytes()[:24], dtype=np.float64).tolist()
    count = int(np.frombuffer(rec.cpu().numpy().tobytes()[24:32], dtype=np.int64)[0])
    assert (c, count) == (clock, n), (c, count)
    return d2, n2


# ---------------------------------------------------------------- averaging
@pytest.mark.parametrize("coef", ["host", "device"])
@pytest.mark.parametrize("dtype", ["bf16", "f32", "f16"])
@latched
def test_lerp(dtype, coef):
    """dpwa_lerp_*_host and dpwa_lerp_* (k_lerp with the coefficients from the host and from a device
    block), in place."""
    pl = ref.single(dtype)
    P, Q = ref.operands(pl, "hard")
    p, q = Buffer(pl, P), Buffer(pl, Q)
    n = ref.N[dtype]
    if coef == "host":
        _lib.call("dpwa_lerp_%s_host" % dtype, p.ptr, q.ptr, n, ref.FACTOR, stream())
    else:
        block = coef_block(ref.FACTOR)
        _lib.call("dpwa_lerp_%s" % dtype, p.ptr, q.ptr, n, ptr(block), stream())
    torch.cuda.synchronize()
    want = ref.average(pl, P, Q, ref.right_cover(pl))
    expect(p, want["param"], ("lerp", dtype, coef), const=ref.lerp_const(P, Q))
    unchanged(q, ("lerp", dtype, coef))


def fused(dtype, pl, family, through, offset=0, tracked=False):
    """One dpwa_average (or _tracked, or _mixed for a segmented payload) launch and its checks."""
    what = ("average", dtype or "mixed", family, "write-through" if through else "plain", offset, tracked)
    P, Q = ref.operands(pl, family)
    p, q = Buffer(pl, P, offset=offset), Buffer(pl, Q, slot=(PEER_CLOCK, PEER_LOSS))
    snap = Buffer(pl, offset=offset) if through else None
    clock, coef = clock_block(), torch.zeros(32, dtype=torch.uint8, device=DEV)
    snap_ptr = snap.ptr if through else None
    if tracked:
        ws, rec = workspace(), torch.full((32,), 0xa5, dtype=torch.uint8, device=DEV)
        _lib.call("dpwa_average_tracked", CODE[dtype], p.ptr, q.slot_ptr, ref.N[dtype], ctypes.byref(CFG), ptr(clock), LOSS,
                  ptr(coef), snap_ptr, ptr(ws), ptr(rec), stream(), None, None)
    elif dtype is None:
        lay = c_layout(pl)
        _lib.call("dpwa_average_mixed", ctypes.byref(lay), p.ptr, q.slot_ptr, ctypes.byref(CFG), ptr(clock), LOSS, ptr(coef),
                  snap_ptr, stream(), None, None)
    else:
        _lib.call("dpwa_average", CODE[dtype], p.ptr, q.slot_ptr, ref.N[dtype], ctypes.byref(CFG), ptr(clock), LOSS, ptr(coef),
                  snap_ptr, stream(), None, None)
    torch.cuda.synchronize()
    want = ref.average(pl, P, Q, ref.right_cover(pl), through=through)
    const = ref.lerp_const(P, Q)
    expect(p, want["param"], (what, "parameters"), const=const)
    if through:
        expect(snap, want["snap"], (what, "snapshot"), const=const)
    unchanged(q, what)
    q.check(what)
    assert clock.cpu().tolist() == [MY_CLOCK, new_clock()], (what, clock.cpu().tolist())
    if tracked:
        got = read_distance(rec, ref.N[dtype], new_clock())
        exact = ref.sums(pl, P, Q, ref.right_cover(pl))
        assert got == exact, (what, got, exact)
        assert not bool(ws.any()), (what, "the accumulators are left zero")


@pytest.mark.parametrize("through", [False, True], ids=["plain", "write-through"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@latched
def test_average(dtype, through):
    """dpwa_average: k_lerp with the fused factor, in place and with the write-through snapshot."""
    fused(dtype, ref.single(dtype), "hard", through)


@latched
def test_average_unaligned():
    """The element-wise kernel (k_lerp_unaligned): parameters and snapshot one element behind a 16-byte
    boundary, so the element index passes 2^31 in its grid-stride loop."""
    fused("bf16", ref.single("bf16"), "hard", True, offset=SIZE["bf16"])


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@latched
def test_average_tracked(dtype):
    """dpwa_average_tracked on the exact family: the averaged parameters, the snapshot, and the record's
    two sums equal to the closed form."""
    fused(dtype, ref.single(dtype), "exact", True, tracked=True)


@pytest.mark.parametrize("through", [False, True], ids=["plain", "write-through"])
@latched
def test_average_mixed(through):
    """dpwa_average_mixed (k_lerp_mixed): the second and third segments begin beyond byte 2^32."""
    fused(None, ref.mixed(), "hard", through)


@pytest.mark.parametrize("name", ["one", "mutual-pair", "U3"])
@latched
def test_resident(name):
    """dpwa_average_many_resident: one entry (k_lerp out of place), the mutual pair (k_lerp_pair) and a
    cycle of three (k_lerp_group); every learner's parameters lie in a slot and are read only."""
    picks = fref.RESIDENT[name]
    pl = ref.single("bf16")
    ops = [ref.learner(pl, i) for i in range(1 + max(max(p) for p in picks))]
    clocks = [2.0 + i for i in range(len(ops))]
    slots = [Buffer(pl, op, slot=(clocks[i], 0.25 + i)) for i, op in enumerate(ops)]
    snaps = [Buffer(pl) for _ in picks]
    blocks = [(clock_block(clocks[a]), torch.zeros(32, dtype=torch.uint8, device=DEV)) for a, _ in picks]
    descs = (_lib.AverageDesc * len(picks))()
    for j, (a, b) in enumerate(picks):
        descs[j] = _lib.AverageDesc(slots[a].ptr.value, slots[b].slot_ptr.value, ref.N["bf16"], blocks[j][0].data_ptr(), LOSS,
                                    blocks[j][1].data_ptr(), snaps[j].ptr.value)
    _lib.call("dpwa_average_many_resident", _lib.BF16, descs, len(picks), ctypes.byref(CFG), stream(), None, None)
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(picks):
        what = ("resident", name, "entry %d" % j)
        want = ref.average(pl, ops[a], ops[b], ref.right_cover(pl), resident=True)
        expect(snaps[j], want["snap"], what, const=ref.lerp_const(ops[a], ops[b]))
        _, c = opolicy.factor_and_clock("constant", ref.FACTOR, 0.0, clocks[a], clocks[b], LOSS, 0.25 + b)
        assert blocks[j][0].cpu().tolist() == [clocks[a], c], what
    for i, s in enumerate(slots):
        unchanged(s, ("resident", name, "learner %d" % i))


# ---------------------------------------------------------------- sums
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one-element-on"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@latched
def test_distance(dtype, offset):
    """dpwa_measure_distance (k_distance, k_distance_unaligned, then the finishing step) on the exact
    family: both sums equal to the closed form."""
    pl = ref.single(dtype)
    P, Q = ref.operands(pl, "exact")
    p, q = Buffer(pl, P, offset=offset * SIZE[dtype]), Buffer(pl, Q, offset=offset * SIZE[dtype])
    ws, rec = workspace(), torch.full((32,), 0xa5, dtype=torch.uint8, device=DEV)
    _lib.call("dpwa_measure_distance", CODE[dtype], p.ptr, q.ptr, ref.N[dtype], ptr(ws), ptr(rec), stream())
    torch.cuda.synchronize()
    got, exact = read_distance(rec, ref.N[dtype], 0.0), ref.sums(pl, P, Q, ref.right_cover(pl))
    assert got == exact, (dtype, offset, got, exact)
    assert not bool(ws.any())
    unchanged(p, ("distance", dtype, offset))
    unchanged(q, ("distance", dtype, offset))


@latched
def test_distance_mixed():
    """dpwa_measure_distance_mixed (k_distance_mixed)."""
    pl = ref.mixed()
    P, Q = ref.operands(pl, "exact")
    p, q = Buffer(pl, P), Buffer(pl, Q)
    ws, rec = workspace(), torch.full((32,), 0xa5, dtype=torch.uint8, device=DEV)
    lay = c_layout(pl)
    _lib.call("dpwa_measure_distance_mixed", ctypes.byref(lay), p.ptr, q.ptr, ptr(ws), ptr(rec), stream())
    torch.cuda.synchronize()
    slots = sum((b - a) // SIZE[d] for d, a, b in pl.segs)
    got, exact = read_distance(rec, slots, 0.0), ref.sums(pl, P, Q, ref.right_cover(pl))
    assert got == exact, (got, exact)
    assert not bool(ws.any())
    unchanged(p, "distance mixed")
    unchanged(q, "distance mixed")


@latched
def test_param_distance():
    """dpwa_measure_param_distance (k_param_distance, k_param_distance_finish) over big_ref.TENSORS: the
    pair of every tensor equal to the closed form over its own bytes, the gaps in no sum."""
    pl = ref.tabled()
    P, Q = ref.operands(pl, "exact")
    p, q = Buffer(pl, P), Buffer(pl, Q)
    count = len(ref.TENSORS)
    ranges = (_lib.ParamRange * count)()
    for i, (a, b) in enumerate(ref.TENSORS):
        ranges[i] = _lib.ParamRange(a, b - a, _lib.BF16, 0)
    _lib.call("dpwa_param_ranges_check", ranges, count, _lib.BF16, ref.N["bf16"], None)
    z = _lib.ParamSizes()
    _lib.call("dpwa_param_distance_sizes", ranges, count, ctypes.byref(z))
    table = torch.zeros(z.table_bytes, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(z.workspace_bytes, dtype=torch.uint8, device=DEV)
    rec = torch.full((z.record_bytes,), 0xa5, dtype=torch.uint8, device=DEV)
    _lib.call("dpwa_param_distance_table", ranges, count, ptr(table))
    _lib.call("dpwa_measure_param_distance", ptr(table), count, p.ptr, q.ptr, pl.nbytes, ptr(ws), ptr(rec), stream(), None,
              None)
    torch.cuda.synchronize()
    host = rec.cpu().numpy().tobytes()
    assert np.frombuffer(host[:8], dtype=np.float64)[0] == 0.0 and np.frombuffer(host[8:16], dtype=np.int64)[0] == count
    got = [tuple(r) for r in np.frombuffer(host[16:16 + 16 * count], dtype=np.float64).reshape(-1, 2).tolist()]
    exact = ref.sums(pl, P, Q, ref.right_cover(pl), ref.table_members(pl, ref.TENSORS))
    assert got == exact, (got, exact)
    assert not bool(ws.any())
    unchanged(p, "param distance")
    unchanged(q, "param distance")


# ---------------------------------------------------------------- finite check
def finite_passes(pl, dtype, offset):
    """The finite peer (no veto), then one finite_ref.BAD pattern at a time at each of
    big_ref.finite_positions (a veto each, with a fresh stamp); each pass is one launch."""
    Q = ref.operands(pl, "finite")[1]
    q = Buffer(pl, Q, offset=offset)
    veto = torch.zeros(1, dtype=torch.int32, device=DEV)
    lay, last = c_layout(pl), 0
    for stamp, (name, peer) in enumerate(ref.finite_plants(pl, Q), 1):
        at = None
        if len(name) == 2:
            at = ref.finite_positions(pl)[name[0]]
            d = pl.split(at, at + 1)[0][0]
            keep = q.bytes[at:at + SIZE[d]].clone()
            q.bytes[at:at + SIZE[d]].copy_(torch.from_numpy(np.array([finite_ref.BAD[d][name[1]]], dtype=NUMPY[d]).view(np.uint8)))
        if dtype is None:
            _lib.call("dpwa_check_finite_mixed", ctypes.byref(lay), q.ptr, ptr(veto), stamp, stream(), None, None)
        else:
            _lib.call("dpwa_check_finite", CODE[dtype], q.ptr, ref.N[dtype], ptr(veto), stamp, stream(), None, None)
        got = int(veto.item())
        want = ref.veto(pl, peer, ref.right_cover(pl))
        assert want == (at is not None)
        last = stamp if want else last        # the word keeps the stamp of the last pass that vetoed
        assert got == last, (dtype, offset, name, "veto word %d at stamp %d, expected %d" % (got, stamp, last))
        if at is not None:
            q.bytes[at:at + SIZE[d]].copy_(keep)
    unchanged(q, ("finite", dtype, offset))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one-element-on"])
@pytest.mark.parametrize("dtype", ["bf16", "f32", "f16"])
@latched
def test_check_finite(dtype, offset):
    """dpwa_check_finite: k_peer_finite and k_peer_finite_unaligned."""
    finite_passes(ref.single(dtype), dtype, offset * SIZE[dtype])


@latched
def test_check_finite_mixed():
    """dpwa_check_finite_mixed (k_peer_finite_mixed): among the positions, the first element of the second
    and of the third segment."""
    finite_passes(ref.mixed(), None, 0)


# ---------------------------------------------------------------- byte movers
class Node:
    """A DPWA_BF16 learner of big_ref.N elements that is its own peer 0 (a fetch pulls its own
    snapshot into its staging buffer)."""

    def __init__(self, self_peer=True):
        self.pl = ref.single("bf16")
        with allocating():
            self.lr = Learner(DEV, ref.N["bf16"], TORCH["bf16"], CFG)
        self.h = self.lr.handle
        sh, sp = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.call("dpwa_learner_pointers", self.h, None, None, ctypes.byref(sh), ctypes.byref(sp))
        self.staging = device_tensor(sp.value, self.pl.nbytes, torch.uint8, DEV)
        if self_peer:
            _lib.call("dpwa_learner_attach_local", self.h, 0, self.h)

    def counter(self, name):
        h = ctypes.c_uint32()
        _lib.call(name, self.h, ctypes.byref(h))
        return h.value

    def resident(self):
        p, slot = ctypes.c_void_p(), ctypes.c_int()
        _lib.call("dpwa_learner_resident_params", self.h, ctypes.byref(p), ctypes.byref(slot))
        return p.value, slot.value

    def close(self):
        with allocating():
            self.lr.close()

    def header(self):
        out, hdr, v = np.zeros(4096, dtype=np.uint8), ctypes.create_string_buffer(256), ctypes.c_uint64()
        _lib.call("dpwa_learner_read_snapshot", self.h, hdr, ctypes.c_void_p(out.ctypes.data), out.nbytes, ctypes.byref(v))
        return _lib.Header.from_buffer_copy(hdr.raw), out, v.value

    def pulled(self, version, mode, max_blocks, S, what):
        """Pulls the snapshot of `version` into the staging buffer and compares it with the operand S."""
        _lib.call("dpwa_learner_set_pull", self.h, mode, max_blocks)
        self.staging.fill_(ref.FILL)
        _lib.call("dpwa_learner_fetch", self.h, 0, version, 0, stream())
        _lib.call("dpwa_learner_wait_fetch", self.h, stream())
        torch.cuda.synchronize()
        got, first = outcome(self.staging, self.pl, S.const)
        failed = ref.failures(self.pl, got, ref.moved(self.pl, S, ref.right_cover(self.pl)), exact_bytes=True)
        assert not failed, (what, failed, got.stray, first)
        _lib.call("dpwa_learner_cancel", self.h)


@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "2-bytes-off"])
@latched
def test_publish(offset):
    """dpwa_learner_publish from an aligned buffer (k_publish<true>) and from one 2 bytes off
    (k_publish<false>): the header read back carries n, and the snapshot, pulled by the copy engine, is
    the source byte for byte."""
    me = Node()
    try:
        S = ref.operands(me.pl, "hard")[0]
        src = Buffer(me.pl, S, offset=offset)
        _lib.call("dpwa_learner_publish", me.h, src.ptr, 1.25, None, stream())
        torch.cuda.synchronize()
        h, head, v = me.header()
        assert (v, h.version, h.n, h.dtype, h.clock, h.loss) == (1, 1, ref.N["bf16"], _lib.BF16, 1.0, 1.25)
        assert np.array_equal(head, S.bytes(0, 4096))
        me.pulled(1, _lib.PULL_COPY_ENGINE, 512, S, ("publish", offset))
        unchanged(src, ("publish", offset))
    finally:
        me.close()


@latched
def test_pull():
    """A local fetch with the pull kernel (k_pull) at max_blocks 512."""
    me = Node()
    try:
        S = ref.operands(me.pl, "hard")[1]
        src = Buffer(me.pl, S)
        _lib.call("dpwa_learner_publish", me.h, src.ptr, 1.0, None, stream())
        me.pulled(1, _lib.PULL_KERNEL, 512, S, "pull")
        unchanged(src, "pull")
    finally:
        me.close()


@latched
def test_relocation():
    """A resident learner that publishes twice with no average in between moves its parameters into the
    other slot with k_copy_payload, and so does dpwa_learner_relocate: both slots hold the initial bytes
    each time."""
    me = Node()
    try:
        pl = me.pl
        S = ref.operands(pl, "hard")[0]
        src = Buffer(pl, S)
        _lib.call("dpwa_learner_set_resident", me.h, src.ptr, stream())

        def where():
            p, slot = ctypes.c_void_p(), ctypes.c_int()
            _lib.call("dpwa_learner_resident_params", me.h, ctypes.byref(p), ctypes.byref(slot))
            return p.value, slot.value

        p0, s0 = where()
        _lib.call("dpwa_learner_publish", me.h, ctypes.c_void_p(p0), 1.0, None, stream())     # header only
        _lib.call("dpwa_learner_publish", me.h, ctypes.c_void_p(p0), 1.0, None, stream())     # slot 0 -> slot 1
        p1, s1 = where()
        assert (s0, s1) == (0, 1) and p1 != p0
        torch.cuda.synchronize()
        want = ref.moved(pl, S, ref.right_cover(pl))
        views = [device_tensor(p, pl.nbytes, torch.uint8, DEV) for p in (p0, p1)]
        for i, v in enumerate(views):
            got, first = outcome(v, pl, S.const)
            failed = ref.failures(pl, got, want, exact_bytes=True)
            assert not failed, ("relocation by publish", "slot %d" % i, failed, got.stray, first)
        views[0].fill_(ref.FILL)                                                              # the slot left behind
        _lib.call("dpwa_learner_relocate", me.h, stream())                                    # slot 1 -> slot 0
        assert where() == (p0, 0)
        _lib.call("dpwa_learner_relocate", me.h, stream())                                    # already there: nothing moves
        torch.cuda.synchronize()
        for i, v in enumerate(views):
            got, first = outcome(v, pl, S.const)
            failed = ref.failures(pl, got, want, exact_bytes=True)
            assert not failed, ("relocation", "slot %d" % i, failed, got.stray, first)
        h, _, ver = me.header()
        assert (ver, h.n) == (2, ref.N["bf16"])
        unchanged(src, "relocation")
    finally:
        me.close()


def differing(a, b):
    """The byte offsets at which two device buffers differ (chunk by chunk, an integer != and nonzero)."""
    out = []
    for c in range(0, a.numel(), ref.CHUNK):
        d = a[c:c + ref.CHUNK] != b[c:c + ref.CHUNK]
        count = int(d.sum())
        assert count < (1 << 16), "%d bytes differ in the chunk at byte %d" % (count, c)
        out += (torch.nonzero(d).reshape(-1).cpu().numpy() + c).tolist()
    return out


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "byte-form"])
@latched
def test_reuse_guard(offset):
    """A reusing publish with the guard on (k_guard_publish; 4 bytes off the alignment:
    k_guard_publish_bytes) after writes around the chunks holding words 2^27 and 2^28 -- the sampled
    word, both end words, and the words just outside -- and to the tail: the snapshot takes exactly the
    written bytes big_ref.guard_model says (two whole chunks, one of them beyond byte 2^32, the tail and,
    in the aligned form, the last word; the byte form copies a dirty chunk in one thread and gets the two
    chunks only) and dpwa_learner_reuse_guard_hits grows by one."""
    me = Node()
    try:
        pl, gen = me.pl, 2
        flat = Buffer(pl, ref.operands(pl, "hard")[0], offset=offset)
        _lib.call("dpwa_learner_set_reuse_guard", me.h, 1)
        _lib.call("dpwa_learner_publish", me.h, flat.ptr, 1.0, None, stream())
        assert me.counter("dpwa_learner_reuse_guard_hits") == 0
        _lib.call("dpwa_learner_fetch", me.h, 0, 1, 0, stream())
        _lib.call("dpwa_learner_average_through", me.h, flat.ptr, 1.0, None, stream())
        torch.cuda.synchronize()
        with allocating():
            before = flat.bytes.clone()                   # what the average wrote through
        at = mref.write_offsets(ref.guard_case(pl.nbytes, gen, two_chunks_only=bool(offset)), pl.nbytes, gen)
        dev_at = torch.from_numpy(at).to(DEV)
        flat.bytes[dev_at] = flat.bytes[dev_at] ^ mref.FLIP
        assert differing(flat.bytes, before) == at.tolist()
        _lib.call("dpwa_learner_publish_reuse", me.h, flat.ptr, 0.5, None, stream())
        torch.cuda.synchronize()
        taken, hit = ref.guard_model(pl.nbytes, gen, at)
        assert me.counter("dpwa_learner_reuse_guard_hits") == int(hit) == 1
        h, _, v = me.header()
        assert (v, h.n) == (gen, ref.N["bf16"])
        _lib.call("dpwa_learner_set_pull", me.h, _lib.PULL_COPY_ENGINE, 512)
        me.staging.fill_(ref.FILL)
        _lib.call("dpwa_learner_fetch", me.h, 0, gen, 0, stream())
        _lib.call("dpwa_learner_wait_fetch", me.h, stream())
        torch.cuda.synchronize()
        got = differing(me.staging, before)
        assert got == taken, ("reuse guard", offset, "the snapshot took %d written bytes, the model %d" % (len(got), len(taken)),
                              sorted(set(got) ^ set(taken))[:8])
        where = torch.tensor(taken, dtype=torch.int64, device=DEV)
        assert torch.equal(me.staging[where], flat.bytes[where])
        _lib.call("dpwa_learner_cancel", me.h)
        assert differing(flat.bytes, before) == at.tolist(), "the publish changed the parameters"
        flat.check(("reuse guard", offset))
    finally:
        me.close()


@latched
def test_window_guard():
    """k_window_roll: a resident learner with the guard on publishes three times; in each window
    big_ref.window_cases' words are written into the published payload: dpwa_learner_window_hits grows iff
    big_ref.window_model says so (unsampled words: no; the sampled word of the chunk beyond byte 2^32:
    yes; the tail: yes), and the publish that first sees a count is refused with DPWA_ERR_STATE."""
    me, peer = Node(self_peer=False), Node(self_peer=False)
    try:
        pl = me.pl
        P, Q = ref.operands(pl, "hard")
        _lib.call("dpwa_learner_attach_local", me.h, 1, peer.h)
        src = Buffer(pl, Q)
        _lib.call("dpwa_learner_publish", peer.h, src.ptr, 0.75, None, stream())
        first = Buffer(pl, P)
        _lib.call("dpwa_learner_set_reuse_guard", me.h, 1)
        _lib.call("dpwa_learner_set_resident", me.h, first.ptr, stream())
        torch.cuda.synchronize()
        del src, first
        where = me.resident()[0]
        _lib.call("dpwa_learner_publish", me.h, ctypes.c_void_p(where), 1.0, None, stream())
        hits, pending, verdicts = me.counter("dpwa_learner_window_hits"), False, []
        assert hits == 0
        for gen, words in ref.window_cases(pl.nbytes):
            what = ("window guard", "generation %d" % gen)
            assert me.header()[2] == gen
            view = device_tensor(where, pl.nbytes, torch.uint8, DEV)
            at = mref.write_offsets(words, pl.nbytes, gen)
            dev_at = torch.from_numpy(at).to(DEV)
            view[dev_at] = view[dev_at] ^ mref.FLIP          # a write while peers can read it
            _lib.call("dpwa_learner_fetch", me.h, 1, 1, 0, stream())
            _lib.call("dpwa_learner_average", me.h, ctypes.c_void_p(where), 1.0, None, stream())
            moved = me.resident()[0]
            assert moved != where
            if pending:                                     # the last window's count, seen first here
                with pytest.raises(_lib.DpwaError) as err:
                    _lib.call("dpwa_learner_publish", me.h, ctypes.c_void_p(moved), 1.0, None, stream())
                assert err.value.code == _lib.ERR_STATE, (what, err.value)
            _lib.call("dpwa_learner_publish", me.h, ctypes.c_void_p(moved), 1.0, None, stream())
            new_hits = me.counter("dpwa_learner_window_hits")
            want = ref.window_model(pl.nbytes, gen, at)
            assert new_hits - hits == int(want), (what, "hits grew by %d, the model says %d" % (new_hits - hits, want))
            verdicts.append(want)
            hits, pending, where = new_hits, want, moved
        assert verdicts == [False, True, True]
    finally:
        me.close()
        peer.close()


# ---------------------------------------------------------------- relay
def test_relay():
    """World 2, one process per rank (tests/relay_worker.py big_rank_main), bf16, picks (1, 0), one round
    of the gathered form (k_relay_phase1, k_relay_phase2, then k_lerp on the staged payload) and one of the
    fused form (k_relay_phase1, k_lerp_relay): the stripe border lies beyond byte 2^31 and has a window of
    its own, the second stripe crosses byte 2^32."""
    if BROKEN:
        pytest.fail("not run: an earlier test of this module met a HIP error (%s)" % BROKEN[0])
    from tests import relay_worker
    from tests.test_gpu_relay import first_failure, run_world
    torch.cuda.empty_cache()
    reports = run_world(ref.RELAY_WORLD, target=relay_worker.big_rank_main, only=ref.RELAY_FORMS)
    assert first_failure(reports) is None, first_failure(reports)
    assert reports == {r: ("ok", len(ref.RELAY_FORMS)) for r in range(ref.RELAY_WORLD)}, reports


def test_wall_times_are_reported():
    """Prints, for every in-process test of this module that ran before, its wall time and how much of it
    went to allocating and freeing device memory (the buffers' torch.full, a learner's slots, empty_cache)."""
    for name, (wall, alloc) in sorted(WALL.items(), key=lambda kv: -kv[1][0]):
        print("%-50s %6.2f s, of which allocating and freeing %6.2f s" % (" ".join(str(x) for x in name), wall, alloc))
