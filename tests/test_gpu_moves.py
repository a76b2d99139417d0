"""The kernels that only move bytes -- k_publish (vector and byte forms), k_publish_header,
k_copy_payload, k_pull, k_guard_publish, k_guard_publish_bytes, k_window_roll -- at the sizes where
their loops and bounds change, against the host model of tests/moves_ref.py.  Everything goes through
the public C ABI (dpwa_amd._lib.call, dpwa_amd.learner.Learner) in this process, peers attached with
attach_local.  The bar is byte equality.

Operands are the hard bit patterns of forms_ref.operands for float32, bfloat16 and float16 (and, for
the payload sizes no element type divides, a DPWA_MIXED learner without a layout, which publishes and
serves plain bytes).  Buffers the test owns lie between guard bands; every source is compared with
its host copy afterwards.  tests/test_moves_host.py shows, without a GPU, that the sizes, generations
and write sets used here tell the model from every wrong kernel restated there."""
import ctypes
import time

import numpy as np
import pytest
import torch

from dpwa_amd import _lib
from dpwa_amd.devview import device_tensor
from dpwa_amd.learner import Learner
from oracle import policy as opolicy
from tests import forms_ref as fref
from tests import moves_ref as ref
from tests.forms_ref import CODE, SIZE, TORCH

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = fref.DTYPES
KINDS = ("bytes",) + DTYPES                       # "bytes": DPWA_MIXED without a layout, one byte per element
BAND = fref.GUARD
SENTINEL = fref.GUARD_BYTE


def interp(value=0.3):
    return _lib.Interp(_lib.INTERP_CONSTANT, 0, value, 0.0)


def stream():
    return _lib.stream_handle(None)


def host(t):
    """The bytes of a device tensor."""
    return t.contiguous().view(torch.uint8).cpu().numpy()


def operand_bytes(kind, nbytes, which=0, seed=1):
    """`nbytes` of forms_ref.operands' hard bit patterns (which: 0 the parameters, 1 the peer)."""
    dtype = "f32" if kind == "bytes" else kind
    n = -(-nbytes // SIZE[dtype])
    bits = fref.operands(dtype, n, seed) if nbytes <= (1 << 24) else fref.sample(dtype, n, seed)    # (not kept)
    return np.array(bits[which]).view(np.uint8)[:nbytes]


def banded(data, offset=0, fill=SENTINEL):
    """(payload, check): a uint8 device tensor holding `data` that begins `offset` bytes behind a
    16-byte boundary, with BAND bytes of `fill` on each side (forms_ref.guarded with a choice of
    fill); check() asserts the bands still hold it."""
    nbytes = len(data)
    whole = torch.full((BAND + 16 + offset + nbytes + BAND,), fill, dtype=torch.uint8, device=DEV)
    start = BAND + (-(whole.data_ptr() + BAND)) % 16 + offset
    payload = whole[start:start + nbytes]
    assert (payload.data_ptr() - offset) % 16 == 0
    payload.copy_(torch.from_numpy(np.array(data, dtype=np.uint8)))

    def check(what=None):
        for name, band in (("before", whole[:start]), ("behind", whole[start + nbytes:])):
            bad = torch.nonzero(band != fill).reshape(-1)
            assert bad.numel() == 0, ("%d bytes written %s the buffer, the first at band offset %d"
                                      % (bad.numel(), name, int(bad[0])), what)
    return payload, check


class Node:
    """One learner: made by dpwa_amd.learner.Learner for an element type, by dpwa_learner_create for
    the byte kind; every other call goes straight to the C ABI."""

    def __init__(self, kind, nbytes, value=0.3):
        self.kind, self.nbytes = kind, nbytes
        self.cfg = interp(value)
        if kind == "bytes":
            self.lr, self.n, self.code = None, nbytes, _lib.MIXED
            self.h = ctypes.c_void_p()
            _lib.call("dpwa_learner_create", ctypes.byref(self.h), 0, nbytes, _lib.MIXED, ctypes.byref(self.cfg))
        else:
            assert nbytes % SIZE[kind] == 0
            self.n, self.code = nbytes // SIZE[kind], CODE[kind]
            self.lr = Learner(DEV, self.n, TORCH[kind], self.cfg)
            self.h = self.lr.handle
        sh, sp = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.call("dpwa_learner_pointers", self.h, None, None, ctypes.byref(sh), ctypes.byref(sp))
        self.staging_header, self.staging_payload = sh.value, sp.value
        self.loss_dtype = _lib.F64
        self.keep = None

    def close(self):
        if self.lr is not None:
            self.lr.close()
        elif self.h:
            _lib.call("dpwa_learner_destroy", self.h)
        self.h = None

    def _loss(self, loss):
        """(host double, device pointer): a device scalar is read in place, float32 or float64."""
        if isinstance(loss, torch.Tensor):
            want = _lib.F32 if loss.dtype == torch.float32 else _lib.F64
            if want != self.loss_dtype:
                _lib.call("dpwa_learner_set_loss_dtype", self.h, want)
                self.loss_dtype = want
            self.keep = loss
            return 0.0, ctypes.c_void_p(loss.data_ptr())
        return float(loss), None

    def publish(self, flat, loss, reuse=False):
        """flat: a uint8 tensor or a raw device address (resident parameters)."""
        if self.lr is not None and not reuse and isinstance(flat, torch.Tensor):
            self.lr.publish(flat.view(TORCH[self.kind]), loss, torch.cuda.current_stream())    # Learner's own path
            return
        h, d = self._loss(loss)
        p = flat.data_ptr() if isinstance(flat, torch.Tensor) else flat
        _lib.call("dpwa_learner_publish_reuse" if reuse else "dpwa_learner_publish", self.h, ctypes.c_void_p(p), h, d,
                  stream())

    def attach(self, peer_id, other):
        _lib.call("dpwa_learner_attach_local", self.h, peer_id, other.h)

    def fetch(self, peer_id, version, flags=0):
        _lib.call("dpwa_learner_fetch", self.h, peer_id, version, flags, stream())

    def cancel(self):
        _lib.call("dpwa_learner_cancel", self.h)

    def average(self, flat, loss=1.0, through=False):
        p = flat.data_ptr() if isinstance(flat, torch.Tensor) else flat
        _lib.call("dpwa_learner_average_through" if through else "dpwa_learner_average", self.h, ctypes.c_void_p(p),
                  float(loss), None, stream())

    def snapshot(self):
        """(header, payload bytes, version) of the latest publish, through dpwa_learner_read_snapshot."""
        out = np.full(self.nbytes, 0xEE, dtype=np.uint8)
        hdr, v = ctypes.create_string_buffer(256), ctypes.c_uint64()
        _lib.call("dpwa_learner_read_snapshot", self.h, hdr, ctypes.c_void_p(out.ctypes.data), out.nbytes,
                  ctypes.byref(v))
        return _lib.Header.from_buffer_copy(hdr.raw), out, v.value

    def clock(self):
        c = ctypes.c_double()
        _lib.call("dpwa_learner_read_clock", self.h, ctypes.byref(c))
        return c.value

    def staged(self, nbytes=None):
        """The staging buffer's payload as a uint8 tensor (what the last copying fetch pulled)."""
        return device_tensor(self.staging_payload, self.nbytes if nbytes is None else nbytes, torch.uint8, DEV)

    def resident(self):
        p, slot = ctypes.c_void_p(), ctypes.c_int()
        _lib.call("dpwa_learner_resident_params", self.h, ctypes.byref(p), ctypes.byref(slot))
        return p.value, slot.value

    def counter(self, name):
        h = ctypes.c_uint32()
        _lib.call(name, self.h, ctypes.byref(h))
        return h.value


def check_header(h, node, version, clock, loss, what):
    assert h.version == version and h.n == node.n and h.dtype == node.code, (what, h.version, h.n, h.dtype)
    assert h.clock == clock, (what, "clock", h.clock, clock)                     # dpwa.py:112
    if loss is not None:
        assert h.loss == loss, (what, "loss", h.loss, loss)


def same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "%d bytes differ, the first at %s" % (bad.size, bad[:5].tolist()),
                           [hex(int(x)) for x in got[bad[:5]]], [hex(int(x)) for x in want[bad[:5]]])


def round16(nbytes):
    return (nbytes + 15) // 16 * 16


# ---------------------------------------------------------------- publish
def publish_sizes(kind, offset):
    """The byte counts of moves_ref.PUBLISH_BYTES; an element type takes the nearest multiples of its
    size on both sides.  An unaligned `flat` (k_publish<false>) adds the size past one pass of its
    capped grid."""
    sizes = list(ref.PUBLISH_BYTES) + ([ref.PUBLISH_BIG_BYTES] if offset else [])
    if kind == "bytes":
        return sizes
    s = SIZE[kind]
    return sorted({m for b in sizes for m in (b // s * s, -(-b // s) * s) if m > 0})


def publish_case(kind, nbytes, offset):
    """Three publishes of one learner -- loss as a host double, as a float64 and as a float32 device
    scalar -- into slots 0, 1, 0: each snapshot read back is the payload, each header is right, the
    other slot keeps its payload (a reader pulls it again), and the third publish leaves the bytes
    between the payload's end and the end of its last 16-byte word as the first left them (the
    sources are followed by different bytes, so a copy that runs over shows)."""
    what = ("publish", kind, nbytes, offset)
    a, b = operand_bytes(kind, nbytes, 0), operand_bytes(kind, nbytes, 1)
    c = b ^ np.uint8(0xFF)
    src_a, chk_a = banded(a, offset, 0xA5)
    src_b, chk_b = banded(b, offset, 0x69)
    src_c, chk_c = banded(c, offset, 0x3C)
    assert offset == 0 or src_a.data_ptr() % 16 == offset
    me, reader = Node(kind, nbytes), Node(kind, nbytes)
    try:
        reader.attach(0, me)

        def pulled(version):
            reader.fetch(0, version)
            torch.cuda.synchronize()
            got = host(reader.staged(round16(nbytes)))
            reader.cancel()
            return got

        me.publish(src_a, 1.25)
        h, got, v = me.snapshot()
        assert v == 1
        check_header(h, me, 1, 1.0, 1.25, what)
        same_bytes(got, a, (what, "first publish"))
        first = pulled(1)
        same_bytes(first[:nbytes], a, (what, "slot 0 as a peer pulls it"))

        me.publish(src_b, torch.tensor(0.1, dtype=torch.float64, device=DEV))
        h, got, v = me.snapshot()
        assert v == 2
        check_header(h, me, 2, 2.0, 0.1, (what, "float64 device loss"))
        same_bytes(got, b, (what, "second publish"))
        same_bytes(pulled(1), first, (what, "the second publish touched slot 0"))
        second = pulled(2)

        me.publish(src_c, torch.tensor(0.1, dtype=torch.float32, device=DEV))
        h, got, v = me.snapshot()
        assert v == 3
        check_header(h, me, 3, 3.0, float(np.float32(0.1)), (what, "float32 device loss"))
        same_bytes(got, c, (what, "third publish"))
        third = pulled(3)
        same_bytes(third[:nbytes], c, (what, "slot 0 rewritten"))
        same_bytes(third[nbytes:], first[nbytes:], (what, "bytes just past the payload in slot 0"))
        same_bytes(pulled(2), second, (what, "the third publish touched slot 1"))
        same_bytes(second[:nbytes], b, (what, "slot 1 as a peer pulls it"))

        for src, bits, chk in ((src_a, a, chk_a), (src_b, b, chk_b), (src_c, c, chk_c)):
            chk(what)
            same_bytes(host(src), bits, (what, "a source changed"))
    finally:
        reader.close()
        me.close()


@pytest.mark.parametrize("kind,offset", [(k, o) for k in KINDS for o in ((0, 4) if k == "f32" else (0, 2, 4))])
def test_publish_at_ragged_sizes(kind, offset):
    """k_publish<true, 64> for an aligned `flat` (copy_span: the buffer descriptor's range check, the
    tail bytes in workgroup 0), k_publish<false> for one 2 or 4 bytes off the alignment (its capped
    grid's second pass at 2 MiB + 777 bytes); read_loss from a host double, a float64 and a float32
    device scalar."""
    for nbytes in publish_sizes(kind, offset):
        publish_case(kind, nbytes, offset)


# ---------------------------------------------------------------- relocate (k_copy_payload)
@pytest.mark.parametrize("kind", KINDS)
def test_relocation_moves_every_byte_and_no_other(kind):
    """A resident learner that publishes with no average in between moves its parameters into the
    other slot with k_copy_payload (publish, and dpwa_learner_relocate): the bytes at
    dpwa_learner_resident_params are the initial ones every time, the slot left behind keeps them,
    the bytes between a payload's end and the end of its last 16-byte word stay as the test set
    them, and a slot scribbled over is whole again after the copy into it."""
    for nbytes in publish_sizes(kind, 0):
        what = ("relocate", kind, nbytes)
        init = operand_bytes(kind, nbytes, 0)
        src, chk = banded(init)
        me = Node(kind, nbytes)
        try:
            _lib.call("dpwa_learner_set_resident", me.h, ctypes.c_void_p(src.data_ptr()), stream())
            p0, slot = me.resident()
            assert slot == 0
            me.publish(p0, 1.0)                                   # header only: the parameters are there
            me.publish(p0, 1.0)                                   # no average since: slot 0 -> slot 1, then the header
            p1, slot = me.resident()
            assert slot == 1 and p1 != p0
            views = [device_tensor(p, round16(nbytes), torch.uint8, DEV) for p in (p0, p1)]
            torch.cuda.synchronize()
            for i, v in enumerate(views):
                same_bytes(host(v)[:nbytes], init, (what, "after the first relocation, slot %d" % i))
                v[nbytes:] = SENTINEL                             # inside the word a pull rounds up to
            views[0][:nbytes] = 0xEE                              # the slot left behind, scribbled
            me.publish(p1, 1.0)                                   # slot 1 -> slot 0
            assert me.resident() == (p0, 0)
            torch.cuda.synchronize()
            for i, v in enumerate(views):
                got = host(v)
                same_bytes(got[:nbytes], init, (what, "after the second relocation, slot %d" % i))
                assert (got[nbytes:] == SENTINEL).all(), (what, "bytes past the payload of slot %d" % i, got[nbytes:])
            h, got, ver = me.snapshot()
            assert ver == 3
            check_header(h, me, 3, 3.0, 1.0, what)
            same_bytes(got, init, (what, "the snapshot served"))
            views[1][:nbytes] = 0xEE
            _lib.call("dpwa_learner_relocate", me.h, stream())    # slot 0 -> slot 1, no publish
            assert me.resident() == (p1, 1)
            _lib.call("dpwa_learner_relocate", me.h, stream())    # already there: nothing moves
            torch.cuda.synchronize()
            for i, v in enumerate(views):
                got = host(v)
                same_bytes(got[:nbytes], init, (what, "after dpwa_learner_relocate, slot %d" % i))
                assert (got[nbytes:] == SENTINEL).all(), (what, "bytes past the payload of slot %d" % i, got[nbytes:])
            chk(what)
            same_bytes(host(src), init, (what, "the initial parameters changed"))
        finally:
            me.close()


# ---------------------------------------------------------------- pull
def slot_room(nbytes):
    """Bytes a learner's slot holds behind its payload offset: the payload rounded up to 4 KiB
    (learner.cpp dpwa_learner_create, slot_stride)."""
    return (nbytes + 4095) // 4096 * 4096


@pytest.mark.parametrize("max_blocks", ref.PULL_BLOCKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pull_at_copy16s_edges(dtype, max_blocks):
    """A copying fetch of a local peer's snapshot with the copy kernel capped at `max_blocks`
    workgroups (k_pull: copy16's four-deep loop and remainder with the stride the cap gives), and with
    the copy engine, at moves_ref.pull_sizes(max_blocks): the staged header is the peer's, the payload
    copied out with dpwa_learner_copy_fetched into a guarded buffer is the peer's byte for byte, the
    staging buffer behind the pulled words keeps the test's bytes, and the average with the constant
    factor 0.3 that follows gives forms_ref.case's bits and the reference's clock."""
    for nbytes in ref.pull_sizes(max_blocks):
        n = nbytes // SIZE[dtype]
        p_bits, q_bits, want = fref.case(dtype, n, fref.seed_of(dtype, n), fref.PULL_FACTOR)
        p, q = np.array(p_bits).view(np.uint8), np.array(q_bits).view(np.uint8)
        me, peer = Node(dtype, nbytes), Node(dtype, nbytes)
        try:
            me.attach(1, peer)
            src, chk_src = banded(q)
            peer.publish(src, 0.75)
            peer_header = bytes(peer.snapshot()[0])
            room = me.staged(slot_room(nbytes))
            my_clock = 0.0
            for mode in (_lib.PULL_KERNEL, _lib.PULL_COPY_ENGINE):
                what = ("pull", dtype, max_blocks, nbytes, "kernel" if mode == _lib.PULL_KERNEL else "copy engine")
                _lib.call("dpwa_learner_set_pull", me.h, mode, max_blocks)
                room[:] = SENTINEL
                out, chk_out = banded(np.full(nbytes, 0xEE, dtype=np.uint8))
                flat, chk_flat = banded(p)
                torch.cuda.synchronize()
                me.fetch(1, 1)
                _lib.call("dpwa_learner_copy_fetched", me.h, ctypes.c_void_p(out.data_ptr()), stream())
                torch.cuda.synchronize()
                chk_out(what)
                same_bytes(host(out), q, (what, "the payload copied out"))
                staged = host(room)
                same_bytes(staged[:nbytes], q, (what, "the staged payload"))
                assert (staged[round16(nbytes):] == SENTINEL).all(), (
                    what, "staging written behind the pulled words",
                    np.flatnonzero(staged[round16(nbytes):] != SENTINEL)[:5].tolist())
                got_header = host(device_tensor(me.staging_header, 256, torch.uint8, DEV)).tobytes()
                assert got_header == peer_header, (what, "the staged header")
                me.average(flat)
                torch.cuda.synchronize()
                chk_flat(what)
                got = host(flat).view(fref.NUMPY[dtype])
                assert fref.same(dtype, got, want), (what, fref.mismatches(dtype, got, want))
                f, new_clock = opolicy.factor_and_clock("constant", fref.PULL_FACTOR, 0.0, my_clock, 1.0, 1.0, 0.75)
                assert f == fref.PULL_FACTOR and me.clock() == new_clock, (what, me.clock(), new_clock)
                my_clock = new_clock
            chk_src(("pull", dtype, max_blocks, nbytes))
            same_bytes(host(src), q, ("pull", dtype, max_blocks, nbytes, "the peer's parameters changed"))
            same_bytes(peer.snapshot()[1], q, ("pull", dtype, max_blocks, nbytes, "the peer's snapshot changed"))
        finally:
            me.close()
            peer.close()


# ---------------------------------------------------------------- reuse guard
def guarded_rounds(dtype, nbytes, offset, header_publish, schedule):
    """Two local learners; the first, with the reuse guard on, publishes, then per entry of
    `schedule` (generation, case, words): fetches, averages with write-through (the next slot now
    holds the parameters), has the case's words written into `flat` and publishes with
    dpwa_learner_publish_reuse.  Each time the snapshot read back must be
    moves_ref.guard_expected(snapshot, flat, generation) byte for byte and
    dpwa_learner_reuse_guard_hits grow by exactly the model's verdict.  Returns, per entry,
    (snapshot before, flat, snapshot read back)."""
    n16, tail = ref.split(nbytes)
    p, q = operand_bytes(dtype, nbytes, 0), operand_bytes(dtype, nbytes, 1)
    me, peer = Node(dtype, nbytes), Node(dtype, nbytes)
    seen = []
    try:
        me.attach(1, peer)
        src, chk_src = banded(q)
        peer.publish(src, 0.75)
        flat, chk_flat = banded(p, offset)
        assert flat.data_ptr() % 16 == offset
        _lib.call("dpwa_learner_set_reuse_guard", me.h, 1)
        _lib.call("dpwa_learner_set_header_publish", me.h, int(header_publish))
        me.publish(flat, 1.0)
        hits = me.counter("dpwa_learner_reuse_guard_hits")
        assert hits == 0
        for gen, name, words in schedule:
            what = ("reuse guard", dtype, n16, tail, offset, header_publish, "generation %d" % gen, name)
            me.fetch(1, 1)
            me.average(flat, 1.0, through=True)
            torch.cuda.synchronize()
            snap = host(flat)                                     # what the average wrote through
            at = torch.from_numpy(ref.write_offsets(words, nbytes, gen)).to(DEV)
            flat[at] = flat[at] ^ ref.FLIP
            now = host(flat)
            same_bytes(now, ref.written(snap, words, gen), (what, "the write set as applied"))
            # the loss as a host double, a float32 and a float64 device scalar in turn (k_publish_header)
            loss = 0.1 * gen
            if gen % 3 == 0:
                loss_arg, loss = torch.tensor(loss, dtype=torch.float32, device=DEV), float(np.float32(loss))
            else:
                loss_arg = torch.tensor(loss, dtype=torch.float64, device=DEV) if gen % 3 == 1 else loss
            me.publish(flat, loss_arg, reuse=True)
            h, got, v = me.snapshot()
            assert v == gen, (what, v)
            want, hit = ref.guard_expected(snap, now, gen)
            same_bytes(got, want, (what, "the snapshot after the guarded publish"))
            new_hits = me.counter("dpwa_learner_reuse_guard_hits")
            assert new_hits - hits == int(hit), (what, "hits grew by %d, the model says %d" % (new_hits - hits, hit))
            hits = new_hits
            check_header(h, me, gen, me.clock(), loss if header_publish else None, what)
            chk_flat(what)
            same_bytes(host(flat), now, (what, "the publish changed the parameters"))
            seen.append((snap, now, got))
        chk_src(("reuse guard", dtype, n16, tail))
        same_bytes(host(src), q, ("reuse guard", dtype, n16, tail, "the peer's parameters changed"))
    finally:
        me.close()
        peer.close()
    return seen


@pytest.mark.parametrize("header_publish", [False, True])
@pytest.mark.parametrize("tail", ref.GUARD_TAILS)
@pytest.mark.parametrize("n16", ref.GUARD_N16)
@pytest.mark.parametrize("dtype", DTYPES)
def test_reuse_guard_copies_exactly_the_differing_chunks(dtype, n16, tail, header_publish):
    """k_guard_publish (aligned `flat`): generations 2 to 6 and on, every case of
    moves_ref.write_sets once, with both header-only branches of the publish (the header written
    ahead by the average, or by the publish)."""
    schedule = ref.guard_schedule(n16, tail, shift=DTYPES.index(dtype))
    assert {g for g, _, _ in schedule} >= set(range(2, 7))
    guarded_rounds(dtype, n16 * 16 + tail, 0, header_publish, schedule)


@pytest.mark.parametrize("header_publish", [False, True])
@pytest.mark.parametrize("tail", ref.GUARD_TAILS)
@pytest.mark.parametrize("n16", ref.GUARD_BYTES_N16)
@pytest.mark.parametrize("dtype", DTYPES)
def test_reuse_guard_byte_form(dtype, n16, tail, header_publish):
    """k_guard_publish_bytes: the same model with `flat` 4 bytes off the alignment."""
    schedule = ref.guard_schedule(n16, tail, shift=DTYPES.index(dtype))
    guarded_rounds(dtype, n16 * 16 + tail, 4, header_publish, schedule)


def test_reuse_guard_copies_a_long_chunk_whole():
    """The smallest size whose chunks (1025 words) make the chunk copy run copy16's four-deep loop and
    its remainder with stride 256: 4095 * 1025 + 1 words, about 67 MB, float32, generation 2.  A middle
    chunk is written whole and its two neighbours everywhere but at their sampled words: the middle
    chunk alone is copied, all of it."""
    began = time.monotonic()
    n16, gen = ref.GUARD_BIG_N16, ref.GUARD_FIRST_GEN
    k, words = ref.big_guard_case(gen)
    (snap, now, got), = guarded_rounds("f32", n16 * 16, 0, False, [(gen, "long chunk", words)])
    lo, hi = ref.chunk_bounds(n16, k)
    assert hi - lo == 1025
    mid = slice(lo * 16, hi * 16)
    same_bytes(got[mid], now[mid], "the written chunk was not copied whole")
    for c in (k - 1, k + 1):
        a, b = ref.chunk_bounds(n16, c)
        same_bytes(got[a * 16:b * 16], snap[a * 16:b * 16], "a neighbour chunk (%d) was touched" % c)
        assert (now[a * 16:b * 16] != snap[a * 16:b * 16]).any()
    print("the 67 MB case took %.1f s" % (time.monotonic() - began))


# ---------------------------------------------------------------- window guard
@pytest.mark.parametrize("shift", ref.WINDOW_SHIFTS)
@pytest.mark.parametrize("tail", ref.GUARD_TAILS)
@pytest.mark.parametrize("n16", ref.WINDOW_N16)
def test_window_guard_counts_exactly_the_written_windows(n16, tail, shift):
    """k_window_roll: a resident learner with the guard on publishes (generations 1, 2, 3); each time
    a case of moves_ref.write_sets is written into the published payload, the average moves the
    parameters to the other slot and the next publish checks the window: dpwa_learner_window_hits
    grows iff moves_ref.window_expected says so; the publish that first sees the count is refused
    with DPWA_ERR_STATE and the one after goes through."""
    dtype = DTYPES[(shift + n16) % len(DTYPES)]
    nbytes = n16 * 16 + tail
    init, q = operand_bytes(dtype, nbytes, 0), operand_bytes(dtype, nbytes, 1)
    me, peer = Node(dtype, nbytes), Node(dtype, nbytes)
    try:
        me.attach(1, peer)
        src, chk_src = banded(q)
        peer.publish(src, 0.75)
        first, chk_first = banded(init)
        _lib.call("dpwa_learner_set_reuse_guard", me.h, 1)
        _lib.call("dpwa_learner_set_resident", me.h, ctypes.c_void_p(first.data_ptr()), stream())
        where = me.resident()[0]
        me.publish(where, 1.0)
        hits = me.counter("dpwa_learner_window_hits")
        assert hits == 0
        pending = False
        for gen, name, words in ref.window_schedule(n16, tail, shift):
            what = ("window guard", dtype, n16, tail, "generation %d" % gen, name)
            assert me.snapshot()[2] == gen
            view = device_tensor(where, nbytes, torch.uint8, DEV)
            published = host(view)
            at = torch.from_numpy(ref.write_offsets(words, nbytes, gen)).to(DEV)
            view[at] = view[at] ^ ref.FLIP                       # a write while peers can read it
            now = host(view)
            same_bytes(now, ref.written(published, words, gen), (what, "the write set as applied"))
            me.fetch(1, 1)
            me.average(where, 1.0)
            moved = me.resident()[0]
            assert moved != where
            if pending:                                           # the last window's count, seen first here
                with pytest.raises(_lib.DpwaError) as err:
                    me.publish(moved, 1.0)
                assert err.value.code == _lib.ERR_STATE, (what, err.value)
            me.publish(moved, 1.0)                                # (the one after) goes through
            new_hits = me.counter("dpwa_learner_window_hits")
            want = ref.window_expected(published, now, gen)
            assert new_hits - hits == int(want), (what, "hits grew by %d, the model says %d" % (new_hits - hits, want))
            same_bytes(host(view), now, (what, "the check changed the payload it read"))
            hits, pending, where = new_hits, want, moved
        chk_first()
        chk_src()
        same_bytes(host(first), init, "the initial parameters changed")
    finally:
        me.close()
        peer.close()
