"""One rank of a lock-step relay job for tests/test_gpu_relay.py: a learner driven through the C ABI
as dpwa_amd/group.py's DistGroup drives it (on_bind, after_publish, after_gate), but with the picks
dictated by the test instead of drawn by a scheduler.  All ranks share GPU 0 and map each other's
snapshot slots and relay buffers over IPC.

Every rank walks tests/relay_ref.py's Job for each case -- the model of all ranks, on the host -- and
compares what it observes with what the model says its rank must observe: the staged header and
payload and the untouched staging bytes around them (the gathered forms), the averaged parameters
(bits of the host reference, forms_ref.same), guard bands, clock and coefficients, its own
snapshot unchanged by its readers, and the snapshot republished after a write-through or resident
average.

Order of a round (DistGroup's over gloo): publish, synchronise, barrier, relay_wait, phase 1,
synchronise the side stream, barrier, phase 2, the form's consumer, synchronise, compare, barrier.

Nothing waits without a limit: every barrier has a timeout; a rank that finds a mismatch or gets an
error reports it, breaks the barrier and starts no further GPU work; every rank, however it ends,
meets the others at a last barrier before it exits, so that no rank frees memory another rank's
kernels still read.
"""
import ctypes
import os
import sys
import threading
import traceback

import numpy as np

from tests import forms_ref as fref
from tests import relay_ref as ref
from tests.forms_ref import TORCH

BARRIER_S = 30.0
HANDLE = 128                          # _lib.IPC_HANDLE_BYTES
BOARD_PER_RANK = 2 * HANDLE + ref.HEADER


class Shared:
    """What the ranks share: the round barrier, the exit barrier, a board of bytes (per rank: slot
    handle, relay handle, published header) and the queue of reports to the parent."""

    def __init__(self, ctx, world):
        self.world = world
        self.barrier = ctx.Barrier(world)
        self.leave = ctx.Barrier(world)
        self.board = ctx.Array("B", world * BOARD_PER_RANK, lock=False)
        self.reports = ctx.Queue()

    def wait(self):
        self.barrier.wait(BARRIER_S)

    def put(self, rank, at, data):
        off = rank * BOARD_PER_RANK + at
        self.board[off:off + len(data)] = list(data)

    def get(self, rank, at, n):
        off = rank * BOARD_PER_RANK + at
        return bytes(self.board[off:off + n])


def differing(got, want):
    """The first offsets at which two byte arrays differ, as tests/test_gpu_moves.py same_bytes says it."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shapes %r and %r" % (got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    return "%d bytes differ, the first at %s: got %s, want %s" % (
        bad.size, bad[:5].tolist(), [hex(int(x)) for x in got[bad[:5]]], [hex(int(x)) for x in want[bad[:5]]])


class Learners:
    """This rank's learner of one case, attached to every other rank's."""

    def __init__(self, shared, rank, job, resident):
        import torch
        from dpwa_amd import _lib
        from dpwa_amd.devview import device_tensor
        from dpwa_amd.learner import Learner
        self.torch, self.lib = torch, _lib
        self.shared, self.rank, self.job, self.resident = shared, rank, job, resident
        self.dev = torch.device("cuda", 0)
        self.nbytes, self.dtype = job.nbytes, job.dtype
        self.cfg = _lib.Interp(_lib.INTERP_LOSS, 0, 0.0, 0.0)
        self.lr = Learner(self.dev, job.n, TORCH[job.dtype], self.cfg)
        self.h = self.lr.handle
        self.views = {}
        if resident:
            init = torch.zeros(self.nbytes, dtype=torch.uint8, device=self.dev)
            _lib.call("dpwa_learner_set_resident", self.h, ctypes.c_void_p(init.data_ptr()), self.stream())
            torch.cuda.synchronize()
            self.flat = self.check = None
        else:
            self.flat, self.check = fref.guarded(self.nbytes)
        self.out, self.check_out = fref.guarded(self.nbytes)
        _lib.call("dpwa_learner_relay_enable", self.h, job.world, rank)
        buf = ctypes.create_string_buffer(HANDLE)
        _lib.call("dpwa_learner_relay_handle", self.h, buf, HANDLE)
        shared.put(rank, 0, self.lr.ipc_handle())
        shared.put(rank, HANDLE, buf.raw)
        shared.wait()
        for r in range(job.world):
            if r != rank:
                self.lr.attach_ipc(r, shared.get(r, 0, HANDLE))
                blob = ctypes.create_string_buffer(shared.get(r, HANDLE, HANDLE), HANDLE)
                _lib.call("dpwa_learner_relay_attach", self.h, r, r, blob, HANDLE)
        sh, side = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.call("dpwa_learner_pointers", self.h, None, None, ctypes.byref(sh), None)
        self.staging = device_tensor(sh.value, ref.PAYLOAD_OFF + ref.slot_room(self.nbytes), torch.uint8, self.dev)
        _lib.call("dpwa_learner_side_stream", self.h, ctypes.byref(side))
        self.side = torch.cuda.ExternalStream(side.value, device=self.dev)
        self.picks = torch.full((job.world,), -1, dtype=torch.int32, device=self.dev)
        shared.wait()                   # every rank has attached: nobody's handle is still needed

    def close(self):
        self.torch.cuda.synchronize()
        self.staging = None
        self.views = {}
        self.lr.close()

    # -- small helpers ------------------------------------------------------
    def stream(self):
        return self.lib.stream_handle(None)

    def host(self, t):
        return t.contiguous().view(self.torch.uint8).cpu().numpy()

    def params(self):
        """The uint8 tensor over this rank's parameters, where they are now."""
        if not self.resident:
            return self.flat
        p = ctypes.c_void_p()
        self.lib.call("dpwa_learner_resident_params", self.h, ctypes.byref(p), None)
        if p.value not in self.views:
            from dpwa_amd.devview import device_tensor
            self.views[p.value] = device_tensor(p.value, self.nbytes, self.torch.uint8, self.dev)
        return self.views[p.value]

    def snapshot(self):
        out = np.full(self.nbytes, 0xEE, dtype=np.uint8)
        hdr, v = ctypes.create_string_buffer(ref.HEADER), ctypes.c_uint64()
        self.lib.call("dpwa_learner_read_snapshot", self.h, hdr, ctypes.c_void_p(out.ctypes.data), out.nbytes,
                      ctypes.byref(v))
        return np.frombuffer(hdr.raw, dtype=np.uint8), out, v.value

    def clock(self):
        return self.lr.read_clock()

    # -- one round ----------------------------------------------------------
    def round(self, form, t, picks, version, seen):
        torch, lib, shared = self.torch, self.lib, self.shared
        me = seen[self.rank]
        what = ("world %d, %d bytes of %s, %d blocks, form %s, round %d, rank %d picks %d"
                % (self.job.world, self.nbytes, self.dtype, self.job.blocks, form, t, self.rank, me.pick))

        def fail(*details):
            raise AssertionError(": ".join([what] + [str(d) for d in details]))

        def expect_bytes(got, want, name):
            d = differing(got, want)
            if d:
                fail(name, d)

        # 1. publish a fresh payload
        if self.resident:
            lib.call("dpwa_learner_relocate", self.h, self.stream())
        flat = self.params()
        flat.copy_(torch.from_numpy(np.array(me.published)))
        lib.call("dpwa_learner_publish", self.h, ctypes.c_void_p(flat.data_ptr()), me.loss, None, self.stream())
        self.staging.fill_(ref.SENTINEL)
        self.out.fill_(fref.GUARD_BYTE)
        torch.cuda.synchronize()                                                        # 2.
        if self.lr.native_version() != version:
            fail("publishes", self.lr.native_version(), version)
        my_header = self.snapshot()[0]
        expect_bytes(my_header[:ref.HEADER_FIELDS], me.header, "the published header")
        shared.put(self.rank, 2 * HANDLE, my_header.tobytes())
        shared.wait()                                                                   # 3.
        lib.call("dpwa_learner_relay_wait", self.h, self.stream())                      # 4.
        self.picks.copy_(torch.tensor(picks, dtype=torch.int32))
        lib.call("dpwa_learner_relay_phase1", self.h, ctypes.c_void_p(self.picks.data_ptr()), version,
                 self.job.blocks, self.stream())                                        # 5.
        self.side.synchronize()                                                         # 6.
        shared.wait()                                                                   # 7.
        lib.call("dpwa_learner_relay_phase2", self.h, ctypes.c_void_p(self.picks.data_ptr()), me.pick, version,
                 self.job.blocks, 0 if form == "gather" else 1)                         # 8.
        if me.pick >= 0:                                                                # 9.
            if form == "copy":
                lib.call("dpwa_learner_copy_fetched", self.h, ctypes.c_void_p(self.out.data_ptr()), self.stream())
                lib.call("dpwa_learner_cancel", self.h)
            else:
                lib.call("dpwa_learner_average_through" if form == "through" else "dpwa_learner_average", self.h,
                         ctypes.c_void_p(flat.data_ptr()), me.loss, None, self.stream())
        torch.cuda.synchronize()                                                        # 10.

        # 11. compare: bands first (an overrun is the plainer finding)
        if self.check is not None:
            self.check(what)
        self.check_out(what)
        staged = self.host(self.staging)
        if me.staging is None or me.pick < 0:
            bad = np.flatnonzero(staged != ref.SENTINEL)
            if bad.size:
                fail("the staging buffer was written", bad[:5].tolist())
        else:
            pick_header = np.frombuffer(shared.get(me.pick, 2 * HANDLE, ref.HEADER), dtype=np.uint8)
            expect_bytes(staged[:ref.HEADER], pick_header, "the staged header is not rank %d's" % me.pick)
            expect_bytes(staged[:ref.HEADER_FIELDS], me.peer_header[:ref.HEADER_FIELDS], "the staged header's fields")
            lo = ref.PAYLOAD_OFF
            expect_bytes(staged[lo:lo + self.nbytes], me.peer, "the staged payload")
            expect_bytes(staged[ref.HEADER:lo], me.staging[ref.HEADER:lo], "staging between header and payload")
            behind = lo + ref.round16(self.nbytes)
            expect_bytes(staged[behind:], me.staging[behind:], "staging behind the gathered words")
        params = self.host(self.params())
        copied = self.host(self.out)
        if me.factor is None:                       # no pick, or the payload only copied out
            expect_bytes(params, me.published, "the parameters changed in a round without an average")
            if form == "copy" and me.pick >= 0:
                expect_bytes(copied, me.peer, "the payload copied out")
            elif (copied != fref.GUARD_BYTE).any():
                fail("the copy's destination was written")
        else:
            want = ref.averaged(self.dtype, self.nbytes, form, self.rank, t, me.factor, me.peer)
            got = params.view(fref.NUMPY[self.dtype])
            if not fref.same(self.dtype, got, want):
                fail("the averaged parameters", fref.mismatches(self.dtype, got, want))
            c = self.lr.read_coef()
            if not (c.status == 0 and c.factor == me.factor and c.a == np.float32(me.factor)
                    and c.b == np.float32(1.0 - me.factor) and c.new_clock == me.clock_after):
                fail("the coefficients", (c.status, c.factor, c.a, c.b, c.new_clock), (me.factor, me.clock_after))
        if self.clock() != me.clock_after:
            fail("the clock", self.clock(), me.clock_after)
        header, payload, v = self.snapshot()
        if v != version:
            fail("the snapshot's version", v, version)
        expect_bytes(header, my_header, "this rank's published header changed")
        expect_bytes(payload, me.published, "this rank's published payload changed")

        if me.republish:
            # the written-through (or resident) parameters are the next snapshot, with no copy
            flat = self.params()
            lib.call("dpwa_learner_publish" if self.resident else "dpwa_learner_publish_reuse", self.h,
                     ctypes.c_void_p(flat.data_ptr()), me.loss + ref.SECOND_LOSS, None, self.stream())
            torch.cuda.synchronize()
            header, payload, v = self.snapshot()
            if v != me.republish:
                fail("the republished version", v, me.republish)
            expect_bytes(header[:ref.HEADER_FIELDS],
                         ref.header_bytes(me.republish_clock, me.loss + ref.SECOND_LOSS, v, self.job.n, self.dtype),
                         "the republished header")
            expect_bytes(payload, params, "the republished snapshot is not the averaged parameters")
            expect_bytes(self.host(self.params()), params, "the parameters changed in the republish")
        shared.wait()                                                                   # 12.


def run(shared, rank, world, only=None):
    done = 0
    for nbytes, blocks, dtype in ref.cases(world):
        if only is not None and (nbytes, blocks, dtype) not in only:
            continue
        job = ref.Job(world, nbytes, dtype, blocks)
        for forms in job.learner_sets():
            ls = Learners(shared, rank, job, resident=forms == ("resident",))
            for form, t, picks, version, seen in job.rounds(forms):
                ls.round(form, t, picks, version, seen)
                done += 1
            # after the round's last barrier nothing of any rank is in flight; a rank that failed never
            # gets here and keeps its memory until every rank has stopped (rank_main)
            ls.close()
    return done


# ---------------------------------------------------------------- payloads beyond 2^32 bytes
def attach_big(shared, rank, world, lr):
    """Enables the relay on `lr` and maps every other rank's slots and relay buffer.  Allocations this
    large are chunks shared as file descriptors: each rank serves its own (dpwa_amd/group.py's
    _FdServer, as DistGroup.on_bind does) and says where on the board, in the header's place."""
    import struct

    from dpwa_amd import _lib
    from dpwa_amd.group import _FdServer, _fetch_fds
    _lib.call("dpwa_learner_relay_enable", lr.handle, world, rank)
    buf = ctypes.create_string_buffer(HANDLE)
    _lib.call("dpwa_learner_relay_handle", lr.handle, buf, HANDLE)
    slot_fds, slot_chunk = lr.export_fds(0)
    relay_fds, relay_chunk = lr.export_fds(1)
    server = _FdServer(slot_fds + relay_fds, world - 1) if (slot_fds or relay_fds) else None
    address = server.address.encode() if server else b""
    fmt = "<6q64s"
    shared.put(rank, 0, lr.ipc_handle())
    shared.put(rank, HANDLE, buf.raw)
    shared.put(rank, 2 * HANDLE, struct.pack(fmt, len(address), len(slot_fds), slot_chunk, len(relay_fds), relay_chunk,
                                             os.getpid(), address))
    try:
        shared.wait()
        infos = {r: struct.unpack(fmt, shared.get(r, 2 * HANDLE, struct.calcsize(fmt))) for r in range(world) if r != rank}
        if server is not None:
            server.allow(info[5] for info in infos.values())
        for r, (alen, ns, cs, nr, cr, _, addr) in infos.items():
            fds = _fetch_fds(addr[:alen].decode(), ns + nr) if alen else []
            try:
                if ns:
                    lr.attach_fds(r, shared.get(r, 0, HANDLE), fds[:ns], cs)
                else:
                    lr.attach_ipc(r, shared.get(r, 0, HANDLE))
                blob = ctypes.create_string_buffer(shared.get(r, HANDLE, HANDLE), HANDLE)
                if nr:
                    arr = (ctypes.c_int * nr)(*fds[ns:])
                    _lib.call("dpwa_learner_relay_attach_fds", lr.handle, r, r, blob, HANDLE, arr, nr, cr)
                else:
                    _lib.call("dpwa_learner_relay_attach", lr.handle, r, r, blob, HANDLE)
            finally:
                for fd in fds:
                    os.close(fd)
    except BaseException:
        if server is not None:
            server.abort()
            server.thread.join(5)
            for fd in server.fds:
                os.close(fd)
            server.fds = []
        raise
    if server is not None:
        server.finish()
    shared.wait()                       # every rank has attached


def run_big(shared, rank, world, forms):
    """tests/test_gpu_big.py's relay case: a bf16 payload of big_ref.N elements (a stripe border beyond
    byte 2^31, the second stripe across byte 2^32), picks big_ref.RELAY_PICKS, one round per form with a
    fresh learner: the staged payload (gathered form) and the averaged parameters against big_ref's
    model, window by window and, on the device, element by element."""
    import torch

    from dpwa_amd import _lib
    from dpwa_amd.devview import device_tensor
    from dpwa_amd.learner import Learner
    from oracle import policy as opolicy
    from tests import big_ref
    from tests import test_gpu_big as big
    assert world == big_ref.RELAY_WORLD
    dev = torch.device("cuda", 0)
    pl = big_ref.relayed()
    n = big_ref.N["bf16"]
    pick = big_ref.RELAY_PICKS[rank]
    mine, peer = big_ref.learner(pl, rank), big_ref.learner(pl, pick)
    done = 0
    for form in forms:
        what = "relay beyond 2^32 bytes, form %s, rank %d picks %d" % (form, rank, pick)
        lr = Learner(dev, n, TORCH["bf16"], big.CFG)
        attach_big(shared, rank, world, lr)
        sh, sp, side = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _lib.call("dpwa_learner_pointers", lr.handle, None, None, ctypes.byref(sh), ctypes.byref(sp))
        staging = device_tensor(sp.value, pl.nbytes, torch.uint8, dev)
        _lib.call("dpwa_learner_side_stream", lr.handle, ctypes.byref(side))
        side = torch.cuda.ExternalStream(side.value, device=dev)
        picks = torch.tensor(big_ref.RELAY_PICKS, dtype=torch.int32, device=dev)
        flat = big.Buffer(pl, mine)
        _lib.call("dpwa_learner_publish", lr.handle, flat.ptr, 0.5 + rank, None, big.stream())
        staging.fill_(big_ref.RELAY_FILL)
        torch.cuda.synchronize()
        shared.wait()
        _lib.call("dpwa_learner_relay_wait", lr.handle, big.stream())
        _lib.call("dpwa_learner_relay_phase1", lr.handle, ctypes.c_void_p(picks.data_ptr()), 1, big_ref.RELAY_BLOCKS,
                  big.stream())
        side.synchronize()
        shared.wait()
        _lib.call("dpwa_learner_relay_phase2", lr.handle, ctypes.c_void_p(picks.data_ptr()), pick, 1, big_ref.RELAY_BLOCKS,
                  0 if form == "gather" else 1)
        _lib.call("dpwa_learner_average", lr.handle, flat.ptr, 0.5 + rank, None, big.stream())
        torch.cuda.synchronize()
        want = big_ref.relay_model(pl, mine, peer, form)
        big.expect(flat, want["param"], (what, "the averaged parameters"), const=big_ref.lerp_const(mine, peer))
        got, first = big.outcome(staging, pl, peer.const if form == "gather" else
                                 {"bf16": int(np.full(2, big_ref.RELAY_FILL, dtype=np.uint8).view(np.uint16)[0])})
        if form == "gather":
            failed = big_ref.failures(pl, got, want["staged"], exact_bytes=True)
            assert not failed, (what, "the staged payload", failed, got.stray, first)
        else:                           # the fused form gathers nothing
            assert got.stray == 0 and all((w == big_ref.RELAY_FILL).all() for _, _, w in got.windows), (
                what, "the staging buffer was written", got.stray, first)
        _, clock = opolicy.factor_and_clock("constant", big_ref.FACTOR, 0.0, 1.0, 1.0, 0.5 + rank, 0.5 + pick)
        assert lr.read_clock() == clock, (what, "the clock", lr.read_clock(), clock)
        head, hdr, v = np.zeros(4096, dtype=np.uint8), ctypes.create_string_buffer(ref.HEADER), ctypes.c_uint64()
        _lib.call("dpwa_learner_read_snapshot", lr.handle, hdr, ctypes.c_void_p(head.ctypes.data), head.nbytes, ctypes.byref(v))
        assert v.value == 1 and differing(head, mine.bytes(0, 4096)) is None, (what, "this rank's snapshot changed")
        shared.wait()                   # nobody reads this rank's slots or relay buffer any more
        del flat, staging
        lr.close()
        torch.cuda.empty_cache()
        done += 1
    return done


def big_rank_main(rank, world, shared, forms=None):
    rank_main(rank, world, shared, forms, run=run_big)


def rank_main(rank, world, shared, only=None, run=run):
    """Process entry: exit status 0, or 1 after a report ("failed", text) -- 2 when another rank broke
    the barrier first."""
    status, report = 0, None
    try:
        import torch
        torch.cuda.set_device(0)
        report = ("ok", run(shared, rank, world, only))
    except threading.BrokenBarrierError:
        status, report = 2, ("stopped", "another rank broke the barrier, or one never arrived")
    except AssertionError as e:
        status, report = 1, ("failed", str(e))
    except BaseException:
        status, report = 1, ("failed", traceback.format_exc())
    if status:
        shared.barrier.abort()
    shared.reports.put((rank,) + report)
    shared.reports.close()
    shared.reports.join_thread()
    try:                                 # every rank's GPU work is over before any rank's memory goes
        shared.leave.wait(BARRIER_S)
    except threading.BrokenBarrierError:
        pass
    sys.stdout.flush()
    os._exit(status)
