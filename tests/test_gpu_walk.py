"""The walks of tests/walk_ref.py through the C ABI: three learners of one dtype on one device, each
attached to the other two, driven call by call in this process (dpwa_amd._lib, as
tests/test_gpu_moves.py does) next to the host model.  After every call the return code is the
model's; then, with the device synchronised, every learner's parameter bits and guard bands, both
snapshot slots (header fields and payload, read as a peer reads them: an observer learner fetches the
slot and is cancelled), dpwa_learner_read_snapshot, the version, the clock, the coefficients, where
resident parameters are and the distance record (tests/dist_ref.problem, its workspace all zero) are
the model's -- after a refused call too, which must have changed none of them.  So are what the two
opt-ins show: dpwa_learner_finite_skips, the sticky status word (read where dpwa_learner_status_word
points, never polled), dpwa_learner_param_distance_rounds and the per-parameter record (its clock and
count; each tensor's pair against tests/pdist_ref.reference with dist_ref.bound of that tensor's own
elements).  The bar is bit equality with the host references (NaN positions coincide), and
dist_ref.bound for the sums.  A "step" of the model is the caller's own write of its parameters: a copy
on that learner's stream.

The second pass gives every learner a stream of its own and compares only every SYNC_EVERY calls, so
that work of several learners is in flight together; before each publish, write-through average and
relocation the producer's stream is first held for about 2 ms (torch.cuda._sleep sized from
tests/helpers.sleep_rate), so a consumer that lacks its ordering edge to that producer reads the old
bytes and fails the comparison.  The hold is a delay, never a pass criterion.  dpwa_learner_write_clock
and dpwa_learner_read_snapshot wait for the device or a stream by their contract (include/dpwa_hip.h), so
a window that holds one of them overlaps less; they stay in, as a caller may issue them there.  A mismatch
found at the end of a window names the calls of that window.

On a mismatch the message gives the walk, the index of the call and the calls so far as
walk_ref.replay_text prints them, to be replayed against the model on the host; nothing is rerun
here.  A call that returns DPWA_ERR_HIP, or a HIP error from torch, fails every later test of this
module at once without touching the GPU.
"""
import ctypes

import numpy as np
import pytest
import torch

from dpwa_amd import _lib
from dpwa_amd.devview import device_tensor
from tests import dist_ref, factor_ref, helpers
from tests import forms_ref as fref
from tests import walk_ref as W

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OFF = _lib.SLOT_PAYLOAD_OFFSET
HOLD_S = 2e-3
SYNC_EVERY = 8
BROKEN = []            # why the module stopped using the GPU (a HIP error), once it has
_RATE = []


def hold_cycles():
    if not _RATE:
        _RATE.append(helpers.sleep_rate())
    return int(HOLD_S * _RATE[0])


def vp(x):
    return ctypes.c_void_p(x)


def host(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def same_double(got, want):
    return W.bits(got) == W.bits(want)


class Node:
    """One learner through the C ABI, and the buffers the test owns for it."""

    def __init__(self, spec, cfg, i=None):
        self.spec = spec
        self.h = ctypes.c_void_p()
        _lib.call("dpwa_learner_create", ctypes.byref(self.h), 0, spec.n, spec.code, ctypes.byref(cfg))
        if spec.dtype == "mixed" and spec.n:
            from tests import mixed_ref
            lay = _lib.Layout()
            segs = mixed_ref.segments(W.MIXED_SPEC)[0]
            lay.count = len(segs)
            for k, (d, off, length, _) in enumerate(segs):
                lay.seg[k].dtype, lay.seg[k].byte_offset, lay.seg[k].byte_length = mixed_ref.CODE[d], off, length
            _lib.call("dpwa_learner_set_layout", self.h, ctypes.byref(lay))
        sh, sp = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.call("dpwa_learner_pointers", self.h, None, None, ctypes.byref(sh), ctypes.byref(sp))
        self.staging_header = device_tensor(sh.value, 256, torch.uint8, DEV)
        self.staging_payload = device_tensor(sp.value, spec.nbytes, torch.uint8, DEV) if spec.nbytes else None
        self.views = {}
        self.flats, self.checks = [], []
        if i is not None:
            for bits in spec.operands(i):
                t, chk = fref.guarded(spec.nbytes, spec.offset_bytes)
                if spec.nbytes:
                    t.copy_(torch.from_numpy(np.ascontiguousarray(bits).view(np.uint8)))
                self.flats.append(t)
                self.checks.append(chk)
            self.fetched_out, self.fetched_chk = fref.guarded(spec.nbytes, 0)
            self.factor_out = torch.zeros(1, dtype=torch.float64, device=DEV)
        self.slot_ptr = {}
        self.dist_ptr = None
        word = ctypes.c_void_p()
        _lib.call("dpwa_learner_status_word", self.h, ctypes.byref(word))
        self.status_word = ctypes.cast(word.value, ctypes.POINTER(ctypes.c_int32))

    def close(self):
        if self.h:
            _lib.call("dpwa_learner_destroy", self.h)
        self.h = None

    def view(self, ptr, nbytes):
        if (ptr, nbytes) not in self.views:
            self.views[(ptr, nbytes)] = device_tensor(ptr, nbytes, torch.uint8, DEV)
        return self.views[(ptr, nbytes)]

    def resident(self):
        p, slot = ctypes.c_void_p(), ctypes.c_int()
        _lib.call("dpwa_learner_resident_params", self.h, ctypes.byref(p), ctypes.byref(slot))
        return p.value, slot.value

    def bits(self, raw):
        return np.ascontiguousarray(raw).view(self.spec.numpy)


class Group:
    def __init__(self, spec, name, streams=False):
        self.spec, self.name = spec, name
        self.lib = _lib.load()
        cfg = _lib.Interp(W.METHOD_CODE[spec.method], 0, 0.0 if spec.value is None else spec.value, spec.threshold)
        self.cfg = cfg
        self.nodes, self.observers = [], []
        ws = ctypes.c_int64()
        _lib.call("dpwa_distance_workspace", ctypes.byref(ws))
        self.workspace_bytes = ws.value
        try:
            for i in range(spec.learners):
                self.nodes.append(Node(spec, cfg, i))
                self.observers.append(Node(spec, cfg))
            for i, a in enumerate(self.nodes):
                for j, b in enumerate(self.nodes):
                    if i != j:
                        _lib.call("dpwa_learner_attach_local", a.h, j, b.h)
                _lib.call("dpwa_learner_attach_local", self.observers[i].h, 0, a.h)
        except Exception:
            self.close()
            raise
        self.streams = [torch.cuda.Stream(DEV) for _ in self.nodes] if streams else None
        self.model = W.Model(spec)
        self.ranges = None         # the dpwa_param_range list of set_param_distance, made at its first use
        self.done = []
        self.pending = []          # outputs of copy_fetched / copy_factor not compared yet
        self.compared = -1         # index of the last call after which the whole state was compared
        torch.cuda.synchronize()

    def close(self):
        for n in self.nodes + self.observers:
            n.close()

    # ------------------------------------------------------------------ calling
    def stream(self, i):
        return vp(self.streams[i].cuda_stream if self.streams else torch.cuda.current_stream().cuda_stream)

    def hold(self, i):
        if self.streams:
            with torch.cuda.stream(self.streams[i]):
                torch.cuda._sleep(hold_cycles())

    def ptr(self, i, flat):
        node = self.nodes[i]
        if flat == "res":
            return node.resident()[0]
        return node.flats[flat].data_ptr()

    def c(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        if rc == _lib.ERR_HIP:
            BROKEN.append("%s returned DPWA_ERR_HIP: %s" % (name, self.lib.dpwa_last_error().decode(errors="replace")))
            pytest.fail(self.where("a HIP call failed: %s" % BROKEN[-1]))
        return rc

    def call(self, op):
        """Issues `op`; returns the library's return code."""
        name, a = op[0], op[1:]
        N = self.nodes
        if name in ("publish", "publish_reuse"):
            i, flat, loss = a
            self.hold(i)
            return self.c("dpwa_learner_" + name, N[i].h, vp(self.ptr(i, flat)), float(loss), None, self.stream(i))
        if name == "fetch":
            i, j, version, kind = a
            if kind != "zc":
                mode, blocks = {"ce": (_lib.PULL_COPY_ENGINE, 512), "k1": (_lib.PULL_KERNEL, 1), "k512": (_lib.PULL_KERNEL, 512)}[kind]
                _lib.call("dpwa_learner_set_pull", N[i].h, mode, blocks)
            return self.c("dpwa_learner_fetch", N[i].h, j, version, _lib.FETCH_ZERO_COPY if kind == "zc" else 0, self.stream(i))
        if name == "factor":
            return self.c("dpwa_learner_factor", N[a[0]].h, float(a[1]), None, self.stream(a[0]))
        if name == "lerp":
            return self.c("dpwa_learner_lerp", N[a[0]].h, vp(self.ptr(a[0], a[1])), self.stream(a[0]))
        if name in ("average", "average_through"):
            i, flat, loss = a
            if name == "average_through" or self.model.L[i].resident:
                self.hold(i)
            return self.c("dpwa_learner_" + name, N[i].h, vp(self.ptr(i, flat)), float(loss), None, self.stream(i))
        if name == "average_many":
            return self.average_many(a[0])
        if name == "cancel":
            return self.c("dpwa_learner_cancel", N[a[0]].h)
        if name == "relocate":
            self.hold(a[0])
            return self.c("dpwa_learner_relocate", N[a[0]].h, self.stream(a[0]))
        if name == "write_clock":
            return self.c("dpwa_learner_write_clock", N[a[0]].h, float(a[1]))
        if name == "copy_fetched":
            i = a[0]
            rc = self.c("dpwa_learner_copy_fetched", N[i].h, vp(N[i].fetched_out.data_ptr() or None), self.stream(i))
            if rc == W.OK:
                self.pending.append(("fetched", i, len(self.done)))
            return rc
        if name == "copy_factor":
            i = a[0]
            rc = self.c("dpwa_learner_copy_factor", N[i].h, vp(N[i].factor_out.data_ptr()), self.stream(i))
            if rc == W.OK:
                self.pending.append(("factor", i, len(self.done)))
            return rc
        if name == "read_snapshot":
            return self.read_snapshot(a[0])
        if name == "set_distance":
            return self.c("dpwa_learner_set_distance", N[a[0]].h, int(a[1]))
        if name == "set_header_publish":
            return self.c("dpwa_learner_set_header_publish", N[a[0]].h, int(a[1]))
        if name == "set_finite_check":
            return self.c("dpwa_learner_set_finite_check", N[a[0]].h, int(a[1]))
        if name == "set_param_distance":
            i, every = a
            if every == 0:
                return self.c("dpwa_learner_set_param_distance", N[i].h, None, 0, 1)
            if self.ranges is None:
                rs = self.spec.param_ranges()
                self.ranges = (_lib.ParamRange * len(rs))(*[_lib.ParamRange(off, length, code, 0) for off, length, code in rs])
            return self.c("dpwa_learner_set_param_distance", N[i].h, self.ranges, len(self.ranges), int(every))
        if name == "step":
            i, flat, bits = a
            raw = torch.from_numpy(np.ascontiguousarray(bits).view(np.uint8))
            dst = N[i].view(N[i].resident()[0], self.spec.nbytes) if flat == "res" else N[i].flats[flat]
            with torch.cuda.stream(self.streams[i] if self.streams else torch.cuda.current_stream()):
                dst.copy_(raw)
            return W.OK
        if name == "set_resident":
            i = a[0]
            return self.c("dpwa_learner_set_resident", N[i].h, vp(self.ptr(i, a[1] if len(a) > 1 else 0)), self.stream(i))
        raise AssertionError(op)

    def average_many(self, entries):
        """One dispatch on the first learner's stream: the caller orders that stream after the other
        learners' own work and theirs after it (a learner's calls are otherwise all on its own stream)."""
        k = len(entries)
        ls = (ctypes.c_void_p * k)(*[self.nodes[e[0]].h.value for e in entries])
        flats = (ctypes.c_void_p * k)(*[self.ptr(e[0], e[1]) for e in entries])
        loss = (ctypes.c_double * k)(*[float(e[2]) for e in entries])
        wt = (ctypes.c_int * k)(*[int(e[3]) for e in entries])
        lead = entries[0][0]
        for e in entries:
            if e[3] or self.model.L[e[0]].resident:
                self.hold(e[0])
        if self.streams:
            for e in entries[1:]:
                self.streams[lead].wait_stream(self.streams[e[0]])
        rc = self.c("dpwa_learner_average_many", ls, flats, loss, None, wt, k, self.stream(lead))
        if self.streams:
            for e in entries[1:]:
                self.streams[e[0]].wait_stream(self.streams[lead])
        return rc

    def read_snapshot(self, i):
        """dpwa_learner_read_snapshot is synchronous: compared with the model here."""
        node, sp = self.nodes[i], self.spec
        out = np.full(sp.nbytes, 0xEE, dtype=np.uint8)
        hdr, v = ctypes.create_string_buffer(256), ctypes.c_uint64()
        rc = self.c("dpwa_learner_read_snapshot", node.h, hdr, vp(out.ctypes.data if sp.nbytes else None), out.nbytes,
                    ctypes.byref(v))
        if rc == W.OK:
            self.last_snapshot = (v.value, _lib.Header.from_buffer_copy(hdr.raw), out)
        return rc

    # ------------------------------------------------------------------ comparing
    def where(self, what):
        at = len(self.done) - 1
        since = ("call %d" % at if self.compared >= at - 1 else
                 "one of the calls %d..%d (the state was last compared after call %d)" % (self.compared + 1, at, self.compared))
        return "%s\n  walk %s, %s of the list replayed by:\n  %s" % (what, self.name, since, W.replay_text(self.spec, self.done))

    def check(self, ok, *what):
        assert ok, self.where(" ".join(str(w) for w in what))

    def check_header(self, h, want, what):
        got = (h.clock, h.loss, h.version, h.n, h.dtype)
        self.check(W.header_same(got, want), what, "header", got, "expected", want)

    def check_payload(self, raw, want, what):
        node = self.nodes[0]
        self.check(self.spec.same(node.bits(raw), want), what, "differs from the model",
                   np.flatnonzero(node.bits(raw) != want)[:5].tolist())

    def compare_snapshot(self, i):
        """The result of the read_snapshot just made against the model's."""
        v, h, out = self.last_snapshot
        want_v, want_h, want_p = self.model.out
        self.check(v == want_v, "read_snapshot of learner", i, "version", v, "expected", want_v)
        if want_v:
            self.check_header(h, want_h, "read_snapshot of learner %d" % i)
            self.check_payload(out, want_p, "read_snapshot of learner %d: payload" % i)

    def compare(self):
        """Synchronises, then everything a caller can observe against the model."""
        torch.cuda.synchronize()
        m, sp = self.model, self.spec
        for kind, i, at in self.pending:
            node = self.nodes[i]
            if kind == "factor":
                got = float(node.factor_out.cpu()[0])
                self.check(same_double(got, self.pending_want[(kind, i, at)]), "copy_factor of call", at, got)
            else:
                node.fetched_chk(self.where("copy_fetched of call %d" % at))
                if sp.nbytes:
                    self.check_payload(host(node.fetched_out), self.pending_want[(kind, i, at)], "copy_fetched of call %d" % at)
        self.pending = []
        for i, (node, l) in enumerate(zip(self.nodes, m.L)):
            who = "learner %d:" % i
            self.compare_slots(i)
            for f in range(2):
                node.checks[f](self.where("%s flat %d" % (who, f)))
                if sp.nbytes:
                    self.check_payload(host(node.flats[f]), l.flats[f], "%s parameters in flat %d" % (who, f))
            v = ctypes.c_uint64()
            _lib.call("dpwa_learner_version", node.h, ctypes.byref(v))
            self.check(v.value == l.version, who, "version", v.value, "expected", l.version)
            c = ctypes.c_double()
            _lib.call("dpwa_learner_read_clock", node.h, ctypes.byref(c))
            self.check(same_double(c.value, l.clock[l.cur]), who, "clock", c.value, "expected", l.clock[l.cur], "ring", l.clock,
                       "cur", l.cur)
            coef = _lib.Coef()
            _lib.call("dpwa_learner_read_coef", node.h, ctypes.byref(coef))
            got = (coef.factor, coef.new_clock, coef.a, coef.b)
            self.check(factor_ref.same_result(got, l.coef[:4]) and coef.status == l.coef[4], who, "coefficients", got,
                       coef.status, "expected", l.coef)
            ptr, slot = node.resident()
            self.check(slot == (l.res_slot if l.resident else -1) and bool(ptr) == l.resident, who, "resident_params",
                       hex(ptr or 0), slot, "expected slot", l.res_slot if l.resident else -1)
            if l.resident:
                self.check(node.slot_ptr.setdefault(slot, ptr) == ptr and len(set(node.slot_ptr.values())) == len(node.slot_ptr),
                           who, "the resident pointer of slot", slot, "moved", node.slot_ptr)
                if sp.nbytes:
                    self.check_payload(host(node.view(ptr, sp.nbytes)), l.slots[slot].payload, who + " resident parameters")
            self.compare_distance(i)
            self.compare_options(i)

    def compare_options(self, i):
        """What the non-finite check and the per-parameter distance show (the device is synchronised)."""
        node, l, sp = self.nodes[i], self.model.L[i], self.spec
        who = "learner %d:" % i
        skips = ctypes.c_uint64()
        _lib.call("dpwa_learner_finite_skips", node.h, ctypes.byref(skips))
        self.check(skips.value == l.skips, who, "finite_skips", skips.value, "expected", l.skips)
        self.check(node.status_word[0] == l.sticky, who, "the sticky status word is", node.status_word[0], "expected", l.sticky)
        averaged, measured = ctypes.c_int64(), ctypes.c_int64()
        _lib.call("dpwa_learner_param_distance_rounds", node.h, ctypes.byref(averaged), ctypes.byref(measured))
        self.check((averaged.value, measured.value) == l.pd_rounds, who, "param_distance_rounds", averaged.value,
                   measured.value, "expected", l.pd_rounds)
        p, count = ctypes.c_void_p(), ctypes.c_int64()
        rc = self.c("dpwa_learner_param_distance", node.h, ctypes.byref(p), ctypes.byref(count))
        self.check(rc == (W.ERR_STATE if l.pd is None else W.OK), who, "dpwa_learner_param_distance returned", rc)
        if l.pd is None:
            return
        clock, written, pairs = l.pd
        lay = sp.param_layout()
        self.check(count.value == len(pairs), who, "per-parameter tensor count", count.value, "expected", len(pairs))
        raw = host(node.view(p.value, 16 + 16 * len(pairs)))
        head = np.frombuffer(raw[:16].tobytes(), dtype=[("clock", "<f8"), ("count", "<i8")])[0]
        got = np.frombuffer(raw[16:].tobytes(), dtype="<f8").reshape(-1, 2)
        self.check(same_double(float(head["clock"]), clock) and int(head["count"]) == written, who, "per-parameter record clock, count",
                   head["clock"], head["count"], "expected", clock, written)
        for t, (want_d2, want_n2) in enumerate(pairs):
            for name, g, want in (("dist2", got[t, 0], want_d2), ("norm2", got[t, 1], want_n2)):
                why = dist_ref.problem(float(g), want, max(lay.elements(t), 1))
                self.check(why is None, who, "per-parameter record, tensor %d %s:" % (t, name), why)

    def compare_slots(self, i):
        """Both slots of learner i as a peer reads them: its observer fetches slot k (a version of that
        parity), the staged header and payload are the model's, the observer is cancelled."""
        obs, l, sp = self.observers[i], self.model.L[i], self.spec
        for k in range(2):
            rc = self.c("dpwa_learner_fetch", obs.h, 0, k + 1, 0, vp(torch.cuda.current_stream().cuda_stream))
            s = l.slots[k]
            self.check(rc == (W.OK if s.published else W.ERR_STATE), "learner %d: a fetch of slot %d returned" % (i, k), rc,
                       "published:", s.published)
            if rc != W.OK:
                continue
            torch.cuda.synchronize()
            h = _lib.Header.from_buffer_copy(host(obs.staging_header).tobytes())
            self.check_header(h, s.header, "learner %d slot %d" % (i, k))
            if sp.nbytes:
                self.check_payload(host(obs.staging_payload), s.payload, "learner %d slot %d payload" % (i, k))
            _lib.call("dpwa_learner_cancel", obs.h)

    def compare_distance(self, i):
        node, l, sp = self.nodes[i], self.model.L[i], self.spec
        p = ctypes.c_void_p()
        rc = self.c("dpwa_learner_distance", node.h, ctypes.byref(p))
        self.check(rc == (W.ERR_STATE if l.dist is None else W.OK), "learner %d: dpwa_learner_distance returned" % i, rc)
        if l.dist is None:
            return
        self.check(node.dist_ptr in (None, p.value), "learner %d: the distance record moved" % i)
        node.dist_ptr = p.value
        rec = _lib.Distance.from_buffer_copy(host(node.view(p.value, 32)).tobytes())
        d2, n2, clock, n = l.dist
        for name, got, want in (("dist2", rec.dist2, d2), ("norm2", rec.norm2, n2)):
            why = dist_ref.problem(got, want, max(sp.terms(), 1))      # dist_ref.bound of the terms summed
            self.check(why is None, "learner %d: distance record %s:" % (i, name), why)
        self.check(same_double(rec.clock, clock) and rec.n == n, "learner %d: distance record clock, n" % i, rec.clock, rec.n,
                   "expected", clock, n)
        ws = node.view(p.value - self.workspace_bytes, self.workspace_bytes)
        self.check(not bool(ws.any()), "learner %d: the distance workspace is not all zero" % i)

    # ------------------------------------------------------------------ the walk
    def run(self, ops, every=1):
        self.pending_want = {}
        self.compare()
        for t, op in enumerate(ops):
            want = self.model.apply(op)
            self.done.append(op)
            got = self.call(op)
            # (the library's message belongs to its last refusal: shown only when this call was refused)
            said = "(%s)" % self.lib.dpwa_last_error().decode(errors="replace") if got != W.OK else ""
            self.check(got == want, "call", op[:3] if op[0] == "step" else op, "returned", got, said, "expected", want,
                       "rule", self.model.rule)
            if op[0] in ("copy_fetched", "copy_factor") and got == W.OK:
                self.pending_want[self.pending[-1]] = self.model.out
            if op[0] == "read_snapshot":
                self.compare_snapshot(op[1])
            # (the buffers copy_fetched and copy_factor write are one per learner: compared before reuse)
            if (t + 1) % every == 0 or t + 1 == len(ops) or op[0] in ("copy_fetched", "copy_factor"):
                self.compare()
                self.compared = t


def run_walk(name, spec, ops, streams=False):
    if BROKEN:
        pytest.fail("an earlier test of this module met a HIP error; the GPU is left alone: %s" % BROKEN[0])
    g = None
    try:
        g = Group(spec, name, streams)
        g.run(ops, SYNC_EVERY if streams else 1)
    except _lib.DpwaError as e:
        if e.code == _lib.ERR_HIP:
            BROKEN.append(str(e))
        raise
    except RuntimeError as e:          # torch's HIP errors
        BROKEN.append("%s: %s" % (type(e).__name__, e))
        raise
    finally:
        if g is not None and not BROKEN:
            g.close()
            torch.cuda.synchronize()


DIRECTED = tuple(W.directed())
SECOND_PASS_WALKS = tuple(next(w for w in W.WALKS if w[0] == p) for p in W.PROFILES)
# with the check on every walk runs in the second pass too, the unaligned one included: a pass that lacks its
# ordering edge to the peer's publish reads the old finite bytes behind the held producer and lets the poison through


@pytest.mark.parametrize("walk", W.WALKS, ids=W.walk_id)
def test_walk(walk):
    spec, ops = W.walk_of(walk)
    run_walk(W.walk_id(walk), spec, ops)


@pytest.mark.parametrize("walk", W.CHECK_WALKS, ids=W.walk_id)
def test_checking_walk(walk):
    spec, ops = W.walk_of(walk)
    run_walk(W.walk_id(walk), spec, ops)


@pytest.mark.parametrize("walk", W.CHECK_WALKS, ids=W.walk_id)
def test_checking_walk_on_separate_streams(walk):
    spec, ops = W.walk_of(walk)
    run_walk(W.walk_id(walk) + " (separate streams)", spec, ops, streams=True)


@pytest.mark.parametrize("name", DIRECTED)
def test_directed_sequence(name):
    spec, ops = W.directed()[name]
    run_walk(name, spec, ops)


@pytest.mark.parametrize("name", DIRECTED)
def test_directed_sequence_on_separate_streams(name):
    spec, ops = W.directed()[name]
    run_walk(name + " (separate streams)", spec, ops, streams=True)


@pytest.mark.parametrize("walk", SECOND_PASS_WALKS, ids=W.walk_id)
def test_walk_on_separate_streams(walk):
    spec, ops = W.walk_of(walk)
    run_walk(W.walk_id(walk) + " (separate streams)", spec, ops, streams=True)
