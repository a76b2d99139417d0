"""The walks and directed sequences of tests/adapter_ref.py through real adapters: two learners of a
LocalGroup on one device, ``fetch_probability`` 1, every op run on the learner's module and on its twin
(a module on the same device that no adapter touches) with the same seeded values.

After every ``update_send``: a spy round ``connection.update_send`` recorded the ``reuse_snapshot`` the
model predicts; ``dpwa_learner_read_snapshot`` returns the predicted payload byte for byte and a header
with the predicted clock, loss, n, dtype and version; every parameter the module holds lies inside the
buffer that was published.  After every ``update_wait``: every parameter is bit-equal to the twin's --
the twin averaged on the host with the payload the model says the peer served -- the clock is the
policy's and ``reuse_guard_hits`` the model's.  A mismatch names the walk, the round, the learner and
the first differing byte; nothing is rerun.

The classes of the op table are observed again on the device.  A HIP error fails every later test of
this module at once without touching the GPU.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from dpwa_amd import DpwaPyTorchAdapter, _lib
from dpwa_amd.flat import FlatParameters
from dpwa_amd.group import LocalGroup
from tests import adapter_ref as A
from tests.test_gpu_gossip import write_cfg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
NAMES = ("a", "b")
BROKEN = []


def same_double(x, y):
    return (math.isnan(x) and math.isnan(y)) or np.float64(x).tobytes() == np.float64(y).tobytes()


class Pair:
    """Two adapters, their modules, their model learners (which own the twins)."""

    def __init__(self, walk, tmp_path, name):
        self.walk, self.name = walk, name
        cfg = tmp_path / "pair.yaml"
        write_cfg(cfg, NAMES, 1, walk.method, 0.0, 0.5)
        kwargs, self.many = A.FORMS[walk.form]
        group = LocalGroup()
        self.nets, self.ads, self.models, self.sent = [], [], [], [[], []]
        for g in (0, 1):
            net = A.build(walk.model, walk.seed + g).to(DEV)
            self.nets.append(net)
            self.models.append(A.Learner(walk.model, walk.seed + g, walk.form, walk.method, device=DEV))
            ad = DpwaPyTorchAdapter(net, NAMES[g], str(cfg), seed=70 + g, group=group, **kwargs)
            self.ads.append(ad)
            self.spy(ad.connection, self.sent[g])
        self.down = [False, False]

    @staticmethod
    def spy(conn, record):
        inner = conn.update_send

        def update_send(parameters, loss, reuse_snapshot=False):
            record.append((bool(reuse_snapshot), parameters))
            return inner(parameters, loss, reuse_snapshot=reuse_snapshot)
        conn.update_send = update_send

    def close(self):
        for ad in self.ads:
            ad.close()

    def where(self, r, g, what):
        return "%s\n  %s, round %d, learner %d (%s, %s, %s interpolation)" % (
            what, self.name, r, g, self.walk.model, self.walk.form, self.walk.method)

    @staticmethod
    def first_byte(got, want):
        return "first differing byte %d of %d (%d differ)" % (int(np.flatnonzero(got != want)[0]), got.size,
                                                              int((got != want).sum()))

    # ------------------------------------------------------------------ the events
    def op(self, r, g, name, seed):
        op = A.OPS[name]
        A.run_op(op, self.nets[g], self.ads[g].flat, seed)
        self.models[g].op(op, seed)

    def send(self, r, g, loss):
        ad, net, model = self.ads[g], self.nets[g], self.models[g]
        reuse, header, payload, _, _ = model.send(loss)
        ad.update_send(loss)
        assert len(self.sent[g]) == model.version, self.where(r, g, "update_send did not reach the connection once")
        got_reuse, buffer = self.sent[g][-1]
        conn = ad.connection
        out = np.full(model.lay.nbytes, 0xEE, dtype=np.uint8)
        hdr, v = ctypes.create_string_buffer(256), ctypes.c_uint64()
        _lib.call("dpwa_learner_read_snapshot", conn._learner.handle, hdr, ctypes.c_void_p(out.ctypes.data), out.nbytes,
                  ctypes.byref(v))
        h = _lib.Header.from_buffer_copy(hdr.raw)
        got = (h.clock, h.loss, h.version, h.n, h.dtype)
        assert np.array_equal(out, payload), self.where(
            r, g, "the served payload is not the model's (reuse_snapshot=%s was passed, the model says %s): %s"
            % (got_reuse, reuse, self.first_byte(out, payload)))
        assert v.value == model.version and same_double(got[0], header[0]) and same_double(got[1], header[1]) \
            and got[2:] == header[2:], self.where(r, g, "the served header is %s, the model's %s" % (got, header))
        assert got_reuse == reuse, self.where(r, g, "reuse_snapshot=%s was passed, the model says %s" % (got_reuse, reuse))
        if model.resident:
            buffer = conn.parameters
        lo = buffer.data_ptr()
        hi = lo + buffer.numel() * buffer.element_size()
        for pname, p in net.named_parameters():
            size = p.numel() * p.element_size()
            assert size == 0 or (lo <= p.data_ptr() and p.data_ptr() + size <= hi and p.is_contiguous()), self.where(
                r, g, "parameter %s is not inside the published buffer" % pname)

    def wait(self, r, waits):
        if self.many:
            DpwaPyTorchAdapter.update_wait_many(self.ads, [loss for _, loss in waits])
        served = [m.served for m in self.models]
        for g, loss in waits:
            if not self.many:
                self.ads[g].update_wait(loss)
            self.models[g].wait(loss, None if self.down[g] else served[1 - g])
        torch.cuda.synchronize()
        for g, _ in waits:
            model = self.models[g]
            got, want = A.module_bytes(self.nets[g], model.lay), A.module_bytes(model.twin, model.lay)
            assert np.array_equal(got, want), self.where(
                r, g, "the parameters after update_wait are not the twin's: %s" % self.first_byte(got, want))
            clock = self.ads[g].connection.clock
            assert same_double(float(clock), float(model.clock)), self.where(r, g, "clock %r, the policy's %r" % (clock, model.clock))
            hits = self.ads[g].reuse_guard_hits
            assert hits == model.hits, self.where(r, g, "reuse_guard_hits %d, the model's %d" % (hits, model.hits))

    def run(self, events):
        for ev in events:
            kind, r = ev[0], ev[1]
            if kind == "op":
                self.op(r, *ev[2:])
            elif kind == "send":
                self.send(r, ev[2], ev[3])
            elif kind == "down":
                self.down[ev[2]] = ev[3]
                conn, peer = self.ads[ev[2]].connection, NAMES[1 - ev[2]]
                if ev[3]:
                    conn.remove_peer(peer)          # no peer to fetch from: the round does not average
                else:
                    conn.add_peer(peer, "localhost", 46000 + 1 - ev[2])
            elif kind == "wait":
                self.wait(r, [(ev[2], ev[3])])
            else:
                self.wait(r, list(enumerate(ev[2])))


def replay(name, walk, events, tmp_path):
    if BROKEN:
        pytest.fail("an earlier test of this module met a HIP error; the GPU is left alone: %s" % BROKEN[0])
    pair = None
    try:
        pair = Pair(walk, tmp_path, name)
        pair.run(events)
    except _lib.DpwaError as e:
        if e.code == _lib.ERR_HIP:
            BROKEN.append(str(e))
        raise
    except RuntimeError as e:
        if "HIP" in str(e) or "hip" in str(e):
            BROKEN.append("%s: %s" % (type(e).__name__, e))
        raise
    finally:
        if pair is not None and not BROKEN:
            pair.close()
            torch.cuda.synchronize()


@pytest.mark.parametrize("walk", A.WALKS, ids=lambda w: w.name)
def test_walk(walk, tmp_path):
    replay(walk.name, walk, A.script(walk), tmp_path)


@pytest.mark.parametrize("name", list(A.directed()))
def test_directed_sequence(name, tmp_path):
    walk, events = A.directed()[name]
    replay(name, walk, events, tmp_path)


@pytest.mark.parametrize("model,name", [(m, op.name) for m in A.MODELS for op in A.OPS.values() if op.applies(m)])
def test_op_class_on_the_device(model, name):
    """The class the adapter can see the op by, on FlatParameters on the MI355X (a fused optimizer
    that moved version counters there would have a ``device_cls`` of its own in the table)."""
    if BROKEN:
        pytest.fail("an earlier test of this module met a HIP error; the GPU is left alone: %s" % BROKEN[0])
    net = A.build(model, 3).to(DEV)
    flat = FlatParameters(net.named_parameters())
    op = A.OPS[name]
    assert A.observe(op, net, flat, 5) == op.device_cls


def _pair(tmp_path, model, form):
    return Pair(A.Walk(model, form, "constant", 31, rounds=2), tmp_path, "%s-%s" % (model, form))


def test_a_replacement_that_changes_the_names_is_refused(tmp_path):
    """``load_state_dict(assign=True)`` unties `odd`'s tied pair: ``named_parameters()`` has a seventh
    name.  The next update_send raises DpwaError naming it and publishes nothing."""
    pair = _pair(tmp_path, "odd", "default")
    try:
        pair.run(A._rounds())
        A.load_sd_assign(pair.nets[0], pair.ads[0].flat, np.random.default_rng(1))
        with pytest.raises(_lib.DpwaError, match="t2.weight"):
            pair.ads[0].update_send(1.0)
        assert len(pair.sent[0]) == 1
    finally:
        pair.close()


@pytest.mark.parametrize("name", ["sgd_fused", "adam_fused", "adamw_fused_small"])
def test_a_fused_step_in_the_resident_window_is_refused(tmp_path, name):
    """Resident parameters are the served snapshot between update_send and update_wait; a fused step
    there moves no version counter and is refused all the same."""
    pair = _pair(tmp_path, "chunky", "resident")
    try:
        pair.run(A._rounds())
        for g in (0, 1):
            pair.ads[g].update_send(1.0)
        A.run_op(A.OPS[name], pair.nets[0], pair.ads[0].flat, 3)
        with pytest.raises(_lib.DpwaError, match="between update_send and update_wait"):
            pair.ads[0].update_wait(1.0)
    finally:
        pair.close()


def test_close_takes_the_optimizer_hook_away(tmp_path):
    import gc

    from dpwa_amd.adapters import pytorch as mod
    gc.collect()
    before = len(mod._OPEN)
    pair = _pair(tmp_path, "mixed", "default")
    assert len(mod._OPEN) == before + 2 and len(mod._HOOK) == 1
    pair.close()
    assert len(mod._OPEN) == before
    if before == 0:
        assert not mod._HOOK
