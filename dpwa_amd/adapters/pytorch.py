"""DpwaPyTorchAdapter on MI355X (mirror of dpwa/adapters/pytorch.py).

Same constructor and methods.  Instead of pickling every parameter through the host
(pytorch.py:17-34, 49-53) and averaging tensor by tensor with three ATen kernels and
three temporaries each (pytorch.py:66-68), the parameters live in one flat HBM buffer
(dpwa_amd/flat.py); update_send publishes it with one kernel and update_wait averages it
in place with one fused HIP kernel whose coefficients come from the device factor.

Differences that are intentional: the average is written in place (the reference
rebinds ``param.data`` to a new tensor), and float32, bfloat16 *and* float16 models are
accepted (the reference maps only FloatTensor, pytorch.py:11-14); the 16-bit types round as
torch-eager does on them.  A model that mixes the three (fp32 norm layers in a bf16 or fp16 body)
is accepted too, in the write-through, plain and resident forms: its flat buffer is segmented by
dtype (dpwa_amd/flat.py) and every parameter is averaged with its own dtype's rounding, as the
reference's tensor-by-tensor loop would.  Not accepted: 16-bit or mixed parameters over the wire
bridge (dpwa_amd/bridge.py carries float32 only), and ``pull='relay-avg'`` with a mixed model
(``'relay'``, ``'kernel'`` and ``'copy'`` move bytes and work); co-resident mixed learners are
averaged one launch each instead of one batched dispatch.
"""
import ctypes
import logging
import weakref

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook

from .. import _lib
from ..dpwa import DpwaConfiguration, DpwaConnection
from ..flat import FlatParameters

LOGGER = logging.getLogger(__name__)

# One process-wide optimizer hook (torch.optim's step post hook) tells every open adapter that an
# optimizer holding one of its parameters has stepped: the fused optimizers (``fused=True``) change
# the parameters and move no version counter.
_OPEN = weakref.WeakSet()
_HOOK = []


def _optimizer_stepped(optimizer, args, kwargs):
    if not _OPEN:               # every adapter was closed or collected: the hook goes too
        while _HOOK:
            _HOOK.pop().remove()
        return
    for adapter in _OPEN:
        if not adapter._stepped and adapter._holds(optimizer):
            adapter._stepped = True


def _watch(adapter):
    _OPEN.add(adapter)
    if not _HOOK:
        _HOOK.append(register_optimizer_step_post_hook(_optimizer_stepped))


def _unwatch(adapter):
    _OPEN.discard(adapter)
    if not _OPEN:
        while _HOOK:
            _HOOK.pop().remove()


class DpwaPyTorchAdapter:
    """write_through (extension, default on): the averaging kernel also writes the next
    snapshot, and the next update_send publishes only the header when nothing was modified in
    between -- 4*N*s bytes for the averaging and the publish instead of 5*N*s.  The reference
    loop never touches the parameters between update_wait and the next update_send (README.md
    and examples/pytorch-cifar/main.py:130-145: update_send, forward/backward/step, update_wait).
    Before reusing a snapshot the adapter checks that no parameter was re-homed
    (``param.data = ...``), that no parameter's version counter moved (optimizer steps,
    ``param.add_``, ``load_state_dict``), that the flat buffer's own counter did not move, that no
    optimizer holding one of the parameters stepped (torch.optim's global step hook: the fused
    optimizers, ``fused=True``, change the parameters and move no version counter) and that the
    module still holds the ``Parameter`` objects the flat buffer was built from
    (``load_state_dict(assign=True)`` and ``mod.weight = nn.Parameter(...)`` put others there: they
    are taken into the buffer when names, shapes and dtypes are unchanged, else DpwaError names
    the parameter; a model whose structure changes needs a new adapter); any of these forces a
    full publish.  update_wait makes the same two checks of storage and objects first, so it
    averages what the module holds at that call (pytorch.py:60-68 walks ``named_parameters()``
    again).  In-place writes through ``param.data`` bypass version
    counters; for them the reuse guard (``reuse_guard``, on by default) compares 4096 16-byte
    words spread over the parameters with the snapshot on the device and publishes in full when
    any differs (two small kernels per update_send, no host sync).  The sampled words move on by
    one each publish, so every word is compared once in any ceil(N*s/16/4095) publishes: a sparse
    write that one publish's samples miss is published late (by a later publish that samples it),
    not never.  A loop that writes parameters sparsely through ``param.data`` between update_wait
    and update_send and needs every snapshot exact should pass ``write_through=False``.

    resident (extension, off by default): the parameters live in the learner's own two snapshot
    slots (``DpwaConnection.make_resident``) and every ``param.data`` is re-pointed to the slot
    they are in after each update_send and update_wait -- a publish moves no bytes and an
    average moves 3*N*s (the write-through form 4*N*s), for one ``.data`` assignment per
    parameter per round on the host.  Writes through ``param.data`` are then always part of the
    next snapshot (no snapshot-reuse check is needed).  The price is the loop order: between update_send
    and update_wait the parameters ARE the snapshot peers read, so nothing may write them
    there.  The reference's loop trains exactly there (README.md:18-29,
    examples/pytorch-cifar/main.py:130-145: update_send, step, update_wait) and keeps the
    default write-through form; a resident adapter needs update_send, update_wait, step (each
    step then comes after the round's average instead of before it).  update_wait raises
    DpwaError when a parameter's (or the flat buffer's) version counter moved since update_send
    -- an optimizer step, ``param.add_``, ``load_state_dict`` in the window -- or an optimizer
    stepped there without moving one (``fused=True``).  Writes through
    ``param.data`` bypass version counters; for them the reuse guard (``reuse_guard``) is a window
    guard here: every update_send runs one small kernel that compares the parameters published at
    the previous update_send with 4096 words sampled then, and samples the new ones (no host
    wait); a window found written makes a later update_send (the first that sees the device's
    count) raise DpwaError without publishing (``window_guard_hits`` counts them, checking the last
    check).  The sampled words move on by one each publish (as the reuse guard's), so a sparse write
    repeated every window is caught within ceil(N*s/16/4095) windows.  Code that keeps raw data
    pointers of the parameters across rounds (a captured HIP graph of the training step) must
    not use it."""

    def __init__(self, net, name, config_file, write_through=True, transport="device", reuse_guard=True,
                 resident=False, track_distance=False, distance_every=1, skip_nonfinite_peer=False,
                 **connection_kwargs):
        """transport: "device" (peers are learners of this process or of the torch.distributed
        job, pulled from HBM/over xGMI) or "wire" (peers are reached over TCP at the YAML's
        host/port with the reference's protocol -- e.g. reference CPU nodes; dpwa_amd/bridge.py).

        track_distance (extension, off by default): every round that averages also measures how far
        the model was from the peer's snapshot it averaged with (``last_distance``; see
        ``DpwaConnection``).  For a single-dtype model the averaging kernel does it with no extra
        bytes in all three forms; a model that mixes dtypes pays one more read of both operands.

        track_distance="per_parameter" (device transport): also the same two sums for every parameter
        tensor, ``last_distance.parameters`` -> ``{name: ...}`` keyed by ``named_parameters()`` names
        (``ParameterDistances``), measured on every ``distance_every``-th round that averages by a
        separate pass that reads both operands once more.

        skip_nonfinite_peer (extension, off by default): a round whose fetched peer snapshot holds a NaN
        or an inf averages nothing and is counted (``nonfinite_skips``) instead of spreading it into
        this model; see ``DpwaConnection``.  One more read of the peer's snapshot per round."""
        connection_kwargs = dict(connection_kwargs, track_distance=track_distance)
        if skip_nonfinite_peer:      # (off: the connection is built exactly as before)
            connection_kwargs["skip_nonfinite_peer"] = True
        if resident and transport != "device":
            raise ValueError("resident parameters need the device transport")
        self._net = net
        gpu = DpwaConfiguration(config_file).get_gpu(name)      # optional per-node placement
        self._flat = FlatParameters(net.named_parameters(), device=None if gpu is None else torch.device("cuda", gpu))
        if transport == "wire":
            from ..bridge import SnapshotCodec, WireConnection
            self._conn = WireConnection(name, config_file, codec=SnapshotCodec.from_flat(self._flat),
                                        **connection_kwargs)
        elif transport == "device":
            if track_distance == "per_parameter":
                connection_kwargs.update(parameter_ranges=self._flat.parameter_ranges(), distance_every=distance_every)
            self._conn = DpwaConnection(name, config_file, layout=self._flat.layout, **connection_kwargs)
        else:
            raise ValueError("transport must be 'device' or 'wire'")
        self._write_through = bool(write_through) and transport == "device"
        self._resident = bool(resident)
        self._reuse_guard = bool(reuse_guard)
        self._guard_set = False
        self._versions = None
        self._sent = None           # resident: the version counters at the last update_send
        self._warned_rehome = False
        self._stepped = False       # an optimizer holding a parameter stepped since the last average
        self._optimizers = weakref.WeakKeyDictionary()     # optimizer -> (its parameter count, holds one of ours)
        self._take_slots()
        _watch(self)

    def _take_slots(self):
        """Where the module keeps each parameter: the submodule's ``_parameters`` dict, the key, and
        the object's id.  A Parameter object put in another one's place
        (``load_state_dict(assign=True)``, ``mod.weight = nn.Parameter(...)``) shows as a slot that
        holds another object; reading the slots costs a small part of a ``named_parameters()`` walk."""
        slots = [(m._parameters, k, p) for m in self._net.modules() for k, p in m._parameters.items() if p is not None]
        self._slot_dicts = [d for d, _, _ in slots]
        self._slot_keys = [k for _, k, _ in slots]
        self._slot_ids = [id(p) for _, _, p in slots]
        self._ids = {id(p) for p in self._flat.params}
        self._optimizers.clear()

    def _holds(self, optimizer):
        groups = optimizer.param_groups
        count = sum(len(g["params"]) for g in groups)
        known = self._optimizers.get(optimizer)
        if known is None or known[0] != count:
            ids = self._ids
            known = self._optimizers[optimizer] = (count, any(id(p) in ids for g in groups for p in g["params"]))
        return known[1]

    def _fold(self):
        """The module's parameters as they are now, into the flat buffer: Parameter objects that were
        replaced are adopted (or DpwaError names the one that does not fit), replaced ``.data`` is
        re-homed.  Returns how many tensors were copied in."""
        try:
            if list(map(id, map(dict.__getitem__, self._slot_dicts, self._slot_keys))) == self._slot_ids:
                return self._flat.resync()
        except KeyError:        # a parameter was deleted from its module
            pass
        try:
            taken = self._flat.adopt(self._net.named_parameters())
        except ValueError as e:
            raise _lib.DpwaError("DpwaPyTorchAdapter", _lib.ERR_STATE, str(e)) from None
        self._take_slots()
        self._versions = None
        return taken + self._flat.resync()

    def close(self):
        """Closes the connection and stops watching optimizer steps for this adapter."""
        _unwatch(self)
        self._conn.close()

    def _warn_rehome(self, moved):
        """Once per adapter: the caller re-homed a parameter (``param.data = ...``), so its loop
        works on ``param.data`` -- and in-place writes through ``.data`` move no version counter.
        When the device reuse guard has not caught any such write so far (its sampled words all
        matched), say plainly where write-through snapshots can go stale (this re-home itself is
        seen: this round publishes in full).  Reading the guard's count synchronises the device,
        once."""
        self._warned_rehome = True
        hits = self.reuse_guard_hits if self._reuse_guard else 0
        if hits == 0:
            LOGGER.warning(
                "DpwaPyTorchAdapter(%s): %d parameter(s) were re-homed through param.data. Write-through "
                "snapshots (the default) are reused when no version counter moved; in-place writes through "
                "param.data move none and are caught only if they change one of the %d words the reuse guard "
                "samples at that publish (the samples move on by one word per publish). A loop that writes parameters sparsely through param.data between update_wait and "
                "update_send must pass write_through=False, or peers may average with a snapshot that lacks "
                "those writes.", self._conn.name, moved, 4096)

    def _param_versions(self):
        return [p._version for p in self._flat.params] + [self._flat.buffer._version]

    def _check_window(self):
        """Resident form: nothing may have written the parameters since update_send (they are
        the snapshot peers read until the average)."""
        if self._sent is not None and (self._stepped or self._param_versions() != self._sent):
            raise _lib.DpwaError(
                "DpwaPyTorchAdapter.update_wait", _lib.ERR_STATE,
                "the parameters were modified between update_send and update_wait (an optimizer step?); "
                "with resident=True they are the snapshot peers read in that window, so the loop must run "
                "update_send -> update_wait -> step.  The reference's order update_send -> step -> "
                "update_wait (README.md, main.py:130-145) needs resident=False (the write-through default)")

    def update_send(self, loss):
        """pytorch.py:42-53: publish the parameters and maybe start a fetch."""
        if _lib.TRACE:
            with _lib.trace_range("adapter.update_send"):
                return self._update_send(loss)
        return self._update_send(loss)

    def _update_send(self, loss):
        if self._resident:
            if self._conn.parameters is None:          # first round: into the learner's slot 0
                self._flat.resync()
                self._flat.rehome(self._conn.make_resident(self._flat.buffer))
                if self._reuse_guard:                      # the window guard (see the class doc)
                    _lib.call("dpwa_learner_set_reuse_guard", self._conn._learner.handle, 1)
            self._fold()                               # a parameter re-homed or replaced by the caller
            self._conn.update_send(self._flat.buffer, loss)
            # a publish with no average since the last one moved the parameters into the slot it
            # published (dpwa_learner_relocate): the views follow them
            self._flat.rehome(self._conn.parameters)
            self._sent = self._param_versions()
            self._stepped = False
            return
        moved = self._fold()
        if moved and self._write_through and not self._warned_rehome:
            self._warn_rehome(moved)
        reuse = (self._write_through and moved == 0 and not self._stepped and self._versions is not None
                 and self._versions == self._param_versions())
        self._versions = None
        self._conn.update_send(self._flat.buffer, loss, reuse_snapshot=reuse)
        if self._write_through and self._reuse_guard and not self._guard_set:    # bound by now
            _lib.call("dpwa_learner_set_reuse_guard", self._conn._learner.handle, 1)
            self._guard_set = True

    def update_wait(self, loss):
        """pytorch.py:55-68: wait for the fetch and average in place (resident: into the other
        slot, where the parameters are re-pointed)."""
        if _lib.TRACE:
            with _lib.trace_range("adapter.update_wait"):
                return self._update_wait(loss)
        return self._update_wait(loss)

    def _update_wait(self, loss):
        if self._resident:
            if self._conn.parameters is None:         # no update_send yet: nothing to average
                return
            self._check_window()
            self._conn.update_wait_average(self._flat.buffer, loss)
            self._flat.rehome(self._conn.parameters)
            self._sent = None
            return
        self._fold()           # what the module holds now is averaged (pytorch.py:60-68 walks it again)
        payload, _ = self._conn.update_wait_average(self._flat.buffer, loss, write_through=self._write_through)
        if self._write_through and payload is not None:
            self._versions = self._param_versions()
            self._stepped = False

    # -- extensions -------------------------------------------------------------------
    @staticmethod
    def update_wait_many(adapters, losses):
        """update_wait of several adapters whose models share a GPU (co-resident learners of
        one process), in order, with their averages as one dispatch (same results as calling
        update_wait on each)."""
        adapters = list(adapters)
        if not adapters:
            return
        wts = {(a._write_through, a._resident) for a in adapters}
        if len(wts) != 1 or any(not isinstance(a._conn, DpwaConnection) or type(a._conn) is not DpwaConnection
                                for a in adapters):
            for a, loss in zip(adapters, losses):     # mixed forms or wire peers: one by one
                a.update_wait(loss)
            return
        wt, resident = wts.pop()
        if resident:
            for a in adapters:
                a._check_window()
        else:
            for a in adapters:
                a._fold()
        res = DpwaConnection.update_wait_average_many([a._conn for a in adapters],
                                                      [a._flat.buffer for a in adapters], list(losses),
                                                      write_through=wt)
        for a, (payload, _) in zip(adapters, res):
            if resident and a._conn.parameters is not None:
                a._flat.rehome(a._conn.parameters)
                a._sent = None
            elif wt and payload is not None:
                a._versions = a._param_versions()
                a._stepped = False

    def state_dict(self):
        """The connection's gossip state (clock, scheduler) for a checkpoint beside the model's
        (extension: the reference checkpoints the net but restarts dpwa's clock at 0)."""
        return self._conn.state_dict()

    def load_state_dict(self, state):
        self._conn.load_state_dict(state)

    @property
    def reuse_guard_hits(self):
        """Publishes whose reuse guard found the parameters changed behind the version counters
        (synchronises the device; 0 before the first publish)."""
        if self._conn._learner is None:
            return 0
        hits = ctypes.c_uint32()
        _lib.call("dpwa_learner_reuse_guard_hits", self._conn._learner.handle, ctypes.byref(hits))
        return hits.value

    @property
    def window_guard_hits(self):
        """Resident form: rounds whose parameters the window guard found written between
        update_send and update_wait (waits for the last check; 0 before the first publish)."""
        if self._conn._learner is None:
            return 0
        hits = ctypes.c_uint32()
        _lib.call("dpwa_learner_window_hits", self._conn._learner.handle, ctypes.byref(hits))
        return hits.value

    @property
    def nonfinite_skips(self):
        """Rounds skipped because the peer's snapshot held a NaN or an inf (``skip_nonfinite_peer=True``;
        an int, 0 with the switch off).  Reading it waits for the device."""
        return self._conn.nonfinite_skips

    @property
    def last_distance(self):
        """The connection's ``last_distance`` (``PeerDistance``): None until a round has averaged
        with ``track_distance=True``.  Its ``.distance`` / ``.norm`` / ``.relative`` / ``.clock``
        read the device record and synchronise with the stream that averaged; ``.tensor()`` does not."""
        return self._conn.last_distance

    def consensus(self, out=None, distance=True, members=None):
        """``DpwaConnection.consensus`` for the model (device transport): the returned object also has
        ``parameters()`` -> ``{name: tensor}``, views of the mean with the parameters' shapes and
        dtypes, and ``load_into(module)``, which copies them into a model of the same structure."""
        if type(self._conn) is not DpwaConnection:
            from ..consensus import WIRE
            raise ValueError(WIRE)
        from ..consensus import ModelConsensus
        return ModelConsensus(self._conn.consensus(out, distance, members), self._flat)

    @property
    def connection(self):
        return self._conn

    @property
    def flat(self):
        return self._flat
