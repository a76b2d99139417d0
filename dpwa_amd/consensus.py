"""The consensus of a gossip group (``DpwaConnection.consensus``; dpwa_consensus in include/dpwa_hip.h).

Gossip training ends with G replicas that are close but not equal.  The consensus model -- the
element-wise mean of the replicas' published snapshots -- is the one to evaluate and save, and the
consensus distance ``sqrt(1/G * sum_i ||x_i - mean||^2)`` says how far apart the group is.  One
kernel pass reads the G snapshots where they are (the learners' published slots, local or mapped),
stores the mean once and forms the sums from the operands it holds: (G + 1) * N * s bytes, no
temporaries, and a rounding that does not depend on the order anything happened to run in.
"""
import ctypes

import torch

from . import _lib

RELAY_AVG = ("consensus() is not available with pull='relay-avg': the relay's fused second phase leaves no "
             "contiguous snapshot; use 'relay', 'kernel' or 'copy'")
WIRE = ("consensus() is not available with transport='wire': the snapshots of peers reached over TCP are not in "
        "memory this device can read")
TOO_MANY = "consensus() averages at most %d members in one pass, got %%d" % _lib.CONSENSUS_MAX


class Consensus:
    """What ``consensus()`` returns.  ``tensor()`` is the flat mean, with the dtype and layout of the
    payload (the segmented ``torch.uint8`` buffer of a model that mixes dtypes) -- no host sync.
    ``spread2`` (``sum_i sum_j (x_i[j] - mean[j])^2``), ``norm2`` (``sum_j mean[j]^2``),
    ``member_spread2`` (``{node name: its own sum}``), ``distance`` (``sqrt(spread2 / G)``, the
    consensus distance), ``relative`` (``sqrt(spread2 / (G * norm2))``) and ``version`` are Python
    values read from the device record, so each of them synchronises with the stream the call ran on.
    All sums are float64 against the float64 mean, not the stored one; they are added across
    workgroups in no fixed order and so are reproducible to the summation bound, not bit-exact."""

    def __init__(self, names, version, out, record, stream):
        self.members = list(names)
        self._version = version
        self._out = out
        self._record = record
        self._stream = stream
        self._rec = None

    def tensor(self):
        if self._out is None:
            raise RuntimeError("this consensus was measured only (out=False): no mean was stored")
        return self._out

    def read(self):
        """The whole record as a ``_lib.ConsensusRecord``; synchronises (once)."""
        if self._record is None:
            raise RuntimeError("this consensus was taken with distance=False: nothing was measured")
        if self._rec is None:
            rec = _lib.ConsensusRecord()
            self._stream.synchronize()
            torch.frombuffer(rec, dtype=torch.uint8).copy_(self._record)
            self._rec = rec
        return self._rec

    @property
    def spread2(self):
        return float(self.read().spread2)

    @property
    def norm2(self):
        return float(self.read().norm2)

    @property
    def member_spread2(self):
        rec = self.read()
        return {name: float(rec.member_spread2[i]) for i, name in enumerate(self.members)}

    @property
    def distance(self):
        return (self.spread2 / len(self.members)) ** 0.5

    @property
    def relative(self):
        rec = self.read()
        if rec.norm2 == 0.0:
            return 0.0 if rec.spread2 == 0.0 else float("inf")
        return (rec.spread2 / (len(self.members) * rec.norm2)) ** 0.5

    @property
    def version(self):
        return int(self.read().version) if self._record is not None else self._version

    def __repr__(self):
        return "Consensus(members=%r, version=%d)" % (self.members, self._version)


class ModelConsensus(Consensus):
    """The adapter's :class:`Consensus`: also ``parameters()`` -> ``{name: tensor}``, views of the mean
    with the parameters' shapes and dtypes, and ``load_into(module)``."""

    def __init__(self, base, flat):
        super().__init__(base.members, base._version, base._out, base._record, base._stream)
        self._flat = flat

    def parameters(self):
        buf = self.tensor()
        return {name: self._flat._view(buf, i) for i, name in enumerate(self._flat.names)}

    def load_into(self, module):
        """Copies the consensus model into ``module``'s parameters (same names and shapes)."""
        mean = self.parameters()
        own = dict(module.named_parameters())
        missing = [name for name in mean if name not in own]
        if missing:
            raise KeyError("the module has no parameter %r" % missing[0])
        with torch.no_grad():
            for name, t in mean.items():
                own[name].copy_(t)
        return module


def consensus(conn, out=None, distance=True, members=None):
    """``DpwaConnection.consensus``'s body."""
    if conn._pull.partition(":")[0] == "relay-avg" or getattr(conn._group, "relay_fused", False):
        raise ValueError(RELAY_AVG)
    refusal = getattr(conn._group, "consensus_refusal", WIRE)      # (a group without the attribute: the wire's)
    if refusal:
        raise ValueError(refusal)
    learner = conn._learner
    if learner is None or learner.version == 0:
        raise RuntimeError("consensus() is valid after this connection's first update_send")
    sources = conn._group.consensus_sources
    version = learner.version
    picked = sources(conn, members)             # [(node name, learner peer id)], YAML node order
    if not picked:
        raise ValueError("consensus(): no member")
    if len(picked) > _lib.CONSENSUS_MAX:
        raise ValueError(TOO_MANY % len(picked))
    if out is False:
        out = None
        if not distance:
            raise ValueError("consensus(out=False, distance=False) has nothing to do")
    elif out is None:
        out = torch.empty(learner.numel, dtype=learner.dtype, device=learner.device)
    elif (not isinstance(out, torch.Tensor) or out.device != learner.device or out.dtype != learner.dtype
          or out.numel() != learner.numel or not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError("consensus(out=...) needs a contiguous, 16-byte aligned %s tensor of %d elements on %s"
                         % (learner.dtype, learner.numel, learner.device))
    record = torch.empty(ctypes.sizeof(_lib.ConsensusRecord), dtype=torch.uint8, device=learner.device) \
        if distance else None
    stream = torch.cuda.current_stream(learner.device)
    ids = (ctypes.c_int32 * len(picked))(*[pid for _, pid in picked])
    _lib.call("dpwa_learner_consensus", learner.handle, ids, len(picked), version,
              ctypes.c_void_p(out.data_ptr()) if out is not None else None,
              ctypes.c_void_p(record.data_ptr()) if record is not None else None,
              ctypes.c_void_p(stream.cuda_stream))
    return Consensus([name for name, _ in picked], version, out, record, stream)
