"""A host model of what DpwaPyTorchAdapter publishes, against the reference's snapshot rule.

The reference's ``update_send`` serves the bytes of ``net.named_parameters()`` as they are at that
call (dpwa/adapters/pytorch.py:49-53) and ``update_wait`` averages what the module holds then, tensor
by tensor, rebinding ``param.data`` (pytorch.py:60-68).  The adapter here decides per ``update_send``
whether to copy the parameters or to reuse the snapshot the last average wrote through
(dpwa_amd/adapters/pytorch.py).  This module states what every publish must serve, without a GPU
library and without torch on a device of its own choosing:

* ``OPS``: what user code does to a model between the two calls -- optimizer steps, loads, conversions,
  writes through ``.data`` -- each with the class the adapter can see it by (``CLASSES``);
* ``MODELS``: four small models whose layouts meet the adapter's edges;
* the twin rule: every learner has a twin module no adapter touches.  Every op runs on both with the
  same seeded values; the twin's average is done here (oracle.lerp, factor and clock from
  oracle.policy, the other operand the payload this model says the peer served) and bound back with
  ``p.data = ...``.  The twin's bits are the expectation;
* ``Learner``: the decision (reuse or copy), the served payload (tests/moves_ref.guard_expected for a
  guarded reuse), the header, the guard's count;
* ``WALKS`` and ``directed()``: the committed seeded walks and the directed sequences, as scripts of
  events a driver replays (``run_host`` replays them on the model alone; tests/test_gpu_adapter.py next
  to real adapters);
* ``MUTANTS``: wrong adapters restated on the model.

The decision.  ``reuse`` is true exactly when the form is write-through, the previous ``update_wait``
averaged, and no op since then was ``counted``, ``rehomed`` or ``replaced`` or was an optimizer step.
The last clause is not a class: the fused optimizers move no version counter (their class is
``silent``), and the adapter learns of them from torch.optim's step hook, which fires for every
optimizer -- so a step with no gradients (class ``none``) also makes the next publish a full one.
"""
import functools
import math
import struct

import numpy as np
import torch
from torch.nn.utils import clip_grad_norm_, vector_to_parameters

from oracle import lerp as olerp
from oracle import policy
from tests import moves_ref
from tests.helpers import guard_chunk, guard_period

CLASSES = ("counted", "rehomed", "replaced", "silent", "none")
ALIGN = 256
BLOCK = 4096
CODE = {"f32": 0, "bf16": 1, "mixed": 4}              # DPWA_F32 / DPWA_BF16 / DPWA_MIXED
DTYPE = {torch.float32: "f32", torch.bfloat16: "bf16"}
SIZE = {"f32": 4, "bf16": 2}
LR = 0.05


# ---------------------------------------------------------------------------------- models
class Odd(torch.nn.Module):
    """A 0-dim parameter, an empty one, a tied pair, a non-contiguous one and a few Linears: six
    names, below 4,096 16-byte words, so every word is its own guard chunk and the guard is exact."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 7)
        self.nc = torch.nn.Parameter(torch.zeros(5, 7).t())          # non-contiguous, storage of its own
        self.s = torch.nn.Parameter(torch.tensor(1.5))
        self.e = torch.nn.Parameter(torch.zeros(0))
        self.t1 = torch.nn.Linear(3, 3, bias=False)
        self.t2 = torch.nn.Linear(3, 3, bias=False)
        self.t2.weight = self.t1.weight


class Chunky(torch.nn.Module):
    """6,000 elements no step of the directed sequences trains, 64 trained ones, then 40,000: 11,520
    words, W = 3."""

    def __init__(self):
        super().__init__()
        self.frozen = torch.nn.Parameter(torch.zeros(6000))
        self.small = torch.nn.Parameter(torch.zeros(64))
        self.big = torch.nn.Parameter(torch.zeros(40000))


def _fill(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(tuple(p.shape), generator=g).to(p.dtype))
    return net


def _bf16(seed):
    net = torch.nn.Sequential(torch.nn.Linear(300, 200), torch.nn.Linear(200, 10))
    return _fill(net, seed).bfloat16()


def _mixed(seed):
    net = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.LayerNorm(17), torch.nn.Linear(17, 9),
                              torch.nn.LayerNorm(9), torch.nn.Linear(9, 5))
    _fill(net, seed)
    for m in net:
        if isinstance(m, torch.nn.Linear):
            m.to(torch.bfloat16)
    return net


MODELS = {"odd": lambda seed: _fill(Odd(), seed), "chunky": lambda seed: _fill(Chunky(), seed),
          "bf16": _bf16, "mixed": _mixed}


def build(model, seed):
    """A fresh CPU module of `model` with seeded values."""
    return MODELS[model](seed)


# ---------------------------------------------------------------------------------- layout
class Layout:
    """dpwa_amd/flat.py restated: ranges [(name, dtype, byte offset, byte length)] in
    ``named_parameters()`` order, the payload's bytes, the header's n and dtype code, and for a model
    that mixes dtypes the segments [(dtype, byte offset, byte length)]."""

    def __init__(self, net):
        named = [(name, DTYPE[p.dtype], p.numel()) for name, p in net.named_parameters()]
        kinds = [d for d in ("f32", "bf16") if any(k == d for _, k, _ in named)]
        self.ranges, self.segments = [None] * len(named), None
        off = 0
        if len(kinds) == 1:
            self.kind = kinds[0]
            for i, (name, d, n) in enumerate(named):
                self.ranges[i] = (name, d, off, n * SIZE[d])
                off += (n * SIZE[d] + ALIGN - 1) // ALIGN * ALIGN
            self.n = off // SIZE[self.kind]
        else:
            self.kind, self.segments = "mixed", []
            for d in kinds:
                begin = off
                for i, (name, k, n) in enumerate(named):
                    if k == d:
                        self.ranges[i] = (name, d, off, n * SIZE[d])
                        off += (n * SIZE[d] + ALIGN - 1) // ALIGN * ALIGN
                off = (max(off, begin + 1) + BLOCK - 1) // BLOCK * BLOCK
                self.segments.append((d, begin, off - begin))
            self.n = off
        self.nbytes = off
        self.code = CODE[self.kind]

    def digest(self):
        """dpwa_layout_digest: FNV-1a over each segment's (int32 code, int64 offset, int64 length)."""
        if self.segments is None:
            return 0
        h = 2166136261
        for d, off, length in self.segments:
            for byte in struct.pack("<iqq", CODE[d], off, length):
                h = ((h ^ byte) * 16777619) & 0xffffffff
        return h or 1

    def gaps(self):
        """A boolean mask of the payload's bytes that belong to no parameter."""
        mask = np.ones(self.nbytes, dtype=bool)
        for _, _, off, length in self.ranges:
            mask[off:off + length] = False
        return mask


def tensor_bytes(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8).cpu().numpy()


def module_bytes(net, lay):
    """The module's parameters as a full publish serves them: laid out by `lay`, every gap byte zero."""
    out = np.zeros(lay.nbytes, dtype=np.uint8)
    for (_, _, off, length), (_, p) in zip(lay.ranges, net.named_parameters()):
        out[off:off + length] = tensor_bytes(p)
    return out


def bind_bytes(net, lay, data):
    """The reference's update_wait: every parameter is rebound to a new tensor (pytorch.py:68)."""
    for (_, d, off, length), (_, p) in zip(lay.ranges, net.named_parameters()):
        if length == 0:
            t = torch.empty(p.shape, dtype=p.dtype)
        else:
            t = torch.from_numpy(data[off:off + length].copy()).view(p.dtype).reshape(p.shape)
        p.data = t.to(p.device)


def average(lay, mine, peer, factor):
    """The averaged payload: per parameter the host reference of its dtype; gap bytes stay zero."""
    out = np.zeros(lay.nbytes, dtype=np.uint8)
    for _, d, off, length in lay.ranges:
        p, q = mine[off:off + length], peer[off:off + length]
        if d == "f32":
            r = olerp.lerp_f32(p.view(np.float32), q.view(np.float32), factor)
        else:
            r = olerp.lerp_bf16(p.view(np.uint16), q.view(np.uint16), factor)
        out[off:off + length] = np.ascontiguousarray(r).view(np.uint8)
    return out


# ---------------------------------------------------------------------------------- ops
def params(net):
    return [p for _, p in net.named_parameters()]


def target(net, which):
    """'first': the first parameter; 'small': the smallest non-empty one that is not the first;
    'last': the last non-empty one."""
    ps = [p for p in params(net) if p.numel()]
    if which == "first":
        return params(net)[0]
    if which == "last":
        return ps[-1]
    return min(ps[1:], key=lambda p: p.numel())


def name_of(net, p):
    return next(name for name, q in net.named_parameters() if q is p)


def values(rng, like, scale=1.0):
    """Seeded values shaped like `like`, on its device in its dtype (drawn on the host)."""
    a = np.asarray(rng.standard_normal(size=tuple(like.shape)), dtype=np.float32) * np.float32(scale)
    return torch.from_numpy(np.ascontiguousarray(a)).reshape(tuple(like.shape)).to(device=like.device, dtype=like.dtype)


def set_grads(net, rng, only=None):
    for p in params(net):
        p.grad = values(rng, p, 0.1) if only is None or p is only else None


def optimizer(net, key, make):
    """The model's optimizer `key`, created at its first step (after the adapter, as the README says)
    and kept for the walk; a loop that replaces Parameter objects makes its optimizers anew."""
    held = net.__dict__.setdefault("_ref_optimizers", {})
    now = {id(p) for p in params(net)}
    if key not in held or {id(p) for group in held[key].param_groups for p in group["params"]} != now:
        held[key] = make(params(net))       # (made anew once the module holds other Parameter objects)
    return held[key]


OPTIMIZERS = {
    # (no momentum: torch's fused SGD cannot take up a parameter whose first gradient comes after
    # the others' first step)
    "sgd_fused": lambda ps: torch.optim.SGD(ps, lr=LR, fused=True),
    "adam_fused": lambda ps: torch.optim.Adam(ps, lr=LR, fused=True),
    "adamw_fused": lambda ps: torch.optim.AdamW(ps, lr=LR, fused=True),
    "sgd_foreach": lambda ps: torch.optim.SGD(ps, lr=LR, momentum=0.9, foreach=True),
    "sgd_single": lambda ps: torch.optim.SGD(ps, lr=LR, momentum=0.9, foreach=False),
    "adam_foreach": lambda ps: torch.optim.Adam(ps, lr=LR, foreach=True),
    "adagrad": lambda ps: torch.optim.Adagrad(ps, lr=LR, foreach=True),
    "rmsprop": lambda ps: torch.optim.RMSprop(ps, lr=LR, foreach=False),
}


def step(key, grads="all"):
    def fn(net, flat, rng):
        if grads == "all":
            set_grads(net, rng)
        elif grads == "small":
            set_grads(net, rng, only=target(net, "small"))
        else:
            set_grads(net, rng, only=())
        optimizer(net, key, OPTIMIZERS[key]).step()
    return fn


def _state(net, rng):
    return {k: v.detach().clone() + values(rng, v, 0.25) for k, v in net.state_dict().items()}


def load_sd(net, flat, rng):
    net.load_state_dict(_state(net, rng))


def load_sd_assign(net, flat, rng):
    net.load_state_dict(_state(net, rng), assign=True)


def attr_replace(net, flat, rng):
    p = target(net, "small")
    name = name_of(net, p)
    owner = net.get_submodule(name.rpartition(".")[0])
    setattr(owner, name.rpartition(".")[2], torch.nn.Parameter(values(rng, p)))


def detach_add(net, flat, rng):
    p = target(net, "small")
    p.detach().add_(values(rng, p))


def init_normal(net, flat, rng):
    p = target(net, "last")
    torch.manual_seed(int(rng.integers(1 << 30)))
    torch.nn.init.normal_(p)          # drawn on the parameter's device, from the seed just set


def copy_nograd(net, flat, rng):
    p = target(net, "last")
    with torch.no_grad():
        p.copy_(values(rng, p))


def nograd_add(net, flat, rng):
    p = target(net, "first")
    with torch.no_grad():
        p.add_(values(rng, p))


def _through_flat(how):
    """A write through the adapter's own buffer (`flat.buffer`) or one of its views (`flat.view`), as
    code that holds the FlatParameters may do; on a twin, which has no flat buffer, the same values
    added to the same parameter."""
    def fn(net, flat, rng):
        p = target(net, "last")
        x = values(rng, p)
        name = name_of(net, p)
        if flat is None or p.data_ptr() != flat.view(name).data_ptr():
            # a twin -- or a parameter an earlier op took out of the buffer (re-homed or replaced, which
            # the adapter folds back at its next call): the write goes where the parameter is
            p.data.add_(x)
            return
        if how == "view":
            flat.view(name).add_(x)
            return
        _, dtype, off, length = next(r for r in flat.parameter_ranges() if r[0] == name)
        flat.buffer.view(torch.uint8)[off:off + length].view(dtype).add_(x.reshape(-1))
    return fn


def half_float(net, flat, rng):
    net.half()
    net.float()


def double_float(net, flat, rng):
    net.double()
    net.float()


def vec_to_params(net, flat, rng):
    vec = torch.cat([p.detach().reshape(-1) for p in params(net)])
    vector_to_parameters(vec + values(rng, vec), params(net))


def set_(net, flat, rng):
    p = target(net, "small")
    with torch.no_grad():
        p.set_(values(rng, p))


def data_assign(net, flat, rng):
    p = target(net, "last")
    p.data = p.data + values(rng, p)


def data_add(net, flat, rng):
    p = target(net, "small")
    p.data.add_(values(rng, p))


def _at(p, k):
    """The index of element k in row-major order (the parameter may be non-contiguous)."""
    return tuple(int(i) for i in np.unravel_index(k, tuple(p.shape)))


def data_index(net, flat, rng):
    """One element of the largest parameter: in a model with chunks of several words the publish's
    samples may miss it."""
    p = max(params(net), key=lambda q: q.numel())
    k = int(rng.integers(p.numel()))
    p.data[_at(p, k)] = float(np.float32(rng.standard_normal()) + np.float32(3.0))


def data_pair(net, flat, rng):
    """Two neighbouring elements of the largest parameter."""
    p = max(params(net), key=lambda q: q.numel())
    k = int(rng.integers(max(p.numel() - 1, 1)))
    for i in range(k, min(k + 2, p.numel())):
        p.data[_at(p, i)] *= -1.5


def foreach_data(net, flat, rng):
    ps = params(net)
    torch._foreach_add_([p.data for p in ps], [values(rng, p) for p in ps])


def clip_only(net, flat, rng):
    set_grads(net, rng)
    clip_grad_norm_(params(net), 1.0)


def freeze(net, flat, rng):
    p = target(net, "small")
    p.requires_grad_(not p.requires_grad)


class Op:
    def __init__(self, name, cls, fn, steps=False, first=False, buffer=False, fused=False, only=None, device_cls=None):
        assert cls in CLASSES
        self.name, self.cls, self.fn, self.steps = name, cls, fn, steps
        self.first = first          # a counted op that moves the first parameter's counter
        self.buffer = buffer        # a counted op that moves the flat buffer's counter only
        self.fused = fused
        self.only = only            # the models it applies to (None: all)
        # the class observed on the MI355X where it differs from the CPU's (None: the same)
        self.device_cls = device_cls or cls

    def applies(self, model):
        return self.only is None or model in self.only


# torch's fused optimizer kernels refuse `odd` on the device (check_fast_path_restrictions)
FUSABLE = ("chunky", "bf16", "mixed")
F32 = ("odd", "chunky")             # conversions through other dtypes: float32 models only
UNTIED = ("chunky", "bf16", "mixed")    # load_state_dict(assign=True) unties a tied pair: the names change
OPS = {op.name: op for op in (
    Op("sgd_fused", "silent", step("sgd_fused"), steps=True, fused=True, only=FUSABLE),
    Op("adam_fused", "silent", step("adam_fused"), steps=True, fused=True, only=FUSABLE),
    Op("adamw_fused", "silent", step("adamw_fused"), steps=True, fused=True, only=FUSABLE),
    Op("sgd_fused_small", "silent", step("sgd_fused", "small"), steps=True, fused=True, only=FUSABLE),
    Op("adam_fused_small", "silent", step("adam_fused", "small"), steps=True, fused=True, only=FUSABLE),
    Op("adamw_fused_small", "silent", step("adamw_fused", "small"), steps=True, fused=True, only=FUSABLE),
    Op("sgd_foreach", "counted", step("sgd_foreach"), steps=True, first=True),
    Op("sgd_single", "counted", step("sgd_single"), steps=True, first=True),
    Op("adam_foreach", "counted", step("adam_foreach"), steps=True, first=True),
    Op("adagrad", "counted", step("adagrad"), steps=True, first=True),
    Op("rmsprop", "counted", step("rmsprop"), steps=True, first=True),
    Op("sgd_one_small", "counted", step("sgd_single", "small"), steps=True),
    Op("step_no_grads", "none", step("sgd_single", "none"), steps=True),
    Op("load_sd", "counted", load_sd, first=True),
    Op("load_sd_assign", "replaced", load_sd_assign, only=UNTIED),
    Op("attr_replace", "replaced", attr_replace),
    Op("detach_add", "counted", detach_add),
    Op("init_normal", "counted", init_normal),
    Op("copy_nograd", "counted", copy_nograd),
    Op("nograd_add", "counted", nograd_add, first=True),
    Op("buffer_add", "counted", _through_flat("buffer"), buffer=True),
    Op("view_add", "counted", _through_flat("view"), buffer=True),
    Op("half_float", "rehomed", half_float, only=F32),
    Op("double_float", "rehomed", double_float, only=F32),
    Op("vec_to_params", "rehomed", vec_to_params, only=F32 + ("bf16",)),
    Op("set_", "rehomed", set_),
    Op("data_assign", "rehomed", data_assign),
    Op("data_add", "silent", data_add),
    Op("data_index", "silent", data_index),
    Op("data_pair", "silent", data_pair),
    Op("foreach_data", "silent", foreach_data),
    Op("clip_only", "none", clip_only),
    Op("freeze", "none", freeze),
)}


def blocking(op):
    """Must the next update_send copy the parameters in full?"""
    return op.steps or op.cls in ("counted", "rehomed", "replaced")


def run_op(op, net, flat, seed):
    """The op on `net` (a learner's module with its FlatParameters, or a twin with None)."""
    op.fn(net, flat, np.random.default_rng(seed))


def observe(op, net, flat, seed):
    """Runs `op` on a module under a FlatParameters and returns the class seen the way the adapter can
    see it: 'replaced' when the module holds another object than `flat.params`, else 'rehomed' when a
    ``data_ptr`` moved, else 'counted' when a parameter's or the buffer's ``_version`` moved, else
    'silent' when a value changed, else 'none'."""
    held = list(flat.params)
    versions = [p._version for p in held] + [flat.buffer._version]
    ptrs = [p.data_ptr() for p in held]
    before = module_bytes(net, Layout(net))
    run_op(op, net, flat, seed)
    now = params(net)
    if len(now) != len(held) or any(a is not b for a, b in zip(now, held)):
        return "replaced"
    if [p.data_ptr() for p in held] != ptrs:
        return "rehomed"
    if [p._version for p in held] + [flat.buffer._version] != versions:
        return "counted"
    return "none" if np.array_equal(before, module_bytes(net, Layout(net))) else "silent"


# ---------------------------------------------------------------------------------- the decision
FORMS = {  # name -> the adapter's keyword arguments, update_wait_many
    "default": (dict(write_through=True, reuse_guard=True), False),
    "noguard": (dict(write_through=True, reuse_guard=False), False),
    "plain": (dict(write_through=False), False),
    "resident": (dict(resident=True), False),
    "many": (dict(write_through=True, reuse_guard=True), True),
}
WRITE_THROUGH = ("default", "noguard", "many")

MUTANTS = ("first-parameter-versions", "no-buffer-counter", "rehome-keeps-reuse", "reuse-after-no-average",
           "guard-hit-copies-all", "fused-step-is-none", "replaced-object-kept", "gaps-from-parameters")


class Learner:
    """One learner: its twin and what the adapter must publish for it."""

    def __init__(self, model, seed, form, method, value=0.5, device="cpu", mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.model, self.form, self.method, self.value, self.mutant = model, form, method, value, mutant
        self.twin = build(model, seed).to(device)
        self.lay = Layout(self.twin)
        self.write_through = form in WRITE_THROUGH
        self.guard = FORMS[form][0].get("reuse_guard", False) and self.write_through
        self.resident = form == "resident"
        self.version, self.clock, self.hits = 0, 0, 0
        self.averaged = False           # the previous update_wait averaged
        self.since = set()              # what the ops since then were seen as
        self.snapshot = None            # the payload the last average wrote through
        self.served = None              # ((clock, loss, version, n, dtype), payload) of the last publish
        self.reuse = None               # the reuse_snapshot the last update_send must have passed
        self.kept = None                # mutant replaced-object-kept: the bytes the orphans hold
        self.silent = False             # a silent write since the last publish or average (coverage)

    def seen(self, op):
        """What the (possibly mutated) adapter takes `op` for: a set of marks."""
        m = self.mutant
        marks = {op.cls}
        if op.steps:
            marks.add("step")
        if m == "first-parameter-versions" and op.cls == "counted" and not op.first and not op.buffer:
            marks = {"silent"} | (marks & {"step"})
        if m == "no-buffer-counter" and op.buffer:
            marks = {"silent"}
        if m == "rehome-keeps-reuse" and op.cls == "rehomed":
            marks = {"silent"}
        if m == "fused-step-is-none" and op.fused:
            marks = {op.cls}
        if m == "replaced-object-kept" and op.cls == "replaced":
            marks = {"none"}
        return marks

    def op(self, op, seed):
        if self.mutant == "replaced-object-kept" and op.cls == "replaced" and self.kept is None:
            self.kept = module_bytes(self.twin, self.lay)
        run_op(op, self.twin, None, seed)
        self.since |= self.seen(op)
        if op.cls == "silent":
            self.silent = True

    def current(self):
        cur = module_bytes(self.twin, self.lay)
        if self.kept is not None:
            cur = self.kept
        if self.mutant == "gaps-from-parameters":
            gaps = self.lay.gaps()
            cur = cur.copy()
            cur[gaps] = np.resize(cur[~gaps], int(gaps.sum())) if (~gaps).any() else 0
        return cur

    def send(self, loss):
        """update_send: returns (reuse_snapshot, header, payload, guard hit, silent write pending)."""
        cur = self.current()
        gen = self.version + 1                  # learner.cpp publish_impl: the version being published
        self.clock += 1
        averaged = self.averaged or (self.mutant == "reuse-after-no-average" and self.snapshot is not None)
        hit = False
        if self.resident:
            reuse, payload, ahead = False, cur, self.averaged
        else:
            reuse = self.write_through and averaged and not (self.since & {"counted", "rehomed", "replaced", "step"})
            really = reuse and self.averaged    # the learner reuses only a snapshot an average wrote
            ahead = really
            if not really:
                payload = cur
            elif self.guard:
                payload, hit = moves_ref.guard_expected(self.snapshot, cur, gen)
                if hit and self.mutant == "guard-hit-copies-all":
                    payload = cur
                self.hits += int(hit)
            else:
                payload = self.snapshot
        # a header written ahead by the average (constant and clock interpolation) carries no loss yet
        header = (float(self.clock), math.nan if ahead else float(loss), gen, self.lay.n, self.lay.code)
        pending = self.silent
        self.version, self.reuse, self.served = gen, reuse, (header, payload.copy())
        self.averaged, self.since, self.silent, self.kept = False, set(), False, None
        return reuse, header, payload, hit, pending

    def wait(self, loss, peer):
        """update_wait: `peer` is the other learner's ``served`` (None: the fetch brought nothing)."""
        if peer is None:
            return False
        (peer_clock, peer_loss, _, _, _), payload = peer
        factor, clock = policy.factor_and_clock(self.method, self.value, 0.0, self.clock, peer_clock, loss,
                                                peer_loss)
        new = average(self.lay, module_bytes(self.twin, self.lay), payload, factor)
        bind_bytes(self.twin, self.lay, new)
        self.clock = clock
        self.snapshot, self.averaged, self.since, self.silent = new, True, set(), False
        return True


# ---------------------------------------------------------------------------------- walks
class Walk:
    def __init__(self, model, form, method, seed, rounds=40):
        self.model, self.form, self.method, self.seed, self.rounds = model, form, method, seed, rounds

    @property
    def name(self):
        return "%s-%s-%s-s%d" % (self.model, self.form, self.method, self.seed)


WALKS = tuple(Walk(model, form, "clock" if (i + j) % 4 == 3 else "constant", 100 * i + j + 7)
              for i, model in enumerate(MODELS) for j, form in enumerate(FORMS))
P_DOWN = 0.08           # a round for which a learner has no peer (remove_peer, add_peer after it): no average


def script(walk):
    """The walk's events, drawn from its seed:
    ("op", round, learner, op name, seed), ("send", round, learner, loss),
    ("down", round, learner, bool: its peer is removed before the round's update_send and added again
    after its update_wait), ("wait", round, learner, loss) or ("wait_many", round, (losses)).
    Before each update_send zero to two ops (half of them ops that leave a snapshot reusable); between
    update_send and update_wait, where the reference's loop trains, usually one -- none for the
    resident form, whose parameters are the served snapshot there."""
    rng = np.random.default_rng(walk.seed)
    able = [op for op in OPS.values() if op.applies(walk.model)]
    quiet = [op.name for op in able if not blocking(op)]
    loud = [op.name for op in able if blocking(op)]
    events = []

    def draw(r, g, names):
        events.append(("op", r, g, names[int(rng.integers(len(names)))], int(rng.integers(1 << 31))))

    for r in range(walk.rounds):
        for g in (0, 1):
            for _ in range(int(rng.choice(3, p=(0.35, 0.45, 0.2)))):
                draw(r, g, quiet if rng.random() < 0.5 else loud)
        down = [bool(rng.random() < P_DOWN) for _ in (0, 1)]
        for g in (0, 1):
            if down[g]:
                events.append(("down", r, g, True))
        for g in (0, 1):
            events.append(("send", r, g, round(float(rng.uniform(0.5, 2.0)), 3)))
        if walk.form != "resident":
            for g in (0, 1):
                if rng.random() < 0.8:
                    draw(r, g, [op.name for op in able])
        losses = tuple(round(float(rng.uniform(0.5, 2.0)), 3) for _ in (0, 1))
        if FORMS[walk.form][1]:
            events.append(("wait_many", r, losses))
        else:
            for g in (0, 1):
                events.append(("wait", r, g, losses[g]))
        for g in (0, 1):
            if down[g]:
                events.append(("down", r, g, False))
    return events


def _rounds(pre=(), mid=(), rounds=1, start=0, down=()):
    """`rounds` rounds of both learners: the ops of `pre` before update_send, of `mid` after it."""
    events = []
    for r in range(start, start + rounds):
        for g in (0, 1):
            events += [("op", r, g, name, 1000 * r + 10 * g + k) for k, name in enumerate(pre)]
        events += [("down", r, g, True) for g in down]
        events += [("send", r, g, 1.0 + 0.125 * g) for g in (0, 1)]
        for g in (0, 1):
            events += [("op", r, g, name, 1000 * r + 10 * g + 5 + k) for k, name in enumerate(mid)]
        events += [("wait", r, g, 0.75 + 0.125 * g) for g in (0, 1)]
        events += [("down", r, g, False) for g in down]
    return events


@functools.lru_cache(maxsize=None)
def directed():
    """name -> (Walk, events).  All on `chunky`; the steps of the two findings have a gradient on the
    64-element tensor only."""
    out = {}
    for form in ("default", "noguard"):
        for opt in ("sgd", "adam", "adamw"):
            # finding 1: a fused step after the average, before the publish, round after round
            w = Walk("chunky", form, "constant", 11, rounds=6)
            out["fused-%s-%s" % (opt, form)] = (w, _rounds(mid=[opt + "_fused"]) +
                                                _rounds(pre=[opt + "_fused_small"], rounds=5, start=1))
        for how in ("load_sd_assign", "attr_replace"):
            # finding 2: the optimizer exists, the parameter is replaced, a step, two rounds
            w = Walk("chunky", form, "constant", 12, rounds=4)
            out["%s-%s" % (how, form)] = (w, _rounds(mid=["sgd_single"]) +
                                          _rounds(pre=[how, "sgd_one_small"], start=1) +
                                          _rounds(rounds=2, start=2))
        w = Walk("chunky", form, "constant", 13, rounds=4)
        out["fused-after-no-average-%s" % form] = (w, _rounds() + _rounds(down=(0, 1), start=1) +
                                                   _rounds(pre=["adamw_fused_small"], start=2) + _rounds(start=3))
        w = Walk("chunky", form, "constant", 14, rounds=3)
        out["silent-then-counted-%s" % form] = (w, _rounds() + _rounds(pre=["data_add", "nograd_add"], start=1) +
                                                _rounds(start=2))
        w = Walk("chunky", form, "constant", 15, rounds=3)
        out["half-float-%s" % form] = (w, _rounds() + _rounds(pre=["half_float"], start=1) + _rounds(start=2))
        w = Walk("chunky", form, "constant", 16, rounds=3)
        out["replaced-in-the-window-%s" % form] = (w, _rounds() + _rounds(mid=["attr_replace"], start=1) +
                                                   _rounds(start=2))
    return out


def chunky_geometry():
    """Where `chunky`'s 64 trained elements lie among the guard's chunks.  The flat buffer starts every
    tensor on a 256-byte boundary: the 6,000-element tensor ends in word 1,499, the 64-element one
    begins in word 1,504, which is where chunk 535 begins -- the two share no chunk.  Its other end does:
    chunk 540 holds the tensor's last two words and the first word of the 40,000-element tensor, which
    the directed steps do not train either.  Returns (that chunk, its words, the small tensor's words)."""
    lay = Layout(build("chunky", 0))
    n16 = lay.nbytes // 16
    small = lay.ranges[1]
    words = range(small[2] // 16, (small[2] + small[3]) // 16)
    chunk, (lo, hi) = guard_chunk(n16, words[-1])
    assert guard_period(n16) == 3
    return chunk, (lo, hi), words, lay.ranges[2][2] // 16


# ---------------------------------------------------------------------------------- replay on the host
def run_host(walk, events, mutant=None, on_send=None, on_wait=None):
    """Replays `events` on two model learners; returns the rows
    (round, learner, reuse, header, payload, guard hit, silent pending, hits, clock) of every publish."""
    L = [Learner(walk.model, walk.seed + g, walk.form, walk.method, mutant=mutant) for g in (0, 1)]
    down = [False, False]
    rows = []
    for ev in events:
        kind, r = ev[0], ev[1]
        if kind == "op":
            L[ev[2]].op(OPS[ev[3]], ev[4])
        elif kind == "send":
            g = ev[2]
            reuse, header, payload, hit, pending = L[g].send(ev[3])
            rows.append((r, g, reuse, header, payload, hit, pending, L[g].hits, None))
        elif kind == "down":
            down[ev[2]] = ev[3]
        else:
            waits = [(ev[2], ev[3])] if kind == "wait" else list(enumerate(ev[2]))
            for g, loss in waits:
                L[g].wait(loss, None if down[g] else L[1 - g].served)
                rows.append((r, g, None, None, module_bytes(L[g].twin, L[g].lay), None, None, L[g].hits, L[g].clock))
    return rows


def first_difference(walk, events, mutant):
    """(round, learner, what) of the first row at which `mutant` differs from the model, or None."""
    for a, b in zip(run_host(walk, events), run_host(walk, events, mutant)):
        for what, x, y in (("reuse", a[2], b[2]), ("payload", a[4].tobytes(), b[4].tobytes()), ("hits", a[7], b[7])):
            if x != y:
                if what == "payload":
                    what = "payload byte %d" % int(np.flatnonzero(a[4] != b[4])[0])
                return a[0], a[1], ("publish " if a[2] is not None else "parameters after update_wait ") + what
    return None
