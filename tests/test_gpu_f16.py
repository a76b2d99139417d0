"""float16 parameters on the GPU: every form of the averaging kernel (host / device coefficients,
the element-wise kernel for unaligned views, the fused average plain and write-through, the
batched, pair and group dispatches of resident learners) and the adapter end to end on a
``.half()`` model, against torch-CPU eager on ``torch.float16`` (tests/f16_ref.py: the expected
values are computed on the host, never by the library or by torch on the device).

Bar: NaN positions coincide, every other element bit-equal -- subnormals, signed zeros and
infinities included.  All shapes are tiny: a one-wave span holds 512 fp16 elements, a 16-byte item
eight, so every path (vector body, ragged tail of 1-7, empty last span, several spans) is reached
below 70,000 elements."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dpwa_amd import DpwaPyTorchAdapter, _lib
from dpwa_amd.group import LocalGroup
from dpwa_amd.learner import Learner
from oracle import policy as opolicy
from tests import f16_ref as ref
from tests.test_gpu_kernels import average_slot, coef_block, ptr, stream
from tests.test_gpu_self_peer import write_self_cfg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OFF = _lib.SLOT_PAYLOAD_OFFSET


def dev(u16):
    return ref.as_half(u16).to(DEV)


def check(got, want, what=None):
    got = ref.as_u16(got) if isinstance(got, torch.Tensor) else got
    assert ref.same(got, want), (what, ref.mismatches(got, want))


def host_lerp(param, peer, f):
    _lib.call("dpwa_lerp_f16_host", ptr(param), ptr(peer), param.numel(), float(f), stream())


def dev_lerp(param, peer, f):
    coef = coef_block(f)
    _lib.call("dpwa_lerp_f16", ptr(param), ptr(peer), param.numel(), ptr(coef), stream())


@functools.lru_cache(maxsize=None)
def every_pattern_expected(f):
    return ref.torch_lerp(ref.PERM, ref.PATTERNS, f)


# ---------------------------------------------------------------- 1. every bit pattern
@pytest.mark.parametrize("f", ref.FACTORS)
def test_every_bit_pattern(f):
    """Peer: all 65,536 fp16 bit patterns; parameters: a fixed permutation of them (+inf meets
    +inf, -0 meets -0); nine factors, the last two overflowing to inf and producing inf - inf.
    Through dpwa_lerp_f16_host and through dpwa_lerp_f16 with dpwa_factor's coefficient block."""
    want = every_pattern_expected(f)
    q = dev(ref.PATTERNS)
    for lerp in (host_lerp, dev_lerp):
        p = dev(ref.PERM)
        lerp(p, q, f)
        torch.cuda.synchronize()
        check(p, want, lerp.__name__)
    check(q, ref.PATTERNS, "the peer is only read")


# ---------------------------------------------------------------- 2. ragged sizes
@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 511, 512, 513, 4099, 65_549])
def test_ragged_sizes(n):
    """Tails of 1-7 elements behind 0, 1, 2 or many 16-byte items, one full span (whose grid has
    an empty last span), one element over, several spans.  The sample puts signed zeros and
    subnormals into the tail as into the body; the last element is -0 meeting -0 (a product of
    exact -0, which a +0 addend would turn into +0).  The elements behind the n are untouched."""
    pad = 24
    p_u, q_u = ref.sample(n + pad, 4 * n)
    if n:
        p_u[n - 1] = q_u[n - 1] = ref.NEG_ZERO
    for f in (0.3, 0.0):
        want = p_u.copy()
        want[:n] = ref.torch_lerp(p_u[:n], q_u[:n], f)
        for lerp in (host_lerp, dev_lerp):
            base, q = dev(p_u), dev(q_u)
            lerp(base[:n], q[:n], f)
            torch.cuda.synchronize()
            check(base, want, (f, lerp.__name__))


# ---------------------------------------------------------------- 3. unaligned views
@pytest.mark.parametrize("off_p,off_q", [(1, 0), (0, 3), (2, 2), (1, 2), (7, 5)])
def test_unaligned_views(off_p, off_q):
    """Views at odd element offsets (2-byte steps off the 16-byte alignment) take the element-wise
    kernel; nothing outside the view changes."""
    n = 10_007
    p_u, q_u = ref.sample(n + 8, 4 * (off_p * 10 + off_q))
    f = 0.3
    want = p_u.copy()
    want[off_p:off_p + n] = ref.torch_lerp(p_u[off_p:off_p + n], q_u[off_q:off_q + n], f)
    for lerp in (host_lerp, dev_lerp):
        base_p, base_q = dev(p_u), dev(q_u)
        lerp(base_p[off_p:off_p + n], base_q[off_q:off_q + n], f)
        torch.cuda.synchronize()
        check(base_p, want, lerp.__name__)
        check(base_q, q_u)


# ---------------------------------------------------------------- 4. fused average
# (method, constant value, divergence threshold, my clock, peer clock, loss, peer loss)
FUSED = [
    ("constant", 0.3, 0.0, 3.0, 7.0, 1.0, 1.0),
    ("clock", None, 0.0, 3.0, 7.0, 1.0, 1.0),
    ("loss", None, 0.0, 3.0, 7.0, 0.75, 1.5),
    ("clock", None, 2.0, 5.0, 2.0, 0.5, 1.0),      # loss < threshold: the factor is scaled by loss / threshold
    ("loss", None, 3.0, 1.0, 4.0, 1.25, 0.5),
]


def average(dtype, p, slot, n, case, snap):
    method, value, thr, my_clock, _, loss, _ = case
    clock = torch.tensor([my_clock, -1.0], dtype=torch.float64, device=DEV)
    coef = torch.zeros(32, dtype=torch.uint8, device=DEV)
    cfg = _lib.Interp(opolicy.METHODS[method], 0, float(value or 0.0), float(thr))
    _lib.call("dpwa_average", dtype, ptr(p), ptr(slot), n, ctypes.byref(cfg), ptr(clock), float(loss), ptr(coef),
              ptr(snap) if snap is not None else None, stream(), None, None)
    torch.cuda.synchronize()
    return _lib.Coef.from_buffer_copy(coef.cpu().numpy().tobytes()), clock[1].item()


@pytest.mark.parametrize("n", [5, 512, 1541])
@pytest.mark.parametrize("write_through", [False, True])
def test_fused_average(n, write_through):
    """dpwa_average(DPWA_F16) -- device factor + lerp (+ the next snapshot) -- at a tail alone, one
    span and three spans with a tail of 5: constant, clock and loss interpolation and a divergence
    threshold; the new clock and dpwa_coef against the oracle policy, the write-through copy equal
    to the averaged parameters."""
    p_u, q_u = ref.sample(n, 4 * n)
    p_u[n - 1] = q_u[n - 1] = ref.NEG_ZERO
    for case in FUSED:
        method, value, thr, my_clock, peer_clock, loss, peer_loss = case
        f, new_clock = opolicy.factor_and_clock(method, value, thr, my_clock, peer_clock, loss, peer_loss)
        want = ref.torch_lerp(p_u, q_u, f)
        p = dev(p_u)
        slot = average_slot(dev(q_u), peer_clock, peer_loss)
        snap = torch.full_like(p, float("nan")) if write_through else None
        c, got_clock = average(_lib.F16, p, slot, n, case, snap)
        check(p, want, case)
        assert c.status == 0 and c.factor == f, case
        assert c.a == np.float32(f) and c.b == np.float32(1.0 - f), case
        assert got_clock == new_clock == c.new_clock, case          # dpwa.py:150
        if write_through:
            assert np.array_equal(ref.as_u16(snap), ref.as_u16(p)), case
        check(slot[OFF:].view(torch.float16), q_u, "the peer's slot is only read")


@pytest.mark.parametrize("n", [5, 512, 1541])
def test_fused_average_zero_division(n):
    """Clock interpolation with both clocks 0 (the reference's ZeroDivisionError,
    interpolation.py:22-24): the parameters and the clock stay, the write-through snapshot
    receives the unchanged parameters, ragged tail included."""
    p_u, q_u = ref.sample(n, 4 * n + 1)
    for write_through in (False, True):
        p = dev(p_u)
        slot = average_slot(dev(q_u), 0.0, 1.0)
        snap = torch.zeros_like(p) if write_through else None
        c, got_clock = average(_lib.F16, p, slot, n, ("clock", None, 0.0, 0.0, 0.0, 1.0, 1.0), snap)
        assert c.status == _lib.STATUS_ZERO_DIVISION
        assert got_clock == 0.0
        assert np.array_equal(ref.as_u16(p), p_u)
        if write_through:
            assert np.array_equal(ref.as_u16(snap), p_u)


# ---------------------------------------------------------------- 5. batched forms
def alone(p_u, q_u, case):
    """The same average through dpwa_average, by itself."""
    p = dev(p_u)
    average(_lib.F16, p, average_slot(dev(q_u), case[4], case[6]), len(p_u), case, None)
    return ref.as_u16(p)


@pytest.mark.parametrize("sizes", [(1541, 5), (512, 1541, 5)])
@pytest.mark.parametrize("write_through", [False, True])
def test_average_many(sizes, write_through):
    """dpwa_average_many over 2 and 3 descriptors of different sizes (clock interpolation, each
    entry its own clocks): each entry bit-equal to torch-CPU eager and to the same average done
    alone, clocks and coefficient blocks written, write-through copies equal to the parameters."""
    ents = []
    for i, n in enumerate(sizes):
        p_u, q_u = ref.sample(n, 4 * (n + i))
        case = ("clock", None, 0.0, float(i + 1), float(3 * i + 2), 0.5 + 0.1 * i, 0.25 + 0.2 * i)
        p = dev(p_u)
        ents.append(dict(n=n, p_u=p_u, q_u=q_u, case=case, p=p, slot=average_slot(dev(q_u), case[4], case[6]),
                         snap=torch.full_like(p, float("nan")) if write_through else None,
                         clock=torch.tensor([case[3], -1.0], dtype=torch.float64, device=DEV),
                         coef=torch.zeros(32, dtype=torch.uint8, device=DEV)))
    d = (_lib.AverageDesc * len(ents))()
    for j, e in enumerate(ents):
        d[j] = _lib.AverageDesc(e["p"].data_ptr(), e["slot"].data_ptr(), e["n"], e["clock"].data_ptr(), e["case"][5],
                                e["coef"].data_ptr(), e["snap"].data_ptr() if write_through else None)
    cfg = _lib.Interp(_lib.INTERP_CLOCK, 0, 0.0, 0.0)
    _lib.call("dpwa_average_many", _lib.F16, d, len(ents), ctypes.byref(cfg), stream(), None, None)
    torch.cuda.synchronize()
    for i, e in enumerate(ents):
        case = e["case"]
        f, new_clock = opolicy.factor_and_clock("clock", None, 0.0, case[3], case[4], case[5], case[6])
        check(e["p"], ref.torch_lerp(e["p_u"], e["q_u"], f), i)
        assert np.array_equal(ref.as_u16(e["p"]), alone(e["p_u"], e["q_u"], case)), i
        c = _lib.Coef.from_buffer_copy(e["coef"].cpu().numpy().tobytes())
        assert c.status == 0 and c.factor == f and e["clock"][1].item() == new_clock, i
        if write_through:
            assert np.array_equal(ref.as_u16(e["snap"]), ref.as_u16(e["p"])), i


class Resident:
    """A resident learner as the batch sees it (tests/test_gpu_pairs.py): its published slot
    (header + parameters), its next slot, its clock pair and coefficient block."""

    def __init__(self, n, seed, clock, loss):
        self.n, self.clock_val, self.loss = n, clock, loss
        self.host, _ = ref.sample(n, seed)
        self.slot = average_slot(dev(self.host), clock, loss)
        self.next = torch.full((OFF + 2 * n,), 0x7f, dtype=torch.uint8, device=DEV)
        self.clock = torch.tensor([clock, -1.0], dtype=torch.float64, device=DEV)
        self.coef = torch.zeros(32, dtype=torch.uint8, device=DEV)


RESIDENT = {
    "one": [(0, 1)],                          # the single kernel, out of place
    "two-apart": [(0, 1), (2, 3)],            # k_lerp_batch, out of place: no read is shared
    "mutual-pair": [(0, 1), (1, 0)],          # k_lerp_pair
    "three-sharing": [(0, 1), (1, 0), (2, 0)],   # k_lerp_group: slot 0 is read by all three
}


@pytest.mark.parametrize("name", sorted(RESIDENT))
@pytest.mark.parametrize("n", [5, 1541])
def test_average_many_resident(name, n):
    """dpwa_average_many_resident with one descriptor, two that share nothing (the batch kernel), a
    mutual pair (the pair kernel) and a group of three sharing reads: every average lands in the entry's next slot, bit-equal to torch-CPU
    eager and to the same average done alone; the published slots are only read."""
    picks = RESIDENT[name]
    ls = [Resident(n, 4 * (n + 7 * i), 1.0 + 0.5 * i, 0.2 + 0.1 * i) for i in range(4)]
    losses = [0.5 + 0.1 * j for j in range(len(picks))]
    d = (_lib.AverageDesc * len(picks))()
    for j, ((a, b), loss) in enumerate(zip(picks, losses)):
        me, peer = ls[a], ls[b]
        d[j] = _lib.AverageDesc(me.slot.data_ptr() + OFF, peer.slot.data_ptr(), n, me.clock.data_ptr(), loss,
                                me.coef.data_ptr(), me.next.data_ptr() + OFF)
    before = [lr.slot.clone() for lr in ls]
    cfg = _lib.Interp(_lib.INTERP_CLOCK, 0, 0.0, 0.0)
    _lib.call("dpwa_average_many_resident", _lib.F16, d, len(picks), ctypes.byref(cfg), stream(), None, None)
    torch.cuda.synchronize()
    for lr, b in zip(ls, before):
        assert torch.equal(lr.slot, b)
    for (a, b), loss in zip(picks, losses):
        me, peer = ls[a], ls[b]
        f, new_clock = opolicy.factor_and_clock("clock", None, 0.0, me.clock_val, peer.clock_val, loss, peer.loss)
        got = me.next[OFF:].cpu().numpy().view(np.uint16)
        check(got, ref.torch_lerp(me.host, peer.host, f), (name, a, b))
        case = ("clock", None, 0.0, me.clock_val, peer.clock_val, loss, peer.loss)
        assert np.array_equal(got, alone(me.host, peer.host, case)), (name, a, b)
        c = _lib.Coef.from_buffer_copy(me.coef.cpu().numpy().tobytes())
        assert c.status == 0 and c.factor == f and me.clock[1].item() == new_clock


# ---------------------------------------------------------------- 6. the adapter end to end
@pytest.mark.parametrize("form", ["write-through", "plain", "resident"])
def test_adapter_on_a_half_model(tmp_path, form):
    """DpwaPyTorchAdapter on a ``.half()`` model whose peer is its own snapshot (the YAML of
    tests/test_gpu_self_peer.py), four rounds of loss interpolation: the default write-through
    form and write_through=False in the reference order (update_send, step, update_wait), the
    resident form in its own (update_send, update_wait, step).  The step writes every parameter
    through a versioned op (``copy_``).  After every update_wait the parameters equal the
    torch-CPU recomputation and the clock the oracle policy's."""
    cfg = tmp_path / "half.yaml"
    write_self_cfg(cfg, 1.0, "loss", 0.0, None)
    g = torch.Generator().manual_seed(6)
    net = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.Linear(17, 5))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    net = net.half().to(DEV)
    host = [p.detach().cpu().clone() for p in net.parameters()]          # the CPU recomputation
    kwargs = {"write-through": {}, "plain": {"write_through": False}, "resident": {"resident": True}}[form]
    ad = DpwaPyTorchAdapter(net, "w1", str(cfg), seed=3, group=LocalGroup(), **kwargs)
    resident = form == "resident"
    clock = 0

    def step():
        with torch.no_grad():
            for k, p in enumerate(net.parameters()):
                host[k] = host[k] + (0.05 * torch.randn(p.shape, generator=g)).half()
                p.copy_(host[k])

    for r in range(4):
        send_loss, wait_loss = 1.0 + 0.25 * r, 0.5 + 0.125 * r
        ad.update_send(send_loss)
        clock += 1                                                       # dpwa.py:112
        snap = [h.clone() for h in host]
        if not resident:
            step()
        ad.update_wait(wait_loss)
        f, new_clock = opolicy.factor_and_clock("loss", None, 0.0, clock, clock, wait_loss, send_loss)
        for k, p in enumerate(net.parameters()):
            assert p.dtype == torch.float16 and p.device == DEV
            want = ref.torch_lerp(ref.as_u16(host[k]).reshape(-1), ref.as_u16(snap[k]).reshape(-1), f)
            host[k] = ref.as_half(want).view(host[k].shape)
            check(ref.as_u16(p).reshape(-1), want, (form, r, k))
        assert ad.connection.clock == new_clock, (form, r)
        assert float(ad.connection._learner.read_coef().factor) == f, (form, r)
        clock = new_clock
        if resident:
            step()
    if resident:
        home = ad.connection.parameters
        p0 = next(net.parameters())
        assert home.dtype == torch.float16
        assert home.data_ptr() <= p0.data_ptr() < home.data_ptr() + 2 * home.numel()
    ad.connection.close()


# ---------------------------------------------------------------- 7. the dtype is the only guard
def test_float16_and_bfloat16_learners_do_not_attach():
    """fp16 and bf16 elements have the same size, so only the dtype code keeps a float16 learner
    from averaging a bfloat16 peer's bits: attaching one to the other fails with DPWA_ERR_ARG
    naming both dtype codes, in either direction, and neither learner's parameters change."""
    n = 1541
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    half = Learner(DEV, n, torch.float16, cfg)
    bf = Learner(DEV, n, torch.bfloat16, cfg)
    p_u, q_u = ref.sample(n, 28)
    p_half = dev(p_u)
    p_bf = torch.from_numpy(q_u.view(np.int16).copy()).view(torch.bfloat16).to(DEV)
    s = torch.cuda.current_stream()
    half.publish(p_half, 1.0, s)
    bf.publish(p_bf, 1.0, s)
    for me, other, mine, theirs in ((half, bf, _lib.F16, _lib.BF16), (bf, half, _lib.BF16, _lib.F16)):
        with pytest.raises(_lib.DpwaError) as err:
            me.attach_local(0, other)
        assert err.value.code == _lib.ERR_ARG
        assert "of dtype %d" % theirs in str(err.value) and "of %d" % mine in str(err.value), str(err.value)
    same = Learner(DEV, n, torch.float16, cfg)
    half.attach_local(0, same)                                            # float16 to float16 attaches
    torch.cuda.synchronize()
    assert np.array_equal(ref.as_u16(p_half), p_u)
    assert np.array_equal(p_bf.view(torch.int16).cpu().numpy().view(np.uint16), q_u)
    for lr in (half, bf, same):
        lr.close()
