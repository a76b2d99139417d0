"""Mixed-dtype (segmented) payloads on the GPU: the averaging kernel through dpwa_average_mixed
(plain and write-through, the no-op round, the single commit), a learner through the split
factor-then-lerp path, and DpwaPyTorchAdapter on models with fp32 norms in a bf16 or fp16 body in
its three forms, alone (self-peer) and as two co-resident learners -- every averaged segment and
parameter against the host reference of its dtype (tests/mixed_ref.py: oracle.lerp for float32 and
bfloat16, torch-CPU eager for float16, and torch-CPU eager tensor by tensor end to end; never the
library or torch on the device).  Then what is refused, and a one-segment layout against the
single-dtype entries (average, finite check, distance).

Bar: bit-equal, NaN positions coinciding.  All shapes are tiny: a segment is at most three 4-KiB
blocks, i.e. twelve one-wave spans."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dpwa_amd import DpwaConnection, DpwaPyTorchAdapter, _lib
from dpwa_amd.flat import c_layout
from dpwa_amd.group import LocalGroup
from dpwa_amd.learner import Learner
from oracle import policy as opolicy
from tests import dist_ref
from tests import mixed_ref as ref
from tests.test_gpu_distance import check_record, fresh_record, read_record, workspace
from tests.test_gpu_f16 import FUSED
from tests.test_gpu_kernels import average_slot, ptr, stream
from tests.test_gpu_self_peer import write_self_cfg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OFF = _lib.SLOT_PAYLOAD_OFFSET
GUARD = 1024               # bytes behind a payload that no kernel may touch


def layout_of(spec):
    segs, total = ref.segments(spec)
    return tuple((ref.TORCH[d], off, length) for d, off, length, _ in segs), total


def tens(host_bytes):
    """A CPU tensor over a copy (the shared expected arrays are read-only)."""
    return torch.from_numpy(np.array(host_bytes))


def on_device(host_bytes):
    """A payload on the device with GUARD bytes of 0x7f behind it; returns (payload view, whole)."""
    whole = torch.full((host_bytes.size + GUARD,), 0x7f, dtype=torch.uint8, device=DEV)
    whole[:host_bytes.size].copy_(tens(host_bytes))
    return whole[:host_bytes.size], whole


def guard_intact(whole):
    return bool((whole[-GUARD:] == 0x7f).all())


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def payloads(name):
    """(param bytes, peer bytes) of a kernel-test layout, made once."""
    p, q = ref.sample(ref.LAYOUTS[name], 11 + len(name))
    p.setflags(write=False)
    q.setflags(write=False)
    return p, q


@functools.lru_cache(maxsize=None)
def expected(name, f):
    """The host references' average of payloads(name) at factor f, computed once and shared."""
    p, q = payloads(name)
    want = ref.lerp(ref.LAYOUTS[name], p, q, f)
    want.setflags(write=False)
    return want


def average_mixed(lay, p, slot, case, snap):
    method, value, thr, my_clock, _, loss, _ = case
    clock = torch.tensor([my_clock, -1.0], dtype=torch.float64, device=DEV)
    coef = torch.zeros(32, dtype=torch.uint8, device=DEV)
    cfg = _lib.Interp(opolicy.METHODS[method], 0, float(value or 0.0), float(thr))
    _lib.call("dpwa_average_mixed", ctypes.byref(c_layout(lay)), ptr(p), ptr(slot), ctypes.byref(cfg), ptr(clock),
              float(loss), ptr(coef), ptr(snap) if snap is not None else None, stream(), None, None)
    torch.cuda.synchronize()
    return _lib.Coef.from_buffer_copy(coef.cpu().numpy().tobytes()), clock[1].item()


# ---------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("name", sorted(ref.LAYOUTS))
@pytest.mark.parametrize("write_through", [False, True])
def test_average_mixed(name, write_through):
    """dpwa_average_mixed over {f32: 1, bf16: 1}, {f32: exactly one block, bf16: a block and one
    element, f16: 5} and {f32: 3, f16: 4097}: constant, clock and loss interpolation and two
    divergence thresholds.  Every segment equals its dtype's host reference (hard values in its
    first and last 16-byte word), the padding stays zero, the clock and dpwa_coef are the oracle
    policy's, the write-through copy equals the parameters, the peer's slot and the bytes behind
    the payloads are untouched."""
    spec = ref.LAYOUTS[name]
    lay, total = layout_of(spec)
    p_h, q_h = payloads(name)
    for case in FUSED:
        method, value, thr, my_clock, peer_clock, loss, peer_loss = case
        f, new_clock = opolicy.factor_and_clock(method, value, thr, my_clock, peer_clock, loss, peer_loss)
        want = expected(name, f)
        p, p_whole = on_device(p_h)
        slot = average_slot(tens(q_h).to(DEV), peer_clock, peer_loss)
        snap, snap_whole = on_device(np.full(total, 0x55, dtype=np.uint8)) if write_through else (None, None)
        c, got_clock = average_mixed(lay, p, slot, case, snap)
        assert ref.same(spec, host(p), want) is None, (case, ref.same(spec, host(p), want))
        assert c.status == 0 and c.factor == f, case
        assert c.a == np.float32(f) and c.b == np.float32(1.0 - f), case
        assert got_clock == new_clock == c.new_clock, case          # dpwa.py:150
        assert guard_intact(p_whole), case
        if write_through:
            assert torch.equal(snap, p) and guard_intact(snap_whole), case
        assert np.array_equal(host(slot[OFF:]), q_h), "the peer's slot is only read"


@pytest.mark.parametrize("write_through", [False, True])
def test_average_mixed_zero_division_is_a_noop(write_through):
    """Clock interpolation with both clocks 0 (the reference's ZeroDivisionError,
    interpolation.py:22-24): the parameters and the clock stay, the status says so, and the
    write-through snapshot still receives the unchanged parameters, all three segments of them."""
    lay, total = layout_of(ref.LAYOUTS["abutting"])
    p_h, q_h = payloads("abutting")
    p, p_whole = on_device(p_h)
    slot = average_slot(tens(q_h).to(DEV), 0.0, 1.0)
    snap, snap_whole = on_device(np.full(total, 0x55, dtype=np.uint8)) if write_through else (None, None)
    c, got_clock = average_mixed(lay, p, slot, ("clock", None, 0.0, 0.0, 0.0, 1.0, 1.0), snap)
    assert c.status == _lib.STATUS_ZERO_DIVISION and got_clock == 0.0
    assert np.array_equal(host(p), p_h) and guard_intact(p_whole)
    if write_through:
        assert np.array_equal(host(snap), p_h) and guard_intact(snap_whole)


def mixed_learner(lay, total, method=_lib.INTERP_CLOCK, value=0.0):
    return Learner(DEV, total, torch.uint8, _lib.Interp(method, 0, value, 0.0), layout=lay)


def read_snapshot(learner, total):
    out = np.empty(total, np.uint8)
    hdr = ctypes.create_string_buffer(256)
    v = ctypes.c_uint64()
    _lib.call("dpwa_learner_read_snapshot", learner.handle, hdr, ctypes.c_void_p(out.ctypes.data), total, ctypes.byref(v))
    return _lib.Header.from_buffer_copy(hdr.raw), out, v.value


def test_one_commit_with_three_segments():
    """A write-through average of a three-segment learner (its peer its own snapshot): the new
    clock, dpwa_coef and the next publish's header {clock + 1, version, n = bytes, DPWA_MIXED} are
    each written once and correctly -- by global workgroup 0; a commit per segment would write the
    same values, so that it is one commit rests on the kernel's code (`blk == 0`)."""
    spec = ref.LAYOUTS["abutting"]
    lay, total = layout_of(spec)
    p_h, q_h = payloads("abutting")
    me = mixed_learner(lay, total)
    s = torch.cuda.current_stream()
    flat = tens(q_h).to(DEV)
    me.write_clock(6.0)
    me.publish(flat, 1.0, s)                                  # the snapshot: q, clock 7
    me.attach_local(0, me)
    flat.copy_(tens(p_h))                         # the "training step"
    me.write_clock(3.0)
    me.fetch(0, 1, True, s)
    _lib.call("dpwa_learner_average_through", me.handle, ptr(flat), 1.0, None, ctypes.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    f, new_clock = opolicy.factor_and_clock("clock", None, 0.0, 3.0, 7.0, 1.0, 1.0)
    assert ref.same(spec, host(flat), expected("abutting", f)) is None
    c = me.read_coef()
    assert c.status == 0 and c.factor == f and c.new_clock == new_clock and me.read_clock() == new_clock
    _lib.call("dpwa_learner_publish_reuse", me.handle, ptr(flat), 2.0, None, ctypes.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    hdr, payload, version = read_snapshot(me, total)
    assert version == 2 and hdr.version == 2 and hdr.clock == new_clock + 1.0
    assert hdr.n == total and hdr.dtype == _lib.MIXED
    assert np.array_equal(payload, host(flat))
    me.close()


# ---------------------------------------------------------------- 2. learner and connection
def test_split_update_wait_then_average(tmp_path):
    """The split path of the reference's seam: update_wait returns (snapshot, factor) and
    average() applies the device coefficients (the kernel's COEF_DEV form).  The snapshot of a
    mixed learner materialises as the segmented buffer's bytes."""
    spec = ref.LAYOUTS["abutting"]
    lay, total = layout_of(spec)
    p_h, q_h = payloads("abutting")
    cfg = tmp_path / "split.yaml"
    write_self_cfg(cfg, 1.0, "loss", 0.0, None)
    conn = DpwaConnection("w1", str(cfg), seed=3, group=LocalGroup(), layout=lay)
    flat = tens(q_h).to(DEV)
    conn.update_send(flat, 1.5)
    flat.copy_(tens(p_h))
    snapshot, factor = conn.update_wait(0.75)
    assert snapshot is not None and snapshot.dtype == torch.uint8 and snapshot.numel == total
    t = snapshot.tensor()
    assert t.dtype == torch.uint8 and np.array_equal(host(t), q_h)
    conn.average(flat)
    torch.cuda.synchronize()
    f, new_clock = opolicy.factor_and_clock("loss", None, 0.0, 1.0, 1.0, 0.75, 1.5)
    assert float(factor) == f and conn.clock == new_clock
    assert ref.same(spec, host(flat), expected("abutting", f)) is None
    conn.close()


def step(net, hosts, g):
    """A training step through a versioned op: every parameter moves, in its own dtype."""
    with torch.no_grad():
        for k, p in enumerate(net.parameters()):
            hosts[k] = hosts[k] + (0.05 * torch.randn(p.shape, generator=g)).to(p.dtype)
            p.copy_(hosts[k])


FORMS = {"write-through": {}, "plain": {"write_through": False}, "resident": {"resident": True}}


@pytest.mark.parametrize("body", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_adapter_on_a_mixed_model(tmp_path, form, body):
    """DpwaPyTorchAdapter on a model with fp32 LayerNorms in a bf16 / fp16 body whose peer is its
    own snapshot, four rounds of loss interpolation: the default write-through form (reuse guard
    on) and write_through=False in the reference order (update_send, step, update_wait), the
    resident form in its own (update_send, update_wait, step).  After every update_wait every
    parameter equals torch-CPU eager's `f * q + (1 - f) * p` on that tensor, dtype kept, and the
    clock the oracle policy's."""
    cfg = tmp_path / "mixed.yaml"
    write_self_cfg(cfg, 1.0, "loss", 0.0, None)
    net = ref.mixed_net(body).to(DEV)
    dtypes = [p.dtype for p in net.parameters()]
    assert set(dtypes) == {torch.float32, body}
    hosts = [p.detach().cpu().clone() for p in net.parameters()]
    ad = DpwaPyTorchAdapter(net, "w1", str(cfg), seed=3, group=LocalGroup(), **FORMS[form])
    assert ad.flat.layout is not None and ad.flat.buffer.dtype == torch.uint8
    resident = form == "resident"
    g = torch.Generator().manual_seed(7)
    clock = 0
    for r in range(4):
        send_loss, wait_loss = 1.0 + 0.25 * r, 0.5 + 0.125 * r
        ad.update_send(send_loss)
        clock += 1                                                       # dpwa.py:112
        snap = [h.clone() for h in hosts]
        if not resident:
            step(net, hosts, g)
        ad.update_wait(wait_loss)
        f, new_clock = opolicy.factor_and_clock("loss", None, 0.0, clock, clock, wait_loss, send_loss)
        for k, p in enumerate(net.parameters()):
            assert p.dtype == dtypes[k] and p.device == DEV
            hosts[k] = ref.torch_eager(hosts[k], snap[k], f)
            assert hosts[k].dtype == dtypes[k]
            assert ref.tensors_same(p, hosts[k]), (form, r, k)
        assert ad.connection.clock == new_clock, (form, r)
        assert float(ad.connection._learner.read_coef().factor) == f, (form, r)
        clock = new_clock
        if resident:
            step(net, hosts, g)
    learner = ad.connection._learner
    assert learner.dtype == torch.uint8 and learner.layout == ad.flat.layout
    if resident:
        home = ad.connection.parameters
        p0 = next(net.parameters())
        assert home.dtype == torch.uint8 and home.numel() == ad.flat.numel
        assert home.data_ptr() <= p0.data_ptr() < home.data_ptr() + home.numel()
    else:
        assert ad.reuse_guard_hits == 0
    ad.connection.close()


def test_two_mixed_learners_in_a_local_group(tmp_path):
    """Two co-resident adapters on mixed models, each the other's only peer, three rounds of loss
    interpolation in the reference order; the second round through update_wait_many (mixed
    learners are not batched: each average is a launch of its own, same results).  Every
    parameter of both against torch-CPU eager, the clocks against the oracle policy."""
    from dpwa_amd.launch import write_config
    cfg = write_config(str(tmp_path / "pair.yaml"), ["w1", "w2"], interpolation="loss", base_port=48200)
    group = LocalGroup()
    nets = [ref.mixed_net(torch.bfloat16, seed=20 + i).to(DEV) for i in range(2)]
    hosts = [[p.detach().cpu().clone() for p in net.parameters()] for net in nets]
    ads = [DpwaPyTorchAdapter(net, name, cfg, seed=5 + i, group=group)
           for i, (net, name) in enumerate(zip(nets, ["w1", "w2"]))]
    g = torch.Generator().manual_seed(8)
    clocks = [0.0, 0.0]
    for r in range(3):
        send = [1.0 + 0.25 * r, 0.625 + 0.5 * r]
        wait = [0.5 + 0.125 * r, 0.75 + 0.25 * r]
        for i in range(2):
            ads[i].update_send(send[i])
            clocks[i] += 1
        snaps = [[h.clone() for h in hs] for hs in hosts]
        published = list(clocks)
        for i in range(2):
            step(nets[i], hosts[i], g)
        if r == 1:
            DpwaPyTorchAdapter.update_wait_many(ads, wait)
        else:
            for i in range(2):
                ads[i].update_wait(wait[i])
        for i in range(2):
            j = 1 - i
            f, new_clock = opolicy.factor_and_clock("loss", None, 0.0, clocks[i], published[j], wait[i], send[j])
            for k, p in enumerate(nets[i].parameters()):
                hosts[i][k] = ref.torch_eager(hosts[i][k], snaps[j][k], f)
                assert ref.tensors_same(p, hosts[i][k]), (r, i, k)
            assert ads[i].connection.clock == new_clock, (r, i)
            clocks[i] = new_clock
    for ad in ads:
        ad.connection.close()


# ---------------------------------------------------------------- 3. what is refused
def test_learners_of_equal_bytes_and_other_layouts_do_not_attach():
    """The layout digest is the only guard between two DPWA_MIXED learners of equal size: attaching
    one to the other fails with DPWA_ERR_ARG naming the layout, in either direction."""
    a = mixed_learner(((torch.float32, 0, 4096), (torch.bfloat16, 4096, 8192)), 12288)
    b = mixed_learner(((torch.float32, 0, 8192), (torch.bfloat16, 8192, 4096)), 12288)
    c = mixed_learner(((torch.float32, 0, 4096), (torch.float16, 4096, 8192)), 12288)
    twin = mixed_learner(((torch.float32, 0, 4096), (torch.bfloat16, 4096, 8192)), 12288)
    for me, other in ((a, b), (b, a), (a, c), (c, a)):
        with pytest.raises(_lib.DpwaError) as err:
            me.attach_local(0, other)
        assert err.value.code == _lib.ERR_ARG and "layout" in str(err.value)
    a.attach_local(0, twin)
    for lr in (a, b, c, twin):
        lr.close()


def test_no_average_before_the_layout_is_set():
    """A learner created as DPWA_MIXED publishes and fetches (bytes), but the fused average and
    the factor of the split path are DPWA_ERR_STATE with a message until it has its layout; a
    layout that does not cover its bytes, or a second one, is refused; then it averages."""
    spec = ref.LAYOUTS["abutting"]
    lay, total = layout_of(spec)
    p_h, q_h = payloads("abutting")
    h = ctypes.c_void_p()
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.3, 0.0)
    _lib.call("dpwa_learner_create", ctypes.byref(h), 0, total, _lib.MIXED, ctypes.byref(cfg))
    lib = _lib.load()
    try:
        s = stream()
        flat = tens(q_h).to(DEV)
        _lib.call("dpwa_learner_publish", h, ptr(flat), 1.0, None, s)
        _lib.call("dpwa_learner_attach_local", h, 0, h)
        _lib.call("dpwa_learner_fetch", h, 0, 1, 1, s)
        flat.copy_(tens(p_h))
        for call in (lambda: lib.dpwa_learner_average(h, ptr(flat), 1.0, None, s),
                     lambda: lib.dpwa_learner_average_through(h, ptr(flat), 1.0, None, s),
                     lambda: lib.dpwa_learner_factor(h, 1.0, None, s)):
            assert call() == _lib.ERR_STATE
            assert b"dpwa_learner_set_layout" in lib.dpwa_last_error()
        short = c_layout(lay[:2])
        assert lib.dpwa_learner_set_layout(h, ctypes.byref(short)) == _lib.ERR_ARG
        assert b"cover" in lib.dpwa_last_error()
        bad = c_layout(((torch.float32, 0, 4096 + 16), (torch.bfloat16, 4096 + 16, total - 4096 - 16)))
        assert lib.dpwa_learner_set_layout(h, ctypes.byref(bad)) == _lib.ERR_ARG
        _lib.call("dpwa_learner_set_layout", h, ctypes.byref(c_layout(lay)))
        _lib.call("dpwa_learner_set_layout", h, ctypes.byref(c_layout(lay)))          # the same again: fine
        other = c_layout(((torch.float32, 0, total),))
        assert lib.dpwa_learner_set_layout(h, ctypes.byref(other)) == _lib.ERR_STATE
        torch.cuda.synchronize()
        assert np.array_equal(host(flat), p_h)                               # nothing ran so far
        _lib.call("dpwa_learner_average", h, ptr(flat), 1.0, None, s)
        torch.cuda.synchronize()
        assert ref.same(spec, host(flat), expected("abutting", 0.3)) is None
        # a single-dtype learner takes no layout
        plain = Learner(DEV, total // 2, torch.bfloat16, cfg)
        assert lib.dpwa_learner_set_layout(plain.handle, ctypes.byref(c_layout(lay))) == _lib.ERR_ARG
        plain.close()
    finally:
        lib.dpwa_learner_destroy(h)


def test_malformed_layouts_and_batches_are_refused_on_the_device():
    """dpwa_average_mixed with a malformed layout or an unaligned pointer, and dpwa_average_many
    with DPWA_MIXED, return DPWA_ERR_ARG and launch nothing."""
    lay, total = layout_of(ref.LAYOUTS["abutting"])
    p_h, q_h = payloads("abutting")
    p, _ = on_device(p_h)
    slot = average_slot(tens(q_h).to(DEV), 7.0, 1.0)
    clock = torch.tensor([3.0, -1.0], dtype=torch.float64, device=DEV)
    coef = torch.zeros(32, dtype=torch.uint8, device=DEV)
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    lib = _lib.load()
    bad = [((torch.float32, 0, 4096), (torch.bfloat16, 4096 + 1024, 8192)),
           ((torch.float32, 0, 4096), (torch.float32, 4096, 8192)),
           ((torch.bfloat16, 4096, 8192), (torch.float32, 0, 4096)),
           ((torch.float32, 0, 8192), (torch.bfloat16, 4096, 8192)),
           ()]
    for b in bad:
        rc = lib.dpwa_average_mixed(ctypes.byref(c_layout(b)), ptr(p), ptr(slot), ctypes.byref(cfg), ptr(clock), 1.0,
                                    ptr(coef), None, stream(), None, None)
        assert rc == _lib.ERR_ARG, b
    rc = lib.dpwa_average_mixed(ctypes.byref(c_layout(lay)), ctypes.c_void_p(p.data_ptr() + 4), ptr(slot),
                                ctypes.byref(cfg), ptr(clock), 1.0, ptr(coef), None, stream(), None, None)
    assert rc == _lib.ERR_ARG
    desc = (_lib.AverageDesc * 1)(_lib.AverageDesc(p.data_ptr(), slot.data_ptr(), total, clock.data_ptr(), 1.0,
                                                    coef.data_ptr(), None))
    for fn in (lib.dpwa_average_many, lib.dpwa_average_many_resident):
        assert fn(_lib.MIXED, desc, 1, ctypes.byref(cfg), stream(), None, None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert np.array_equal(host(p), p_h) and clock[1].item() == -1.0


def test_relay_avg_wire_and_bare_uint8_are_refused(tmp_path):
    """A bound mixed connection refuses pull='relay-avg' with a ValueError naming it ('kernel'
    moves bytes and is accepted); the wire transport refuses a mixed model with the KeyError a
    16-bit model gets; a uint8 buffer without a layout is the KeyError of any other dtype."""
    lay, total = layout_of(ref.LAYOUTS["one-each"])
    cfg = tmp_path / "r.yaml"
    write_self_cfg(cfg, 1.0, "constant", 0.0, 0.5)
    conn = DpwaConnection("w1", str(cfg), seed=3, group=LocalGroup(), layout=lay)
    flat = torch.zeros(total, dtype=torch.uint8, device=DEV)
    conn.update_send(flat, 1.0)
    with pytest.raises(ValueError, match="relay-avg"):
        conn.set_pull("relay-avg")
    conn.set_pull("kernel:8")
    conn.update_wait_average(flat, 1.0)
    conn.close()
    bare = DpwaConnection("w1", str(cfg), seed=3, group=LocalGroup())
    with pytest.raises(KeyError, match="float32, bfloat16 or float16"):
        bare.update_send(flat, 1.0)
    bare.close()
    errors = []
    for net in (ref.mixed_net(torch.float16).to(DEV), torch.nn.Linear(3, 2).half().to(DEV)):
        ad = DpwaPyTorchAdapter(net, "w1", str(cfg), transport="wire", seed=1, serve=False)
        with pytest.raises(KeyError) as err:
            ad.update_send(1.0)
        errors.append(str(err.value))
        ad.connection.close()
    assert errors[0] == errors[1] and "float32" in errors[0]


# ---------------------------------------------------------------- 4. nothing else changed
def test_a_single_dtype_model_binds_as_before(tmp_path):
    """A bf16 model through the adapter: a bfloat16 flat buffer, no layout, a DPWA_BF16 learner
    whose published header says so."""
    cfg = tmp_path / "bf16.yaml"
    write_self_cfg(cfg, 1.0, "constant", 0.0, 0.5)
    net = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.LayerNorm(17)).bfloat16().to(DEV)
    ad = DpwaPyTorchAdapter(net, "w1", str(cfg), seed=3, group=LocalGroup())
    assert ad.flat.layout is None and ad.flat.buffer.dtype == torch.bfloat16
    ad.update_send(1.0)
    learner = ad.connection._learner
    assert learner.dtype == torch.bfloat16 and learner.layout is None and learner.numel == ad.flat.numel
    hdr = ctypes.create_string_buffer(256)
    out = np.empty(ad.flat.numel, np.uint16)
    v = ctypes.c_uint64()
    _lib.call("dpwa_learner_read_snapshot", learner.handle, hdr, ctypes.c_void_p(out.ctypes.data), out.nbytes,
              ctypes.byref(v))
    h = _lib.Header.from_buffer_copy(hdr.raw)
    assert h.dtype == _lib.BF16 and h.n == ad.flat.numel and v.value == 1
    ad.update_wait(1.0)
    ad.connection.close()


# ---------------------------------------------------------------- 5. one segment is the single-dtype call
@functools.lru_cache(maxsize=None)
def seam_operands(d, nbytes):
    """(param bits, peer bits) of `nbytes` of dtype d: N(0,1), -0 meeting the smallest subnormal in the
    first element and the largest finite value meeting +0 in the last.  Made once, read-only."""
    n = nbytes // ref.SIZE[d]
    rng = np.random.default_rng(nbytes + ref.CODE[d])
    p, q = dist_ref.to_bits(d, rng.standard_normal(n)), dist_ref.to_bits(d, rng.standard_normal(n))
    hard = ref.HARD[d]
    p[0], q[0] = hard[1], hard[2]
    p[-1], q[-1] = hard[7], hard[0]
    p.setflags(write=False)
    q.setflags(write=False)
    return p, q


def average_single(d, n, p, slot, case, snap):
    """average_mixed's twin through dpwa_average."""
    method, value, thr, my_clock, _, loss, _ = case
    clock = torch.tensor([my_clock, -1.0], dtype=torch.float64, device=DEV)
    coef = torch.zeros(32, dtype=torch.uint8, device=DEV)
    cfg = _lib.Interp(opolicy.METHODS[method], 0, float(value or 0.0), float(thr))
    _lib.call("dpwa_average", ref.CODE[d], ptr(p), ptr(slot), n, ctypes.byref(cfg), ptr(clock), float(loss), ptr(coef),
              ptr(snap) if snap is not None else None, stream(), None, None)
    torch.cuda.synchronize()
    return _lib.Coef.from_buffer_copy(coef.cpu().numpy().tobytes()), clock[1].item()


@pytest.mark.parametrize("nbytes", [4096, 8192])
@pytest.mark.parametrize("d", ref.ORDER)
def test_a_single_segment_is_the_single_dtype_call(d, nbytes):
    """A layout of one segment (one and two 4-KiB blocks: 4 and 8 spans) through the three _mixed
    entries against the single-dtype entries with n = bytes / size, on copies of the same operands.
    The average, plain and write-through: parameters, snapshot payload, dpwa_coef and clock bit-equal
    to each other and to the host reference of the dtype and the oracle policy.  The finite check,
    without a non-finite element and with +inf in the peer's last element: both veto words are what
    the host expects.  The distance: both within tests/dist_ref.py's bound of its fsum reference."""
    n = nbytes // ref.SIZE[d]
    spec = [(d, n)]
    lay, total = layout_of(spec)
    assert total == nbytes and len(lay) == 1
    p_bits, q_bits = seam_operands(d, nbytes)
    p_h, q_h = p_bits.view(np.uint8), q_bits.view(np.uint8)
    case = FUSED[1]
    method, value, thr, my_clock, peer_clock, loss, peer_loss = case
    f, new_clock = opolicy.factor_and_clock(method, value, thr, my_clock, peer_clock, loss, peer_loss)
    want = ref.lerp(spec, p_h, q_h, f)
    for write_through in (False, True):
        left = []
        for mixed in (True, False):
            p, p_whole = on_device(p_h)
            slot = average_slot(tens(q_h).to(DEV), peer_clock, peer_loss)
            snap, snap_whole = on_device(np.full(total, 0x55, dtype=np.uint8)) if write_through else (None, None)
            c, got_clock = average_mixed(lay, p, slot, case, snap) if mixed else average_single(d, n, p, slot, case, snap)
            what = (d, nbytes, write_through, "mixed" if mixed else "single")
            assert ref.same(spec, host(p), want) is None, (what, ref.same(spec, host(p), want))
            assert c.status == 0 and c.factor == f and c.a == np.float32(f) and c.b == np.float32(1.0 - f), what
            assert got_clock == new_clock == c.new_clock, what
            assert guard_intact(p_whole) and np.array_equal(host(slot[OFF:]), q_h), what
            if write_through:
                assert ref.same(spec, host(snap), want) is None and guard_intact(snap_whole), what
            left.append((host(p).tobytes(), host(snap).tobytes() if write_through else None, bytes(c), got_clock))
        assert left[0] == left[1], (d, nbytes, write_through, "the two entries leave different bytes")

    clean = tens(q_h).to(DEV)
    q_inf = np.array(q_bits)
    q_inf[-1] = ref.HARD[d][9]
    poisoned = tens(q_inf.view(np.uint8)).to(DEV)
    sentinel, stamp = 0x5a5a5a5a, 0x9e3779b9
    words = torch.full((4,), sentinel, dtype=torch.int32, device=DEV)
    for i, (buf, mixed) in enumerate(((clean, True), (clean, False), (poisoned, True), (poisoned, False))):
        word = ctypes.c_void_p(words.data_ptr() + 4 * i)
        if mixed:
            _lib.call("dpwa_check_finite_mixed", ctypes.byref(c_layout(lay)), ptr(buf), word, stamp, stream(), None, None)
        else:
            _lib.call("dpwa_check_finite", ref.CODE[d], ptr(buf), n, word, stamp, stream(), None, None)
    torch.cuda.synchronize()
    assert words.cpu().numpy().view(np.uint32).tolist() == [sentinel, sentinel, stamp, stamp], (d, nbytes)

    # (the largest finite value's square hides every other term under the bound: once more without it)
    p_small = np.array(p_bits)
    p_small[-1] = ref.HARD[d][1]
    for name, pb in (("hard", p_bits), ("no-huge", p_small)):
        want_dist = dist_ref.reference(d, pb, q_bits)
        p, q = tens(pb.view(np.uint8)).to(DEV), tens(q_h).to(DEV)
        for mixed in (True, False):
            rec = fresh_record()
            if mixed:
                _lib.call("dpwa_measure_distance_mixed", ctypes.byref(c_layout(lay)), ptr(p), ptr(q), ptr(workspace()),
                          ptr(rec), stream())
            else:
                _lib.call("dpwa_measure_distance", ref.CODE[d], ptr(p), ptr(q), n, ptr(workspace()), ptr(rec), stream())
            torch.cuda.synchronize()
            check_record(read_record(rec), want_dist, n, 0.0, (d, nbytes, name, "mixed" if mixed else "single"))
        assert np.array_equal(host(p), pb.view(np.uint8)) and np.array_equal(host(q), q_h)
    assert not bool(workspace().any()), "both entries leave the accumulators zero"
