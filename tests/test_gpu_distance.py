"""The distance to the peer on the GPU (include/dpwa_hip.h ``dpwa_distance``): the tracked form of the
fused average, the stand-alone pass and the finishing step, against tests/dist_ref.py (float64 terms
summed exactly on the host) within its derived bound; the averaged parameters, snapshot, clock and
coefficients of a tracked average bit-equal to the untracked one and to the host references.

Shapes are the smallest at which each case can go wrong: a one-wave span is 256 fp32 / 512 16-bit
elements, a lane's item 4 / 8; the only larger size has three times as many spans as the
implementation has accumulators (the count is read from the workspace size and stated below)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dpwa_amd import DpwaConnection, DpwaPyTorchAdapter, _lib
from dpwa_amd.devview import device_tensor
from dpwa_amd.flat import c_layout
from dpwa_amd.group import LocalGroup
from dpwa_amd.learner import Learner
from oracle import lerp as olerp
from oracle import policy as opolicy
from tests import dist_ref as ref
from tests import f16_ref, mixed_ref
from tests.test_gpu_kernels import average_slot, ptr, stream
from tests.test_gpu_self_peer import write_self_cfg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OFF = _lib.SLOT_PAYLOAD_OFFSET
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
NAME = {v: k for k, v in TORCH.items()}
# clock interpolation, my clock 3, the peer's 7: f = 0.7, the new clock 5.8
CASE = ("clock", None, 0.0, 3.0, 7.0, 1.0, 1.0)
F, NEW_CLOCK = opolicy.factor_and_clock(*CASE)


@functools.lru_cache(maxsize=None)
def workspace_bytes():
    b = ctypes.c_int64()
    _lib.call("dpwa_distance_workspace", ctypes.byref(b))
    return b.value


def accumulators():
    """How many accumulators the implementation has: 1024 (128 KiB of 128-byte rows) as built."""
    return workspace_bytes() // _lib.DISTANCE_ACC_STRIDE


@functools.lru_cache(maxsize=None)
def workspace():
    """One zeroed workspace for every stateless call of this module: each call must leave it zero."""
    return torch.zeros(workspace_bytes(), dtype=torch.uint8, device=DEV)


def fresh_record():
    return torch.full((32,), 0xa5, dtype=torch.uint8, device=DEV)        # poisoned: a record must be written


def read_record(t):
    return _lib.Distance.from_buffer_copy(t.cpu().numpy().tobytes())


def to_dev(dtype, bits):
    bits = np.ascontiguousarray(bits)
    signed = bits.view(np.int32 if dtype == "f32" else np.int16)
    return torch.from_numpy(signed.copy()).view(TORCH[dtype]).to(DEV)


def bits_of(dtype, t):
    t = t.detach().contiguous().cpu().reshape(-1)
    if dtype == "f32":
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def host_average(dtype, p_bits, q_bits, f):
    if dtype == "f32":
        return olerp.lerp_f32(p_bits.view(np.float32), q_bits.view(np.float32), f).view(np.uint32)
    if dtype == "bf16":
        return olerp.lerp_bf16(p_bits, q_bits, f)
    return f16_ref.torch_lerp(p_bits, q_bits, f)


def same_bits(dtype, got, want):
    if dtype == "f32":
        return olerp.bits_equal(got.view(np.float32), want.view(np.float32))
    if dtype == "bf16":
        return olerp.bits_equal(got, want)
    return f16_ref.same(got, want)


def check_record(rec, want, n, clock, what):
    for got, w, name in ((rec.dist2, want[0], "dist2"), (rec.norm2, want[1], "norm2")):
        why = ref.problem(got, w, n)
        print("%s %s: got %r ref %r bound %.3g" % (what, name, got, w, ref.bound(n)))
        assert why is None, (what, name, why)
    assert rec.clock == clock and rec.n == n, (what, rec.clock, clock, rec.n, n)


def fused(entry, dtype, p_bits, q_bits, write_through, case=CASE, rec=None):
    """One dpwa_average / dpwa_average_tracked on fresh buffers; everything it wrote, on the host."""
    n = len(p_bits)
    p = to_dev(dtype, p_bits)
    slot = average_slot(to_dev(dtype, q_bits), case[4], case[6])
    snap = torch.full_like(p, float("nan")) if write_through else None
    clock = torch.tensor([case[3], -1.0], dtype=torch.float64, device=DEV)
    coef = torch.zeros(32, dtype=torch.uint8, device=DEV)
    cfg = _lib.Interp(opolicy.METHODS[case[0]], 0, float(case[1] or 0.0), float(case[2]))
    head = (ref.CODE[dtype], ptr(p), ptr(slot), n, ctypes.byref(cfg), ptr(clock), float(case[5]), ptr(coef),
            ptr(snap) if snap is not None else None)
    if entry == "dpwa_average":
        _lib.call(entry, *head, stream(), None, None)
    else:
        _lib.call(entry, *head, ptr(workspace()), ptr(rec), stream(), None, None)
    torch.cuda.synchronize()
    return {"p": bits_of(dtype, p), "snap": bits_of(dtype, snap) if write_through else None,
            "coef": coef.cpu().numpy().tobytes(), "clock": clock.cpu().tolist(),
            "peer": bits_of(dtype, slot[OFF:].view(TORCH[dtype]))}


def measure(dtype, p, q, n, rec):
    _lib.call("dpwa_measure_distance", ref.CODE[dtype], ptr(p), ptr(q), n, ptr(workspace()), ptr(rec), stream())
    torch.cuda.synchronize()
    return read_record(rec)


def run_cases(dtype, n, only=None):
    for name, p_bits, q_bits in ref.cases(dtype, n, accumulators()):
        if only is not None and name not in only:
            continue
        what = (dtype, n, name)
        want = ref.reference(dtype, p_bits, q_bits)         # once, shared by the three entries below
        averaged = host_average(dtype, p_bits, q_bits, F)
        for write_through in (False, True):
            rec = fresh_record()
            plain = fused("dpwa_average", dtype, p_bits, q_bits, write_through)
            tracked = fused("dpwa_average_tracked", dtype, p_bits, q_bits, write_through, rec=rec)
            assert same_bits(dtype, tracked["p"], averaged), what
            for key in ("p", "snap", "coef", "clock", "peer"):          # exactly what dpwa_average leaves
                a, b = plain[key], tracked[key]
                assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, (what, write_through, key)
            assert np.array_equal(tracked["peer"], q_bits), what
            if write_through:
                assert np.array_equal(tracked["snap"], tracked["p"]), what
            assert tracked["clock"] == [CASE[3], NEW_CLOCK], what
            check_record(read_record(rec), want, n, NEW_CLOCK, what + ("tracked", write_through))
        p, q = to_dev(dtype, p_bits), to_dev(dtype, q_bits)
        check_record(measure(dtype, p, q, n, fresh_record()), want, n, 0.0, what + ("stand-alone",))
        assert np.array_equal(bits_of(dtype, p), p_bits) and np.array_equal(bits_of(dtype, q), q_bits), what
    assert not bool(workspace().any()), "every entry leaves the accumulators zero"


# ---------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("dtype,n", [(d, n) for d in ref.DTYPES for n in ref.SIZES[d]])
def test_tracked_average_and_stand_alone_pass(dtype, n):
    """Every input set of tests/dist_ref.py (N(0,1); q == p, exactly 0; the one difference in the last
    tail element / the last lane of the last full span; huge values of opposite signs; subnormal-only
    differences; signed zeros; one NaN; one inf) through dpwa_average_tracked, plain and write-through,
    and through dpwa_measure_distance."""
    run_cases(dtype, n)


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_more_spans_than_accumulators(dtype):
    """(3 * accumulators + 2) spans and a tail -- 1024 accumulators as built, so 3074 spans: every
    accumulator is added into three times or more, and the case whose only difference lies in span
    accumulators + 1 wraps around onto accumulator 1."""
    n = ref.many_spans(dtype, accumulators())
    assert n // ref.SPAN[dtype] >= 3 * accumulators()
    run_cases(dtype, n, only=("normal", "equal", "span-beyond-the-accumulators"))


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_operands_four_bytes_off_alignment(dtype):
    """Operands 4 bytes off a 16-byte boundary take the element-wise pass (dpwa_measure_distance), and
    dpwa_average_tracked on such parameters runs it ahead of dpwa_average's own unaligned kernel."""
    n, off = 10_007, 4 // ref.SIZE[dtype]
    _, p_bits, q_bits = ref.cases(dtype, n + 16)[0]
    want = ref.reference(dtype, p_bits[off:off + n], q_bits[2 * off:2 * off + n])
    base_p, base_q = to_dev(dtype, p_bits), to_dev(dtype, q_bits)
    p, q = base_p[off:off + n], base_q[2 * off:2 * off + n]
    assert p.data_ptr() % 16 == 4 and q.data_ptr() % 16 == 8
    check_record(measure(dtype, p, q, n, fresh_record()), want, n, 0.0, (dtype, "stand-alone"))
    assert np.array_equal(bits_of(dtype, base_p), p_bits) and np.array_equal(bits_of(dtype, base_q), q_bits)
    # the fused entry on unaligned parameters (the peer payload of a slot is always aligned)
    slot = average_slot(to_dev(dtype, q_bits[:n]), CASE[4], CASE[6])
    want = ref.reference(dtype, p_bits[off:off + n], q_bits[:n])
    got = {}
    for entry in ("dpwa_average", "dpwa_average_tracked"):
        base = to_dev(dtype, p_bits)
        clock = torch.tensor([CASE[3], -1.0], dtype=torch.float64, device=DEV)
        coef = torch.zeros(32, dtype=torch.uint8, device=DEV)
        cfg = _lib.Interp(_lib.INTERP_CLOCK, 0, 0.0, 0.0)
        rec = fresh_record()
        head = (ref.CODE[dtype], ptr(base[off:off + n]), ptr(slot), n, ctypes.byref(cfg), ptr(clock), 1.0, ptr(coef), None)
        tail = (stream(), None, None)
        _lib.call(entry, *head, *(tail if entry == "dpwa_average" else (ptr(workspace()), ptr(rec)) + tail))
        torch.cuda.synchronize()
        got[entry] = (bits_of(dtype, base), coef.cpu().numpy().tobytes(), clock.cpu().tolist())
    assert np.array_equal(got["dpwa_average"][0], got["dpwa_average_tracked"][0])
    assert got["dpwa_average"][1:] == got["dpwa_average_tracked"][1:]
    averaged = host_average(dtype, p_bits[off:off + n], q_bits[:n], F)
    assert same_bits(dtype, got["dpwa_average_tracked"][0][off:off + n], averaged)
    check_record(read_record(rec), want, n, NEW_CLOCK, (dtype, "tracked, unaligned"))
    assert not bool(workspace().any())


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_a_zero_division_round_leaves_the_record(dtype):
    """Clock interpolation with both clocks 0: nothing is averaged, the record keeps its bytes and the
    accumulators are zero for the next round, which then reports only its own sums."""
    n = 1541
    _, p_bits, q_bits = ref.cases(dtype, n)[0]
    rec = fresh_record()
    out = fused("dpwa_average_tracked", dtype, p_bits, q_bits, True, case=("clock", None, 0.0, 0.0, 0.0, 1.0, 1.0),
                rec=rec)
    assert _lib.Coef.from_buffer_copy(out["coef"]).status == _lib.STATUS_ZERO_DIVISION
    assert np.array_equal(out["p"], p_bits) and np.array_equal(out["snap"], p_bits)
    assert bool((rec == 0xa5).all()) and not bool(workspace().any())
    fused("dpwa_average_tracked", dtype, p_bits, q_bits, False, rec=rec)
    check_record(read_record(rec), ref.reference(dtype, p_bits, q_bits), n, NEW_CLOCK, (dtype, "the round after"))


# ---------------------------------------------------------------- 2. one learner, two rounds
def learner_record(learner):
    p = ctypes.c_void_p()
    _lib.call("dpwa_learner_distance", learner.handle, ctypes.byref(p))
    return read_record(device_tensor(p.value, 32, torch.uint8, DEV))


@pytest.mark.parametrize("dtype", ref.DTYPES)
@pytest.mark.parametrize("write_through", [False, True])
def test_two_rounds_back_to_back_on_one_learner(dtype, write_through):
    """A tracking learner whose peer is its own snapshot, two rounds with different data and no host
    wait between them: the record after the second round holds only the second round's sums and the
    second round's clock (the accumulators are reset by the finishing step)."""
    n = 3 * ref.SPAN[dtype] + 5
    me = Learner(DEV, n, TORCH[dtype], _lib.Interp(_lib.INTERP_CLOCK, 0, 0.0, 0.0))
    with pytest.raises(_lib.DpwaError) as err:               # never switched on: no record yet
        learner_record(me)
    assert err.value.code == _lib.ERR_STATE
    _lib.call("dpwa_learner_set_distance", me.handle, 1)
    me.attach_local(0, me)
    s = torch.cuda.current_stream()
    sets = [ref.cases(dtype, n, seed=r)[0] for r in (1, 2)]
    flat = to_dev(dtype, sets[0][2])
    for r, (_, p_bits, q_bits) in enumerate(sets):
        flat.copy_(to_dev(dtype, q_bits))
        me.publish(flat, 1.0, s)                             # the snapshot: this round's q
        flat.copy_(to_dev(dtype, p_bits))                    # the "training step"
        me.fetch(0, me.version, True, s)
        fn = "dpwa_learner_average_through" if write_through else "dpwa_learner_average"
        _lib.call(fn, me.handle, ptr(flat), 1.0, None, ctypes.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    _, p_bits, q_bits = sets[1]
    check_record(learner_record(me), ref.reference(dtype, p_bits, q_bits), n, me.read_clock(), (dtype, "round 2"))
    assert me.read_coef().status == 0
    me.close()


def test_tracking_refuses_the_fused_relay_phase():
    """dpwa_learner_relay_phase2(fuse != 0) on a tracking learner is DPWA_ERR_STATE (the fused second
    phase has no contiguous peer snapshot), before any relay work is queued."""
    n = 4096
    me = Learner(DEV, n, torch.float32, _lib.Interp(_lib.INTERP_CLOCK, 0, 0.0, 0.0))
    _lib.call("dpwa_learner_set_distance", me.handle, 1)
    _lib.call("dpwa_learner_relay_enable", me.handle, 2, 0)
    picks = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    lib = _lib.load()
    assert lib.dpwa_learner_relay_phase2(me.handle, ptr(picks), 1, 1, 1, 1) == _lib.ERR_STATE
    assert b"dpwa_learner_relay_phase2" in lib.dpwa_last_error() and b"distance" in lib.dpwa_last_error()
    me.close()


# ---------------------------------------------------------------- 3. segmented payloads
MIXED = {"f32-3+f16-4097": [("f32", 3), ("f16", 4097)], "f32-block+bf16-block-and-one": [("f32", 1024), ("bf16", 2049)]}


def mixed_payloads(spec, seed):
    """(param bytes, peer bytes, [(dtype, p_bits, q_bits)] of the real elements): N(0,1) in every
    element, zero padding."""
    segs, total = mixed_ref.segments(spec)
    rng = np.random.default_rng(seed)
    p, q, parts = np.zeros(total, np.uint8), np.zeros(total, np.uint8), []
    for d, off, _, n in segs:
        pb, qb = ref.to_bits(d, rng.standard_normal(n)), ref.to_bits(d, rng.standard_normal(n))
        p[off:off + n * ref.SIZE[d]] = pb.view(np.uint8)
        q[off:off + n * ref.SIZE[d]] = qb.view(np.uint8)
        parts.append((d, pb, qb))
    return p, q, parts, segs, total


@pytest.mark.parametrize("name", sorted(MIXED))
@pytest.mark.parametrize("write_through", [False, True])
def test_mixed_payload(name, write_through):
    """A segmented learner with tracking on runs the stand-alone pass before its unchanged average:
    the record is the reference over the real elements of all segments (the padding adds 0), each
    segment alone through dpwa_measure_distance is its own reference, and the averaged bytes are
    the untracked learner's."""
    spec = MIXED[name]
    p_h, q_h, parts, segs, total = mixed_payloads(spec, 5)
    lay = tuple((mixed_ref.TORCH[d], off, length) for d, off, length, _ in segs)
    slots = sum(length // ref.SIZE[d] for d, _, length, _ in segs)
    real = sum(n for _, _, _, n in segs)
    results = {}
    for track in (False, True):
        me = Learner(DEV, total, torch.uint8, _lib.Interp(_lib.INTERP_CLOCK, 0, 0.0, 0.0), layout=lay)
        if track:
            _lib.call("dpwa_learner_set_distance", me.handle, 1)
        s = torch.cuda.current_stream()
        flat = torch.from_numpy(q_h.copy()).to(DEV)
        me.write_clock(6.0)
        me.publish(flat, 1.0, s)
        me.attach_local(0, me)
        flat.copy_(torch.from_numpy(p_h.copy()))
        me.write_clock(3.0)
        me.fetch(0, 1, True, s)
        fn = "dpwa_learner_average_through" if write_through else "dpwa_learner_average"
        _lib.call(fn, me.handle, ptr(flat), 1.0, None, ctypes.c_void_p(s.cuda_stream))
        torch.cuda.synchronize()
        results[track] = (flat.cpu().numpy(), me.read_clock())
        if track:
            rec = learner_record(me)
            want = ref.reference_many(parts)
            for got, w, what in ((rec.dist2, want[0], "dist2"), (rec.norm2, want[1], "norm2")):
                assert ref.problem(got, w, real) is None, (name, what, ref.problem(got, w, real))
            assert rec.clock == NEW_CLOCK == me.read_clock() and rec.n == slots
        me.close()
    assert np.array_equal(results[False][0], results[True][0]) and results[False][1] == results[True][1]
    assert mixed_ref.same(spec, results[True][0], mixed_ref.lerp(spec, p_h, q_h, F)) is None
    # the stateless entry on the whole payload, and each segment alone as a single-dtype buffer
    p, q = torch.from_numpy(p_h.copy()).to(DEV), torch.from_numpy(q_h.copy()).to(DEV)
    rec = fresh_record()
    _lib.call("dpwa_measure_distance_mixed", ctypes.byref(c_layout(lay)), ptr(p), ptr(q), ptr(workspace()), ptr(rec),
              stream())
    torch.cuda.synchronize()
    check_record(read_record(rec), ref.reference_many(parts), slots, 0.0, (name, "stateless"))
    for (d, off, _, n), (_, pb, qb) in zip(segs, parts):
        view = lambda t: t[off:off + n * ref.SIZE[d]].view(TORCH[d])            # noqa: E731
        check_record(measure(d, view(p), view(q), n, fresh_record()), ref.reference(d, pb, qb), n, 0.0, (name, d))
    assert not bool(workspace().any())


# ---------------------------------------------------------------- 4. the adapter and the connection
def make_net(kind):
    if kind == "mixed":
        return mixed_ref.mixed_net(torch.bfloat16).to(DEV)
    g = torch.Generator().manual_seed(6)
    net = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.Linear(17, 5))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    return (net.bfloat16() if kind == "bf16" else net).to(DEV)


def model_reference(host, snap):
    parts = [(NAME[h.dtype], mixed_ref.tensor_bits(h), mixed_ref.tensor_bits(q)) for h, q in zip(host, snap)]
    return ref.reference_many(parts), sum(h.numel() for h in host)


FORMS = {"write-through": {}, "plain": {"write_through": False}, "resident": {"resident": True}}


@pytest.mark.parametrize("kind", ["f32", "bf16", "mixed"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_adapter_rounds(tmp_path, kind, form):
    """DpwaPyTorchAdapter(track_distance=True) on a small fp32 model, a ``.bfloat16()`` model and an
    fp32-norm + bf16-body model, in its three forms, its peer its own snapshot: four rounds with an
    optimiser-like write between them.  After every round last_distance is the reference over
    torch-CPU copies of the parameters and of the snapshot taken before the average, and its clock
    the connection's.  (The resident form steps after the average, so there p == q: exactly 0.)"""
    cfg = tmp_path / "adapter.yaml"
    write_self_cfg(cfg, 1.0, "loss", 0.0, None)
    net = make_net(kind)
    ad = DpwaPyTorchAdapter(net, "w1", str(cfg), seed=3, group=LocalGroup(), track_distance=True, **FORMS[form])
    assert ad.last_distance is None
    g = torch.Generator().manual_seed(9)
    resident = form == "resident"

    def step():
        with torch.no_grad():
            for p in net.parameters():
                p.copy_((p.detach().cpu().float() + 0.05 * torch.randn(p.shape, generator=g)).to(p.dtype))

    for r in range(4):
        ad.update_send(1.0 + 0.25 * r)
        snap = [p.detach().cpu().clone() for p in net.parameters()]
        if not resident:
            step()
        host = [p.detach().cpu().clone() for p in net.parameters()]
        ad.update_wait(0.5 + 0.125 * r)
        d = ad.last_distance
        assert d is not None and ad.connection.last_distance is d
        want, n = model_reference(host, snap)
        rec = d.read()
        for got, w, what in ((rec.dist2, want[0], "dist2"), (rec.norm2, want[1], "norm2")):
            print("%s %s round %d %s: got %r ref %r" % (kind, form, r, what, got, w))
            assert ref.problem(got, w, n) is None, (kind, form, r, what, ref.problem(got, w, n))
        assert d.clock == ad.connection.clock, (kind, form, r)
        t = d.tensor()
        assert t.dtype == torch.float64 and t.device == DEV and t.cpu().tolist() == [rec.dist2, rec.norm2, rec.clock]
        assert d.distance == rec.dist2 ** 0.5 and d.norm == rec.norm2 ** 0.5
        assert d.relative == (rec.dist2 / rec.norm2) ** 0.5
        if resident:
            assert rec.dist2 == 0.0
            step()
    ad.connection.close()


def test_gated_off_and_zero_division_rounds(tmp_path):
    """fetch_probability 0: no round averages and last_distance stays None.  A round whose loss
    interpolation divides by zero leaves the previous round's record, bit for bit."""
    cfg = tmp_path / "off.yaml"
    write_self_cfg(cfg, 0.0, "loss", 0.0, None)
    net = make_net("f32")
    ad = DpwaPyTorchAdapter(net, "w1", str(cfg), seed=3, group=LocalGroup(), track_distance=True)
    for r in range(3):
        ad.update_send(1.0)
        ad.update_wait(1.0)
    torch.cuda.synchronize()
    assert ad.last_distance is None
    ad.connection.close()

    cfg = tmp_path / "zd.yaml"
    write_self_cfg(cfg, 1.0, "loss", 0.0, None)
    net = make_net("f32")
    ad = DpwaPyTorchAdapter(net, "w1", str(cfg), seed=3, group=LocalGroup(), track_distance=True)
    ad.update_send(1.0)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.125)
    ad.update_wait(0.5)
    first = bytes(ad.last_distance.read())
    assert ad.last_distance.read().dist2 > 0.0
    ad.update_send(0.0)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.25)
    ad.update_wait(0.0)                                      # loss + peer loss == 0
    with pytest.raises(ZeroDivisionError):
        ad.connection.synchronize()
    assert bytes(ad.last_distance.read()) == first
    ad.connection.close()


def test_split_update_wait_then_average(tmp_path):
    """The reference's seam: update_wait() returns (payload, factor) and leaves last_distance as it
    was; conn.average(parameters) after it measures, through the stand-alone pass."""
    n = 1541
    cfg = tmp_path / "split.yaml"
    write_self_cfg(cfg, 1.0, "loss", 0.0, None)
    conn = DpwaConnection("w1", str(cfg), seed=3, group=LocalGroup(), track_distance=True)
    _, p_bits, q_bits = ref.cases("f32", n)[0]
    flat = to_dev("f32", q_bits)
    conn.update_send(flat, 1.5)
    flat.copy_(to_dev("f32", p_bits))
    payload, factor = conn.update_wait(0.75)
    assert payload is not None and conn.last_distance is None
    conn.average(flat)
    torch.cuda.synchronize()
    f, new_clock = opolicy.factor_and_clock("loss", None, 0.0, 1.0, 1.0, 0.75, 1.5)
    assert olerp.bits_equal(flat.cpu().numpy(), olerp.lerp_f32(p_bits.view(np.float32), q_bits.view(np.float32), f))
    check_record(conn.last_distance.read(), ref.reference("f32", p_bits, q_bits), n, new_clock, "split")
    assert conn.clock == new_clock
    conn.close()


def test_two_tracking_learners_through_update_wait_many(tmp_path):
    """Two co-resident adapters that average with each other through update_wait_many (one batched
    dispatch, which stays as it is): both records are right, and the averaged parameters and clocks
    are bit-equal to the same rounds with tracking off."""
    cfg = tmp_path / "many.yaml"
    lines = ["- nodes:", "  - {name: a0, host: localhost, port: 46100}", "  - {name: a1, host: localhost, port: 46101}",
             "- fetch_probability: 1.0", "- timeout_ms: 2500", "- interpolation: clock", "- divergence_threshold: 0",
             "- constant: { value: 0.5 }", "- clock: 0", "- loss: 0"]
    cfg.write_text("\n".join(lines) + "\n")
    runs = {}
    for track in (False, True):
        nets = [make_net("f32") for _ in range(2)]
        with torch.no_grad():
            for p in nets[1].parameters():
                p.mul_(-0.5)
        grp = LocalGroup()
        ads = [DpwaPyTorchAdapter(nets[g], "a%d" % g, str(cfg), seed=40 + g, group=grp, track_distance=track)
               for g in range(2)]
        for r in range(3):
            for g, ad in enumerate(ads):
                ad.update_send(1.0 + g + r)
            snaps = [[p.detach().cpu().clone() for p in net.parameters()] for net in nets]
            with torch.no_grad():
                for net in nets:
                    for p in net.parameters():
                        p.add_(0.01 * (r + 1))
            hosts = [[p.detach().cpu().clone() for p in net.parameters()] for net in nets]
            DpwaPyTorchAdapter.update_wait_many(ads, [0.5 + g + r for g in range(2)])
            for g, ad in enumerate(ads):
                if not track:
                    assert ad.last_distance is None
                    continue
                want, n = model_reference(hosts[g], snaps[1 - g])
                rec = ad.last_distance.read()
                for got, w, what in ((rec.dist2, want[0], "dist2"), (rec.norm2, want[1], "norm2")):
                    assert ref.problem(got, w, n) is None, (r, g, what, ref.problem(got, w, n))
                assert rec.clock == ad.connection.clock and rec.n == ad.flat.buffer.numel() >= n
        runs[track] = ([torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu() for net in nets],
                       [ad.connection.clock for ad in ads])
        for ad in ads:
            ad.connection.close()
    for a, b in zip(runs[False][0], runs[True][0]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert runs[False][1] == runs[True][1]
