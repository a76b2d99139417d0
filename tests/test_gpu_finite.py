"""Skipping a round whose peer snapshot holds a NaN or an inf (``skip_nonfinite_peer``,
``dpwa_learner_set_finite_check``), on the GPU: the pass alone against tests/finite_ref.py's bit-pattern
rule at every edge size and alignment; a learner's rounds in every averaging form (a skipped round
changes nothing and is counted, the round after and an all-finite run are bit-equal to the switch
off); the adapter against a host model; the relay-avg refusals.

Shapes are the smallest at which each case can go wrong: a lane's item is 4 fp32 / 8 16-bit elements,
a one-wave span 256 / 512; 100,003 elements have many spans and a tail."""
import ctypes

import numpy as np
import pytest
import torch

from dpwa_amd import DpwaConnection, DpwaPyTorchAdapter, _lib
from dpwa_amd.flat import c_layout
from dpwa_amd.group import LocalGroup
from dpwa_amd.learner import Learner
from tests import dist_ref, f16_ref, mixed_ref
from tests import finite_ref as ref
from tests.test_gpu_distance import learner_record, to_dev
from tests.test_gpu_kernels import ptr, stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TORCH = mixed_ref.TORCH
SENTINEL = 0x5a5a5a5a            # what a veto word holds before a launch: never a stamp used here


def stamp_of(i):
    return (0x9e3779b9 * (i + 1)) & 0xffffffff or 1           # all 32 bits in use, never 0


# ---------------------------------------------------------------- 1. the pass alone
def check_words(words, cases, what):
    got = words.cpu().numpy().view(np.uint32)
    for i, (name, _, want) in enumerate(cases):
        expect = stamp_of(i) if want else SENTINEL
        assert got[i] == expect, (what, name, "vetoed" if got[i] == stamp_of(i) else hex(got[i]), "want veto" if want else "want none")


@pytest.mark.parametrize("dtype,n", [(d, n) for d in ref.DTYPES for n in ref.sizes(d)])
def test_the_pass_alone(dtype, n):
    """dpwa_check_finite on every input of tests/finite_ref.py -- a quiet NaN, a signalling NaN, +inf
    and -inf in the first element, the last of the last full span, the last of the tail and an odd and
    an even half of a dword; non-finite values just past n; the largest finite values, subnormals,
    signed zeros, 16-bit infinities in fp32 low halves -- 16-byte aligned and 4 bytes off: the veto
    word holds the stamp exactly when the reference says so and is untouched otherwise."""
    cases = ref.cases(dtype, n)
    for shift in (0, 4 // ref.SIZE[dtype]):
        words = torch.full((len(cases),), SENTINEL, dtype=torch.int32, device=DEV)
        keep = []
        for i, (name, bits, want) in enumerate(cases):
            buf = to_dev(dtype, np.concatenate([np.zeros(shift, dtype=bits.dtype), bits]))
            keep.append(buf)
            assert buf.data_ptr() % 16 == 0
            payload = ctypes.c_void_p(buf.data_ptr() + shift * ref.SIZE[dtype])
            _lib.call("dpwa_check_finite", ref.CODE[dtype], payload, n, ctypes.c_void_p(words.data_ptr() + 4 * i),
                      stamp_of(i), stream(), None, None)
        torch.cuda.synchronize()
        check_words(words, cases, (dtype, n, "shift %d" % shift))


@pytest.mark.parametrize("name", sorted(ref.MIXED))
def test_the_pass_alone_on_a_segmented_payload(name):
    """dpwa_check_finite_mixed: a bad element in the first and the last element of every segment vetoes;
    16-bit infinities in the low halves of the fp32 segment, the zero padding and an all-zero payload
    do not."""
    segs, total, cases = ref.mixed_cases(ref.MIXED[name])
    lay = c_layout(tuple((TORCH[d], off, length) for d, off, length, _ in segs))
    words = torch.full((len(cases),), SENTINEL, dtype=torch.int32, device=DEV)
    keep = []
    for i, (_, payload, _) in enumerate(cases):
        buf = torch.from_numpy(payload.copy()).to(DEV)
        keep.append(buf)
        _lib.call("dpwa_check_finite_mixed", ctypes.byref(lay), ptr(buf), ctypes.c_void_p(words.data_ptr() + 4 * i),
                  stamp_of(i), stream(), None, None)
    torch.cuda.synchronize()
    check_words(words, cases, name)


def test_a_timed_launch_and_an_empty_payload():
    """Events as dpwa_average: the pass is timed by its own dispatch; n = 0 launches nothing."""
    n = 3 * ref.SPAN["f32"] + 5
    bits = ref.cases("f32", n)[1][1]
    buf, word = to_dev("f32", bits), torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(), b.record()          # created
    _lib.call("dpwa_check_finite", _lib.F32, ptr(buf), n, ptr(word), 7, stream(), ctypes.c_void_p(a.cuda_event),
              ctypes.c_void_p(b.cuda_event))
    _lib.call("dpwa_check_finite", _lib.F32, ptr(buf), 0, ctypes.c_void_p(word.data_ptr() + 4), 7, stream(), None, None)
    torch.cuda.synchronize()
    assert word.cpu().tolist() == [7, SENTINEL] and a.elapsed_time(b) >= 0.0


# ---------------------------------------------------------------- 2. rounds on a learner
FORMS = [(f, d) for f in ("plain", "write-through", "resident", "split") for d in ref.DTYPES] + \
        [("mixed", "mixed"), ("unaligned", "f32")]
SPEC = ref.MIXED["three-types"]


def interp():
    return _lib.Interp(_lib.INTERP_CLOCK, 0, 0.0, 0.0)


def noise(dtype, seed):
    """Finite random bits of a rig's payload: (bits or bytes)."""
    if dtype == "mixed":
        return ref.mixed_cases(SPEC, seed)[2][0][1]
    return ref.finite_noise(dtype, 3 * ref.SPAN[dtype] + 5, seed)


def poisoned(dtype, seed):
    """The same with one non-finite element: the last of the tail, or the last bf16 of its segment."""
    if dtype == "mixed":
        cases = {name: payload for name, payload, _ in ref.mixed_cases(SPEC, seed)[2]}
        return cases["bf16-+inf-last"]
    bits = noise(dtype, seed).copy()
    bits[-1] = ref.BAD[dtype]["snan" if seed % 2 else "-inf"]
    return bits


class Rig:
    """A learner `me` and the peer it fetches from, one averaging form; round(q, p) publishes q as the
    peer's snapshot, makes p the parameters and averages (or, average=False, is a round without a
    fetch), and returns what the round left."""

    def __init__(self, form, dtype, check):
        self.form, self.dtype = form, dtype
        lay = None
        if dtype == "mixed":
            segs, n = mixed_ref.segments(SPEC)
            lay = tuple((TORCH[d], off, length) for d, off, length, _ in segs)
            self.tdtype = torch.uint8
        else:
            n = 3 * ref.SPAN[dtype] + 5
            self.tdtype = TORCH[dtype]
        self.n = n
        self.me = Learner(DEV, n, self.tdtype, interp(), layout=lay)
        self.peer = Learner(DEV, n, self.tdtype, interp(), layout=lay)
        self.me.attach_local(0, self.peer)
        if check:
            self.me.set_finite_check(True)
        self.qbuf = torch.zeros(n, dtype=self.tdtype, device=DEV)
        self.base = torch.zeros(n + 4, dtype=self.tdtype, device=DEV)
        self.flat = self.base[1:1 + n] if form == "unaligned" else self.base[:n]
        assert self.flat.data_ptr() % 16 == (4 if form == "unaligned" else 0)
        self.through = form in ("write-through", "mixed")
        if form == "resident":
            _lib.call("dpwa_learner_set_resident", self.me.handle, ptr(self.flat), stream())

    def dev(self, bits):
        return torch.from_numpy(bits.copy()).to(DEV) if self.dtype == "mixed" else to_dev(self.dtype, bits)

    def snapshot(self):
        out = np.full(self.n * self.flat.element_size(), 0xEE, dtype=np.uint8)
        hdr, v = ctypes.create_string_buffer(256), ctypes.c_uint64()
        _lib.call("dpwa_learner_read_snapshot", self.me.handle, hdr, ctypes.c_void_p(out.ctypes.data), out.nbytes,
                  ctypes.byref(v))
        return out.tobytes()

    def round(self, q, p, average=True):
        me, s = self.me, torch.cuda.current_stream()
        self.qbuf.copy_(self.dev(q))
        self.peer.publish(self.qbuf, 1.0, s)
        flat = self.flat
        if self.form == "resident":          # publish, then average: the parameters are the served snapshot
            flat = me.resident_params()
            flat.copy_(self.dev(p))
            me.publish(flat, 1.0, s)
            flat = me.resident_params()
        else:
            flat.copy_(self.dev(p))
        before = me.read_clock()
        if average:
            me.fetch(0, self.peer.version, False, s)
            if self.form == "split":
                me.factor(1.0, s)
                me.lerp(flat, s)
            elif self.through:
                _lib.call("dpwa_learner_average_through", me.handle, ptr(flat), 1.0, None, ctypes.c_void_p(s.cuda_stream))
            else:
                me.average(flat, 1.0, s)
        if self.form == "resident":
            flat = me.resident_params()
        out = {"before": before, "clock": me.read_clock(), "coef": bytes(me.read_coef()), "word": me._status.value,
               "skips": me.finite_skips(), "flat": flat.cpu().view(torch.uint8).numpy().tobytes(), "snap": None}
        if self.through:                     # what the average wrote through, made the published snapshot
            fn = "dpwa_learner_publish_reuse" if average else "dpwa_learner_publish"
            _lib.call(fn, me.handle, ptr(flat), 1.0, None, ctypes.c_void_p(s.cuda_stream))
            me.version += 1
            torch.cuda.synchronize()
            out["snap"] = self.snapshot()
        return out

    def close(self):
        torch.cuda.synchronize()
        self.me.close()
        self.peer.close()


def as_bytes(bits):
    return np.ascontiguousarray(bits).view(np.uint8).tobytes()


SAME = ("flat", "snap", "clock", "coef")


@pytest.mark.parametrize("form,dtype", FORMS)
def test_a_skipped_round_and_the_round_after(form, dtype):
    """Rounds finite, non-finite, finite with the switch on.  The middle round leaves the parameters
    bit-equal, the write-through / resident snapshot equal to them and the clock where it was, reports
    status 2 with the no-op's coefficients, leaves the sticky status word 0 and counts one skip.  The
    round after is bit-equal to the same round of a learner with the switch off whose middle round had
    no fetch: the stamp of the skipped round vetoes nothing any more."""
    q = [noise(dtype, 10), poisoned(dtype, 11), noise(dtype, 12)]
    p = [noise(dtype, 20), noise(dtype, 21), noise(dtype, 22)]
    on, off = Rig(form, dtype, True), Rig(form, dtype, False)
    got = [on.round(q[r], p[r]) for r in range(3)]
    want = [off.round(q[r], p[r], average=r != 1) for r in range(3)]
    mid = got[1]
    coef = _lib.Coef.from_buffer_copy(mid["coef"])
    assert mid["flat"] == as_bytes(p[1]), "a skipped round changed the parameters"
    if mid["snap"] is not None:
        assert mid["snap"] == mid["flat"], "the write-through snapshot of a skipped round is not the parameters"
    assert mid["clock"] == mid["before"] == got[0]["clock"] + (1.0 if form == "resident" or on.through else 0.0)
    assert (coef.status, coef.factor, coef.a, coef.b, coef.new_clock) == (_lib.STATUS_PEER_NONFINITE, 0.0, 0.0, 1.0, mid["before"])
    assert mid["word"] == 0 and on.me.take_status() == 0
    assert [g["skips"] for g in got] == [0, 1, 1] and [w["skips"] for w in want] == [0, 0, 0]
    for r in (0, 2):
        for key in SAME:
            assert got[r][key] == want[r][key], (form, dtype, r, key)
        assert _lib.Coef.from_buffer_copy(got[r]["coef"]).status == _lib.STATUS_OK
        assert got[r]["flat"] != as_bytes(p[r]), "a finite round must average"
    on.close(), off.close()


@pytest.mark.parametrize("form,dtype", FORMS)
def test_six_finite_rounds_are_bit_equal_to_the_switch_off(form, dtype):
    on, off = Rig(form, dtype, True), Rig(form, dtype, False)
    for r in range(6):
        q, p = noise(dtype, 30 + r), noise(dtype, 40 + r)
        a, b = on.round(q, p), off.round(q, p)
        for key in SAME + ("word", "skips"):
            assert a[key] == b[key], (form, dtype, r, key)
        assert a["skips"] == 0 and _lib.Coef.from_buffer_copy(a["coef"]).status == _lib.STATUS_OK
    on.close(), off.close()


def test_a_zero_division_round_stays_one():
    """Clock interpolation with both clocks 0 and a NaN peer: ZeroDivision keeps precedence -- status 1,
    the sticky word set (Python raises on it as before), no skip counted."""
    rig = Rig("plain", "f32", True)
    rig.peer.write_clock(-1.0)                       # its publish serves clock 0
    out = rig.round(poisoned("f32", 11), noise("f32", 21))
    assert _lib.Coef.from_buffer_copy(out["coef"]).status == _lib.STATUS_ZERO_DIVISION
    assert out["word"] == _lib.STATUS_ZERO_DIVISION and out["skips"] == 0 and out["flat"] == as_bytes(noise("f32", 21))
    assert rig.me.take_status() == _lib.STATUS_ZERO_DIVISION and rig.me.take_status() == 0
    rig.close()


@pytest.mark.parametrize("form", ["plain", "split", "unaligned"])
def test_a_skipped_round_leaves_the_distance_record(form):
    """With the whole-model distance on (the tracked kernel; the stand-alone pass before a split or an
    unaligned average): a skipped round leaves the record's bytes, and the round after reports only
    its own sums."""
    rig = Rig(form, "f32", True)
    _lib.call("dpwa_learner_set_distance", rig.me.handle, 1)
    n = rig.n
    q, p = [noise("f32", 50), poisoned("f32", 51), noise("f32", 52)], [noise("f32", 60 + r) for r in range(3)]
    rig.round(q[0], p[0])
    first = bytes(learner_record(rig.me))
    assert rig.round(q[1], p[1])["skips"] == 1
    assert bytes(learner_record(rig.me)) == first
    out = rig.round(q[2], p[2])
    rec, want = learner_record(rig.me), dist_ref.reference("f32", p[2], q[2])
    for got, w in ((rec.dist2, want[0]), (rec.norm2, want[1])):
        assert dist_ref.problem(got, w, n) is None, (form, dist_ref.problem(got, w, n))
    assert rec.clock == out["clock"] and rec.n == n
    rig.close()


def write_pair_cfg(path, interp="clock"):
    lines = ["- nodes:", "  - {name: a0, host: localhost, port: 46300}", "  - {name: a1, host: localhost, port: 46301}",
             "- fetch_probability: 1.0", "- timeout_ms: 2500", "- interpolation: %s" % interp, "- divergence_threshold: 0",
             "- constant: { value: 0.5 }", "- clock: 0", "- loss: 0"]
    path.write_text("\n".join(lines) + "\n")


@pytest.mark.parametrize("resident", [False, True])
def test_two_learners_in_one_dispatch_one_peer_poisoned(tmp_path, resident):
    """a0 and a1 average with each other through update_wait_average_many (one batched dispatch; resident:
    the mutual pair's kernel) and a1's parameters are NaN: a0 is skipped and unchanged, a1 averages with
    status OK and is still NaN (it is not healed); nothing raises, then or at the next call."""
    cfg = tmp_path / "pair.yaml"
    write_pair_cfg(cfg)
    n = 3 * ref.SPAN["f32"] + 5
    grp = LocalGroup()
    conns = [DpwaConnection("a%d" % g, str(cfg), seed=70 + g, group=grp, skip_nonfinite_peer=True) for g in range(2)]
    good = ref.finite_noise("f32", n, 80)
    flats = [to_dev("f32", good), torch.full((n,), float("nan"), device=DEV)]
    if resident:
        flats = [c.make_resident(f) for c, f in zip(conns, flats)]
    for r in range(2):
        for c, f in zip(conns, flats):
            c.update_send(f, 1.0)
        if resident:
            flats = [c.parameters for c in conns]
        res = DpwaConnection.update_wait_average_many(conns, flats, [1.0, 1.0], write_through=False)
        assert all(payload is not None for payload, _ in res)
        if resident:
            flats = [c.parameters for c in conns]
        torch.cuda.synchronize()
        assert flats[0].cpu().view(torch.uint8).numpy().tobytes() == as_bytes(good), (r, "a0 took from a NaN peer")
        assert bool(torch.isnan(flats[1]).all()), (r, "a1 is not healed")
        st = [c._learner.read_coef().status for c in conns]
        assert st == [_lib.STATUS_PEER_NONFINITE, _lib.STATUS_OK], (r, st)
        assert [c.nonfinite_skips for c in conns] == [r + 1, 0]
    for c in conns:
        c.synchronize()                  # raises a pending ZeroDivisionError: there is none
        c.close()


# ---------------------------------------------------------------- 3. the adapter
def f16_net(seed):
    g = torch.Generator().manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.Linear(17, 5))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    return net.half().to(DEV)


def net_bits(net):
    return [f16_ref.as_u16(p.detach().cpu()).reshape(-1).copy() for p in net.parameters()]


def gossip(tmp_path, skip):
    """Two fp16 adapters that average with each other, constant factor 0.5: one healthy round, then a1
    is filled with inf and three more rounds.  Returns a0's parameters after every round, the host
    model's, both skip counts and the model's."""
    cfg = tmp_path / ("gossip_%d.yaml" % skip)
    write_pair_cfg(cfg, "constant")
    nets = [f16_net(90), f16_net(91)]
    grp = LocalGroup()
    kwargs = {"skip_nonfinite_peer": True} if skip else {}
    ads = [DpwaPyTorchAdapter(nets[g], "a%d" % g, str(cfg), seed=95 + g, group=grp, **kwargs) for g in range(2)]
    model, model_skips, seen, want = net_bits(nets[0]), 0, [], []
    for r in range(4):
        if r == 1:
            with torch.no_grad():
                for p in nets[1].parameters():
                    p.fill_(float("inf"))
        for ad in ads:
            ad.update_send(1.0)
        peer = net_bits(nets[1])                                # what a1 published
        with torch.no_grad():                                   # a0's training step: exact in fp16
            for p in nets[0].parameters():
                p.mul_(0.5)
        model = [f16_ref.as_u16(f16_ref.as_half(m) * 0.5) for m in model]
        for ad in ads:
            ad.update_wait(1.0)
        if any(ref.vetoes("f16", q) for q in peer):             # the whole snapshot is one payload
            model_skips += 1
        else:
            model = [f16_ref.torch_lerp(m, q, 0.5) for m, q in zip(model, peer)]
        torch.cuda.synchronize()
        seen.append(net_bits(nets[0]))
        want.append([m.copy() for m in model])
    skips = [ad.nonfinite_skips for ad in ads]
    for ad in ads:
        ad.connection.synchronize()
        ad.close()
    return seen, want, skips, model_skips


def test_two_fp16_adapters_after_one_overflowed(tmp_path):
    """With the switch the healthy adapter's trajectory is the host model's (tests/f16_ref.py: the first
    round averages, the three after it are skipped) bit for bit, and it counted the model's skips;
    without the switch the same loop ends non-finite."""
    seen, want, skips, model_skips = gossip(tmp_path, True)
    assert model_skips == 3 and skips == [3, 0]
    for r, (got, w) in enumerate(zip(seen, want)):
        for t, (a, b) in enumerate(zip(got, w)):
            assert f16_ref.same(a, b), (r, t, f16_ref.mismatches(a, b))
            assert not ref.vetoes("f16", a), (r, t)
    seen, _, skips, _ = gossip(tmp_path, False)
    assert skips == [0, 0]
    assert all(ref.nonfinite("f16", a).all() for a in seen[-1]), "without the switch the inf must have spread"


def test_the_connection_counts_and_does_not_raise(tmp_path):
    """update_wait() + average(), the reference's seam: the factor of a skipped round is 0, average()
    leaves the parameters alone, nonfinite_skips counts it, and no later call raises."""
    cfg = tmp_path / "seam.yaml"
    write_pair_cfg(cfg)
    n = 1541
    grp = LocalGroup()
    conns = [DpwaConnection("a%d" % g, str(cfg), seed=75 + g, group=grp, skip_nonfinite_peer=True) for g in range(2)]
    good = ref.finite_noise("f32", n, 81)
    flats = [to_dev("f32", good), torch.full((n,), float("inf"), device=DEV)]
    for c, f in zip(conns, flats):
        c.update_send(f, 1.0)
    payload, factor = conns[0].update_wait(1.0)
    assert payload is not None and float(factor) == 0.0
    conns[0].average(flats[0])
    conns[0].update_send(flats[0], 1.0)              # the next call: nothing pending
    conns[0].synchronize()
    assert flats[0].cpu().view(torch.uint8).numpy().tobytes() == as_bytes(good)
    assert conns[0].nonfinite_skips == 1 and conns[0]._learner.read_coef().status == _lib.STATUS_PEER_NONFINITE
    for c in conns:
        c.close()


# ---------------------------------------------------------------- 4. the refusals
def test_checking_refuses_the_fused_relay_phase():
    """dpwa_learner_relay_phase2(fuse != 0) on a checking learner is DPWA_ERR_STATE (the fused second
    phase has no contiguous peer snapshot), before any relay work is queued; with the switch off again
    the same call is past that refusal."""
    me = Learner(DEV, 4096, torch.float32, interp())
    me.set_finite_check(True)
    _lib.call("dpwa_learner_relay_enable", me.handle, 2, 0)
    picks = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    lib = _lib.load()
    assert lib.dpwa_learner_relay_phase2(me.handle, ptr(picks), 1, 1, 1, 1) == _lib.ERR_STATE
    assert b"dpwa_learner_relay_phase2" in lib.dpwa_last_error() and b"set_finite_check" in lib.dpwa_last_error()
    me.close()


def test_bind_refuses_relay_avg(tmp_path):
    """A connection whose pull became relay-avg behind set_pull's back is refused when it binds."""
    cfg = tmp_path / "bind.yaml"
    write_pair_cfg(cfg)
    conn = DpwaConnection("a0", str(cfg), seed=1, group=LocalGroup(), skip_nonfinite_peer=True)
    conn._pull = "relay-avg"
    with pytest.raises(ValueError) as err:
        conn.update_send(torch.zeros(64, device=DEV), 1.0)
    assert "relay-avg" in str(err.value) and "skip_nonfinite_peer" in str(err.value)
    conn.close()
