"""Healing non-finite elements inside the averaging kernel (``heal_nonfinite``, ``dpwa_average_guarded``), on
the GPU against tests/heal_ref.py: every form at the sizes where the span code takes another path (the tail
alone, exactly one span, a second span of one item and a one-element tail, the longest tail), bad elements
planted by bit pattern in the peer, in the parameters and in both; a segmented payload; two fp16 adapters."""
import ctypes

import numpy as np
import pytest
import torch

from dpwa_amd import DpwaPyTorchAdapter, _lib, dpwa
from dpwa_amd.flat import c_layout
from dpwa_amd.group import LocalGroup
from dpwa_amd.learner import Learner
from tests import forms_ref, mixed_ref
from tests import heal_ref as ref
from tests.test_gpu_distance import CASE, DEV, TORCH, bits_of, to_dev
from tests.test_gpu_finite import f16_net, interp, net_bits, write_pair_cfg
from tests.test_gpu_kernels import average_slot, ptr, stream

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements behind the payload that no launch may write
FACTOR = forms_ref.fused_factor(CASE)[0]


def record(t):
    r = _lib.HealRecord.from_buffer_copy(t.cpu().numpy().tobytes())
    return r.healed, r.refused, r.rounds, r.clock


def fused(entry, dtype, p_bits, q_bits, write_through, case=CASE, rec=None, lay=None):
    """One dpwa_average[_mixed] / dpwa_average_guarded[_mixed] on fresh buffers (bits, or bytes with a layout)
    that go on for GUARD elements behind the payload; what it wrote, on the host."""
    n = len(p_bits)
    fill = np.full(GUARD, 0xA5, dtype=p_bits.dtype)
    up = (lambda b: torch.from_numpy(np.concatenate([b, fill])).to(DEV)) if lay else \
        (lambda b: to_dev(dtype, np.concatenate([b, fill])))
    down = (lambda t: t.cpu().numpy()) if lay else (lambda t: bits_of(dtype, t))
    p, snap = up(p_bits), (up(np.zeros_like(p_bits)) if write_through else None)
    q = torch.from_numpy(q_bits).to(DEV) if lay else to_dev(dtype, q_bits)
    slot = average_slot(q, case[4], case[6])
    clock = torch.tensor([case[3], -1.0], dtype=torch.float64, device=DEV)
    coef = torch.zeros(32, dtype=torch.uint8, device=DEV)
    cfg = _lib.Interp(_lib.INTERP_CLOCK, 0, 0.0, float(case[2]))
    head = ([ctypes.byref(lay), ptr(p), ptr(slot)] if lay else [mixed_ref.CODE[dtype], ptr(p), ptr(slot), n]) + \
        [ctypes.byref(cfg), ptr(clock), float(case[5]), ptr(coef), ptr(snap) if write_through else None]
    _lib.call(entry, *head, *([ptr(rec)] if rec is not None else []), stream(), None, None)
    torch.cuda.synchronize()
    out = {"p": down(p), "snap": down(snap) if write_through else None, "coef": coef.cpu().numpy().tobytes(),
           "clock": clock.cpu().numpy().tobytes()}
    for key in ("p", "snap"):
        if out[key] is not None:
            assert (out[key][n:] == fill).all(), (entry, key, "bytes behind the payload were written")
            out[key] = out[key][:n]
    return out


@pytest.mark.parametrize("write_through", [False, True])
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_the_fused_forms_against_the_rule(dtype, write_through):
    """Plain and write-through, every size x every planting, one cumulative record: parameters and snapshot
    bit-equal to the reference (NaN bits included: bad elements are copied), coefficients and clock bit-equal
    to dpwa_average's, the counters the reference's sums; a clean input is dpwa_average's bits and counts
    nothing; a ZeroDivision round leaves parameters and counters alone and still writes the snapshot."""
    rec = torch.zeros(4, dtype=torch.int64, device=DEV)
    healed = refused = rounds = 0
    for n in ref.sizes(dtype):
        for variant in ref.VARIANTS:
            p, q = ref.inputs(dtype, n, variant)
            got = fused("dpwa_average_guarded", dtype, p, q, write_through, rec=rec)
            plain = fused("dpwa_average", dtype, p, q, write_through)
            want, h, r = ref.heal(dtype, p, q, FACTOR)
            healed, refused, rounds = healed + h, refused + r, rounds + 1
            what = (dtype, n, variant)
            print(what, "healed", h, "refused", r, record(rec))
            assert got["p"].tobytes() == want.tobytes(), (what, np.flatnonzero(got["p"] != want)[:8])
            assert not write_through or got["snap"].tobytes() == want.tobytes(), what
            assert got["coef"] == plain["coef"] and got["clock"] == plain["clock"], what
            assert record(rec) == (healed, refused, rounds, forms_ref.fused_factor(CASE)[1]), what
            if variant == "clean":
                assert (h, r) == (0, 0) and got["p"].tobytes() == plain["p"].tobytes(), what
    p, q = ref.inputs(dtype, ref.sizes(dtype)[2], "both")
    got = fused("dpwa_average_guarded", dtype, p, q, write_through, case=forms_ref.ZERO_DIVISION, rec=rec)
    assert _lib.Coef.from_buffer_copy(got["coef"]).status == _lib.STATUS_ZERO_DIVISION
    assert got["p"].tobytes() == p.tobytes() and (not write_through or got["snap"].tobytes() == p.tobytes())
    assert record(rec)[:3] == (healed, refused, rounds)


def learner_rounds(form, dtype, pq, heal):
    """Rounds (p, q) of a learner that fetches q from a peer, `form` "split" (factor, then the lerp with
    device coefficients) or "resident": what each round left."""
    n = len(pq[0][0])
    me, peer = Learner(DEV, n, TORCH[dtype], interp()), Learner(DEV, n, TORCH[dtype], interp())
    me.attach_local(0, peer)
    me.set_heal(heal)
    me.write_clock(3.0)
    flat, s, out = torch.zeros(n, dtype=TORCH[dtype], device=DEV), torch.cuda.current_stream(), []
    if form == "resident":
        _lib.call("dpwa_learner_set_resident", me.handle, ptr(flat), stream())
    for p, q in pq:
        peer.publish(to_dev(dtype, q), 1.0, s)
        if form == "resident":
            flat = me.resident_params()
            flat.copy_(to_dev(dtype, p))
            me.publish(flat, 1.0, s)
            flat = me.resident_params()
        else:
            flat.copy_(to_dev(dtype, p))
        me.fetch(0, peer.version, False, s)
        if form == "split":
            me.factor(1.0, s)
            me.lerp(flat, s)
        else:
            me.average(flat, 1.0, s)
            flat = me.resident_params()
        out.append({"r": bits_of(dtype, flat), "coef": bytes(me.read_coef()), "clock": me.read_clock(),
                    "rec": me.heal_record()})
    torch.cuda.synchronize()
    me.close(), peer.close()
    return out


@pytest.mark.parametrize("form", ["split", "resident"])
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_device_coefficients_and_the_resident_form(dtype, form):
    """Two rounds back to back per size on a healing learner: the parameters (resident: the next slot) against
    the rule at the round's own factor, coefficients and clock bit-equal to the same rounds with the switch off,
    the record accumulating over the rounds."""
    for n in ref.sizes(dtype):
        pq = [ref.inputs(dtype, n, "both"), ref.inputs(dtype, n, "p", seed=5)]
        on, off = learner_rounds(form, dtype, pq, True), learner_rounds(form, dtype, pq, False)
        healed = refused = 0
        for k, ((p, q), a, b) in enumerate(zip(pq, on, off)):
            assert a["coef"] == b["coef"] and a["clock"] == b["clock"], (dtype, form, n, k)
            want, h, r = ref.heal(dtype, p, q, _lib.Coef.from_buffer_copy(a["coef"]).factor)
            healed, refused = healed + h, refused + r
            assert a["r"].tobytes() == want.tobytes(), (dtype, form, n, k, np.flatnonzero(a["r"] != want)[:8])
            assert a["rec"] == (healed, refused, k + 1, a["clock"]) and b["rec"] == (0, 0, 0, 0.0), (dtype, form, n, k)
        assert healed and refused


@pytest.mark.parametrize("write_through", [False, True])
def test_a_segmented_payload(write_through):
    """{fp32: one 4-KiB block, fp16: one block}, a bad element in the first and the last word of each segment,
    in the peer, the parameters and both: each segment by its own type's test and lerp."""
    spec = [("f32", 1024), ("f16", 2048)]
    segs, total = mixed_ref.segments(spec)
    lay = c_layout(tuple((TORCH[d], off, length) for d, off, length, _ in segs))
    p, q = np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=np.uint8)
    for k, (d, off, length, n) in enumerate(segs):
        pe, qe = ref.normal(d, n, 40 + k), ref.normal(d, n, 50 + k)
        nan, inf = ref.BAD[d]["qnan"], ref.BAD[d]["-inf"]
        qe[0], pe[1], pe[2], qe[2] = nan, inf, nan, inf                  # the first word: refused, healed, both
        qe[n - 1], pe[n - 2], pe[n - 3], qe[n - 3] = inf, nan, inf, nan  # the last word
        p[off:off + length], q[off:off + length] = pe.view(np.uint8), qe.view(np.uint8)
    rec = torch.zeros(4, dtype=torch.int64, device=DEV)
    got = fused("dpwa_average_guarded_mixed", None, p, q, write_through, rec=rec, lay=lay)
    plain = fused("dpwa_average_mixed", None, p, q, write_through, lay=lay)
    want, healed, refused = np.zeros(total, dtype=np.uint8), 0, 0
    for seg in segs:
        r, h, f = ref.heal(seg[0], mixed_ref.elements(p, seg), mixed_ref.elements(q, seg), FACTOR)
        want[seg[1]:seg[1] + seg[2]] = r.view(np.uint8)
        healed, refused = healed + h, refused + f
    assert got["p"].tobytes() == want.tobytes() and (not write_through or got["snap"].tobytes() == want.tobytes())
    assert got["coef"] == plain["coef"] and got["clock"] == plain["clock"]
    assert record(rec)[:3] == (healed, refused, 1) and (healed, refused) == (4, 8)


def test_two_fp16_adapters_one_all_nan(tmp_path):
    """a0's model is all NaN, a1's finite; one round.  Healing: every parameter of a0 has a1's bits and
    healed == N, a1 took nothing and refused == N.  With the option off a0 stays NaN and a1 becomes NaN."""
    for on in (True, False):
        cfg = tmp_path / ("heal_%d.yaml" % on)
        write_pair_cfg(cfg, "constant")
        nets, grp = [f16_net(90), f16_net(91)], LocalGroup()
        with torch.no_grad():
            for p in nets[0].parameters():
                p.fill_(float("nan"))
        ads = [DpwaPyTorchAdapter(nets[g], "a%d" % g, str(cfg), seed=95 + g, group=grp,
                                  **({"heal_nonfinite": True} if on else {})) for g in range(2)]
        peer, count = net_bits(nets[1]), sum(p.numel() for p in nets[1].parameters())
        for ad in ads:
            ad.update_send(1.0)
        for ad in ads:
            ad.update_wait(1.0)
        torch.cuda.synchronize()
        for g in range(2):
            for got, w in zip(net_bits(nets[g]), peer):
                assert (got.tobytes() == w.tobytes()) if on else bool(forms_ref.is_nan("f16", got).all()), (on, g)
        elems = [ad.nonfinite_elements for ad in ads]
        assert [e[:3] for e in elems] == ([(count, 0, 1), (0, count, 1)] if on else [(0, 0, 0)] * 2)
        for ad in ads:
            ad.close()


def test_the_refusals_by_their_messages(tmp_path):
    """Unaligned parameters (average and lerp), the fused relay phase on a healing learner and the switch while
    one is pending are refused by name with nothing queued; relay-avg at bind."""
    n, lib = 4096, _lib.load()
    me, peer = Learner(DEV, n, torch.float32, interp()), Learner(DEV, n, torch.float32, interp())
    me.attach_local(0, peer)
    me.set_heal(True)
    base, s = torch.zeros(n + 4, device=DEV), torch.cuda.current_stream()
    peer.publish(base[:n], 1.0, s)
    me.fetch(0, peer.version, False, s)
    assert lib.dpwa_learner_average(me.handle, ptr(base[1:n + 1]), 1.0, None, stream()) == _lib.ERR_ARG
    assert b"dpwa_learner_average" in lib.dpwa_last_error() and b"dpwa_learner_set_heal" in lib.dpwa_last_error()
    me.factor(1.0, s)
    assert lib.dpwa_learner_lerp(me.handle, ptr(base[1:n + 1]), stream()) == _lib.ERR_ARG
    assert b"dpwa_learner_lerp" in lib.dpwa_last_error() and b"16-byte aligned" in lib.dpwa_last_error()
    me.lerp(base[:n], s)
    _lib.call("dpwa_learner_relay_enable", me.handle, 2, 0)
    picks = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    assert lib.dpwa_learner_relay_phase2(me.handle, ptr(picks), 1, 1, 1, 1) == _lib.ERR_STATE
    assert b"dpwa_learner_relay_phase2" in lib.dpwa_last_error() and b"dpwa_learner_set_heal" in lib.dpwa_last_error()
    assert me.heal_record() == (0, 0, 1, me.read_clock())
    torch.cuda.synchronize()
    me.close(), peer.close()
    cfg = tmp_path / "relay.yaml"
    write_pair_cfg(cfg)
    conn = dpwa.DpwaConnection("a0", str(cfg), seed=1, group=LocalGroup(), heal_nonfinite=True)
    conn._pull = "relay-avg"                         # (what a group's default would make it before the bind)
    with pytest.raises(ValueError) as err:
        conn.update_send(torch.zeros(64, device=DEV), 1.0)
    assert str(err.value) == dpwa.HEAL_RELAY_AVG
    conn.close()
