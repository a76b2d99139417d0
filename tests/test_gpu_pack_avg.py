"""The average straight from a packed image (dpwa_average_packed, pull 'packed-avg') against the host model:
tests/pack_ref.roundtrip for what the peer's payload becomes, then the project's host lerp of that dtype.  NaN
positions equal, everything else bit-equal."""
import ctypes

import numpy as np
import pytest

from tests import f16_ref, helpers
from tests import pack_ref as ref
from tests.test_gpu_pack import CODE, GUARD, hard_payload

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
BITS = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16}


def host_lerp(dtype, p_bits, q_bits, f):
    from oracle import lerp as olerp
    if dtype == "f32":
        return olerp.lerp_f32(p_bits.view(np.float32), q_bits.view(np.float32), f).view(np.uint32)
    return olerp.lerp_bf16(p_bits, q_bits, f) if dtype == "bf16" else f16_ref.numpy_lerp(p_bits, q_bits, f)


def same(dtype, got, want):
    """NaN positions equal, every other element's bits equal (uint8 payloads)."""
    gn, wn = np.isnan(ref.widen(got, dtype)), np.isnan(ref.widen(want, dtype))
    return np.array_equal(gn, wn) and np.array_equal(got.view(BITS[dtype])[~gn], want.view(BITS[dtype])[~wn])


def average(dtype, n32, cfg, loss, write_through, fused):
    """One round on fresh guarded buffers: (parameters before, peer payload, parameters after, snapshot, coef,
    new clock), the first two and the results as host bytes.  `fused`: dpwa_average_packed on the image dpwa_pack
    made; else dpwa_unpack into a slot and dpwa_average from it."""
    import torch
    from dpwa_amd import _lib
    nbytes = 4 * n32
    n, dev, s = nbytes // ref.SIZE[dtype], torch.device("cuda", 0), _lib.stream_handle(None)
    payload = hard_payload(dtype, nbytes)
    before = ref.narrow(np.random.default_rng(7 * n32).standard_normal(n), dtype)

    def guarded(size, body=None):
        t = torch.full((size + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
        if body is not None:
            t[:len(body)] = torch.from_numpy(np.frombuffer(body, np.uint8).copy()).to(dev)
        return t

    def ptr(t, at=0):
        return ctypes.c_void_p(t.data_ptr() + at)

    size = ctypes.c_int64()
    _lib.call("dpwa_pack_bytes", CODE[dtype], n, ctypes.byref(size))
    off = _lib.SLOT_PAYLOAD_OFFSET
    src, img, p, snap = guarded(nbytes, payload), guarded(size.value), guarded(nbytes, before), guarded(nbytes)
    slot = guarded(off + nbytes, bytes(_lib.Header(5.0, 0.0, 1, n, CODE[dtype])))   # the peer's header; payload at `off`
    clock = torch.tensor([2.0, -1.0], dtype=torch.float64, device=dev)
    coef = torch.zeros(32, dtype=torch.uint8, device=dev)
    _lib.call("dpwa_pack", CODE[dtype], ptr(src), n, ptr(img), s, None, None)
    tail = (ctypes.byref(cfg), ptr(clock), loss, ptr(coef), ptr(snap) if write_through else None, s, None, None)
    if fused:
        _lib.call("dpwa_average_packed", CODE[dtype], ptr(p), ptr(slot), ptr(img), n, *tail)
    else:
        _lib.call("dpwa_unpack", CODE[dtype], ptr(img), n, ptr(slot, off), 512, s, None, None)
        _lib.call("dpwa_average", CODE[dtype], ptr(p), ptr(slot), n, *tail)
    torch.cuda.synchronize()
    for t in (src, img, p, snap, slot):
        assert (t.cpu().numpy()[-GUARD:] == 0xFF).all(), "bytes behind a buffer were written"
    return (before, payload, p.cpu().numpy()[:nbytes], snap.cpu().numpy()[:nbytes], coef.cpu().numpy().tobytes(),
            clock[1].item())


@pytest.mark.parametrize("factor", [0.5, 1.0 - 2.0 ** -20])
@pytest.mark.parametrize("n32", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 1])
@pytest.mark.parametrize("write_through", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_average_packed_is_the_host_model(dtype, write_through, n32, factor):
    from dpwa_amd import _lib
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, factor, 0.0)
    before, payload, got, snap, coef, clock = average(dtype, n32, cfg, 1.0, write_through, True)
    peer = ref.roundtrip(payload, dtype)
    want = host_lerp(dtype, before.view(BITS[dtype]), peer.view(BITS[dtype]), factor).view(np.uint8)
    assert same(dtype, got, want), "the parameters"
    assert not write_through or np.array_equal(snap, got), "the write-through snapshot"
    assert (coef, clock) == average(dtype, n32, cfg, 1.0, write_through, False)[4:], "dpwa_average's coef and clock"
    assert _lib.Coef.from_buffer_copy(coef).status == 0 and clock == factor * 5.0 + (1.0 - factor) * 2.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_op_round_still_writes_the_snapshot(dtype):
    """Loss interpolation with both losses 0 (ZeroDivisionError in the reference): parameters and clock stay,
    the write-through snapshot receives the parameters, the ragged item included."""
    from dpwa_amd import _lib
    cfg = _lib.Interp(_lib.INTERP_LOSS, 0, 0.0, 0.0)
    before, _, got, snap, coef, clock = average(dtype, 1025, cfg, 0.0, True, True)
    assert _lib.Coef.from_buffer_copy(coef).status == _lib.STATUS_ZERO_DIVISION and clock == 2.0
    assert np.array_equal(got, before) and np.array_equal(snap, before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_equals_unpack_then_average(dtype):
    """Byte for byte, NaN bits included: both paths run the same instructions on the same values."""
    from dpwa_amd import _lib
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 1.0 - 2.0 ** -20, 0.0)
    fused, two = (average(dtype, 3 * 1024 + 1, cfg, 1.0, True, f) for f in (True, False))
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(fused, two))


@pytest.mark.parametrize("dtype,fds,resident", [("f16", False, False), ("f32", False, False), ("f16", True, False),
                                                ("f32", True, False), ("f32", False, True)])
def test_lockstep_group_walks_both_packed_modes(tmp_path, monkeypatch, dtype, fds, resident):
    """Two ranks under a DistGroup walk pack_avg_worker.PULLS: every round's parameters, clocks and peers equal
    oracle.gossip.simulate's, whose fetched payload every packed round replaces by pack_ref.roundtrip of it; the
    last round's tracked distance on rank 0 is within dist_ref's bound of the host's.  The fused rounds, and they
    alone, leave the staging payload as it was."""
    from oracle import gossip as ogossip
    from oracle import lerp as olerp
    from tests import dist_ref, dist_worker, group_ref, pack_avg_worker as worker
    from tests.test_gpu_group_dtypes import free_port, run_job
    if fds:
        helpers.need_fd_sharing()
        monkeypatch.setenv("DPWA_VMM", "1")
    cfg = str(tmp_path / "pack.yaml")
    dist_worker.write_cfg(cfg, worker.NAMES, 1, "clock", 0.0)
    reports = run_job("packed-avg-%s" % dtype, 2, worker.walk_main, (dtype, resident, free_port(), cfg, str(tmp_path)))
    assert reports == {0: ("ok", worker.T), 1: ("ok", worker.T)}, reports
    plain = olerp.lerp_f32 if dtype == "f32" else group_ref.lerp("f16")
    calls = []

    def lerp(param, peer, factor):      # fetch_probability 1: both ranks average in every round, in order
        if worker.PULLS[len(calls) // 2].startswith("packed"):
            raw = ref.roundtrip(np.ascontiguousarray(peer).view(np.uint8), dtype)
            peer = raw.view(np.float32 if dtype == "f32" else np.uint16)
        calls.append((param.copy(), peer))
        return plain(param, peer, factor)

    init, deltas = worker.deltas_of(dtype)
    exp = ogossip.simulate(worker.NAMES, init, deltas, worker.SEND, worker.WAIT, "clock", None, 0.0, 1, worker.SEEDS,
                           lerp=lerp, add=None if dtype == "f32" else group_ref.add("f16"), train_after_wait=resident)
    for g in range(2):
        got = np.load(tmp_path / ("rank%d.npz" % g))
        assert list(got["peers"]) == [exp["picks"][r][g][0] for r in range(worker.T)], g
        assert np.array_equal(got["clocks"], exp["clocks"][:, g]), (g, got["clocks"], exp["clocks"][:, g])
        for r in range(worker.T):
            assert np.array_equal(got["params"][r].view(np.uint8), exp["params"][r, g].view(np.uint8)), (
                "rank %d, round %d (%s)" % (g, r, worker.PULLS[r]))       # (finite values: bits)
        # the staging payload is written by every round but a fused one: 'copy', 'packed', and the tracked round
        wrote = [r == 0 or not np.array_equal(got["staged"][r], got["staged"][r - 1]) for r in range(worker.T)]
        assert wrote == [True, True, False, False, False, True, g == 0], (g, wrote)
    p, q = (x.view(BITS[dtype]) for x in calls[2 * (worker.T - 1)])       # rank 0's operands of the tracked round
    for got, want in zip(np.load(tmp_path / "rank0.npz")["dist"], dist_ref.reference(dtype, p, q)):
        assert dist_ref.problem(float(got), want, p.size) is None, dist_ref.problem(float(got), want, p.size)


@pytest.mark.parametrize("what", ["mixed", "local", "wire", "relay"])
def test_packed_avg_is_refused_as_packed_is(tmp_path, what):
    """The same refusals by the same messages; nothing is launched."""
    import torch
    from dpwa_amd import DpwaConnection
    from dpwa_amd.adapters.pytorch import DpwaPyTorchAdapter
    from dpwa_amd.dpwa import GROUP_PACKED, MIXED_PACKED, RELAY_PACKED
    from dpwa_amd.group import LocalGroup
    from tests import dist_worker
    cfg = str(tmp_path / "pack.yaml")
    dist_worker.write_cfg(cfg, ["w1", "w2"], 1, "clock", 0.0)
    relay = DpwaConnection("w1", cfg, group=LocalGroup(), pull="relay:8") if what == "relay" else None
    with pytest.raises(ValueError) as e:
        if what == "mixed":
            DpwaConnection("w1", cfg, group=LocalGroup(), pull="packed-avg", layout=((torch.float32, 0, 4096),))
        elif what == "local":
            DpwaConnection("w1", cfg, group=LocalGroup(), pull="packed-avg:8")
        elif what == "wire":
            DpwaPyTorchAdapter(torch.nn.Linear(4, 4).to("cuda"), "w1", cfg, transport="wire", pull="packed-avg")
        else:
            relay.set_pull("packed-avg")
    if relay is not None:
        relay.close()
    want = {"mixed": MIXED_PACKED, "local": GROUP_PACKED, "relay": RELAY_PACKED}.get(what)
    assert str(e.value) == want if want else "pull='packed' needs the device transport" in str(e.value)
