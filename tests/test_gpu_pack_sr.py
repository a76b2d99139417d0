"""Stochastically rounded packed images on the GPU against tests/test_pack_sr_host.py's numpy model, byte for byte:
the stateless pack, the fused emit against the two launches it replaces, a learner's round and one lock-step round
between two ranks of which only one rounds stochastically."""
import ctypes

import numpy as np
import pytest

from tests import pack_ref as ref
from tests import test_pack_sr_host as model
from tests.test_gpu_pack import CODE, GUARD, hard_payload
from tests.test_gpu_pack_emit import RAGGED, parameters, planes

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
N = 3 * 1024 + 1          # elements: a ragged 16-byte item, a partial last group, more than one 4-KiB block
SALT = 0xA5A5F00D12345678


def ptr(t, at=0):
    return ctypes.c_void_p(t.data_ptr() + at)


def guarded(size, body=None, at=0):
    """`size` bytes of 0xFF (NaN patterns of every type) with GUARD more behind them, `body` at `at`."""
    import torch
    t = torch.full((size + GUARD,), 0xFF, dtype=torch.uint8, device="cuda:0")
    if body is not None:
        t[at:at + len(body)] = torch.from_numpy(np.frombuffer(bytes(body), np.uint8).copy()).to(t.device)
    return t


def image_bytes(dtype, n):
    from dpwa_amd import _lib
    size = ctypes.c_int64()
    _lib.call("dpwa_pack_bytes", CODE[dtype], n, ctypes.byref(size))
    return size.value


def check_image(dtype, nbytes, got, want):
    """Both planes whole are `want`'s (the image of an `nbytes` payload) and no other byte of the 0xFF buffer
    was written, behind it included."""
    q, scales, rest = planes(dtype, nbytes, got[:want.size])
    wq, ws, _ = planes(dtype, nbytes, want)
    assert np.array_equal(q, wq), "the q plane"
    assert np.array_equal(scales, ws), "the scale plane"
    assert (rest == 0xFF).all() and (got[want.size:] == 0xFF).all(), "bytes of no plane were written"


@pytest.mark.parametrize("nonce", model.NONCES)
@pytest.mark.parametrize("n", [N, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_stochastic_is_the_host_model(dtype, n, nonce):
    import torch
    from dpwa_amd import _lib
    nbytes = n * ref.SIZE[dtype]
    payload = hard_payload(dtype, nbytes)
    src, img = guarded(nbytes, payload), guarded(image_bytes(dtype, n))
    _lib.call("dpwa_pack_stochastic", CODE[dtype], ptr(src), n, ptr(img), nonce, _lib.stream_handle(None), None, None)
    torch.cuda.synchronize()
    check_image(dtype, nbytes, img.cpu().numpy(), model.image(payload, dtype, nonce))


def test_small_elements_are_published_with_the_right_frequency():
    """4096 fp32 groups of one 1.0 and sixty-three 0.3 / 127: nearest rounding publishes every small element as 0;
    stochastic rounding publishes 1 for a fraction within six binomial standard deviations of 0.3, on the device as
    in the model."""
    import torch
    from dpwa_amd import _lib
    p, m, nonce = 0.3, 4096 * 63, model.NONCES[1]
    band = 6.0 * np.sqrt(p * (1.0 - p) / m)
    g = np.full((4096, 64), np.float32(0.3) / np.float32(127.0), dtype=np.float32)
    g[:, 0] = 1.0
    payload = g.reshape(-1).view(np.uint8)
    src, near, sr = guarded(payload.size, payload), guarded(image_bytes("f32", g.size)), guarded(image_bytes("f32", g.size))
    s = _lib.stream_handle(None)
    _lib.call("dpwa_pack", CODE["f32"], ptr(src), g.size, ptr(near), s, None, None)
    _lib.call("dpwa_pack_stochastic", CODE["f32"], ptr(src), g.size, ptr(sr), nonce, s, None, None)
    torch.cuda.synchronize()
    q_near, q_sr = (t.cpu().numpy()[:g.size].view(np.int8).reshape(g.shape) for t in (near, sr))
    assert (q_near[:, 0] == 127).all() and not q_near[:, 1:].any()
    for q in (q_sr, model.pack(payload, "f32", nonce)[0].reshape(g.shape)):
        assert (q[:, 0] == 127).all() and np.isin(q[:, 1:], (0, 1)).all()
        assert abs((q[:, 1:] == 1).mean() - p) <= band, ((q[:, 1:] == 1).mean(), band)


def round_(dtype, cfg, loss, source, fused, nonce):
    """tests/test_gpu_pack_emit.round_ with the stochastic entries: one write-through round of N elements on fresh
    guarded buffers, by dpwa_average_pack_stochastic or by the average and dpwa_pack_stochastic of its snapshot.
    Every output buffer whole, guards included, then coef and the new clock."""
    import torch
    from dpwa_amd import _lib
    n, nbytes, s, off = N, N * ref.SIZE[dtype], _lib.stream_handle(None), _lib.SLOT_PAYLOAD_OFFSET
    payload, before = hard_payload(dtype, nbytes), parameters(dtype, (nbytes + 3) // 4)[:nbytes]
    slot = guarded(off + nbytes, bytes(_lib.Header(5.0, 0.0, 1, n, CODE[dtype])))
    slot[off:off + nbytes] = torch.from_numpy(payload).to(slot.device)
    size = image_bytes(dtype, n)
    peer_img, out_img, p, snap = guarded(size), guarded(size), guarded(nbytes, before), guarded(nbytes)
    clock = torch.tensor([2.0, -1.0], dtype=torch.float64, device=slot.device)
    coef = torch.zeros(32, dtype=torch.uint8, device=slot.device)
    _lib.call("dpwa_pack", CODE[dtype], ptr(slot, off), n, ptr(peer_img), s, None, None)
    head = (ctypes.byref(cfg), ptr(clock), loss, ptr(coef), ptr(snap))
    if fused:
        operands = (ptr(slot, off), None) if source == "payload" else (None, ptr(peer_img))
        _lib.call("dpwa_average_pack_stochastic", CODE[dtype], ptr(p), ptr(slot), *operands, n, *head, ptr(out_img), s,
                  None, None, nonce)
    else:
        if source == "payload":
            _lib.call("dpwa_average", CODE[dtype], ptr(p), ptr(slot), n, *head, s, None, None)
        else:
            _lib.call("dpwa_average_packed", CODE[dtype], ptr(p), ptr(slot), ptr(peer_img), n, *head, s, None, None)
        _lib.call("dpwa_pack_stochastic", CODE[dtype], ptr(snap), n, ptr(out_img), nonce, s, None, None)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (p, snap, out_img, coef, clock)], before


@pytest.mark.parametrize("noop", [False, True])
@pytest.mark.parametrize("source", ["payload", "image"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_launch_equals_the_two_it_replaces(dtype, source, noop):
    """Byte for byte, NaN bits and guards included, in a round that averages and in the ZeroDivision no-op round
    (loss interpolation, both losses 0), whose image is the unchanged parameters'; and the image is the model's."""
    from dpwa_amd import _lib
    cfg = _lib.Interp(_lib.INTERP_LOSS, 0, 0.0, 0.0) if noop else _lib.Interp(_lib.INTERP_CONSTANT, 0, 1.0 - 2.0 ** -20, 0.0)
    nonce = model.NONCES[1]
    (one, before), (two, _) = (round_(dtype, cfg, 0.0 if noop else 1.0, source, f, nonce) for f in (True, False))
    assert all(np.array_equal(a, b) for a, b in zip(one, two))
    status = _lib.Coef.from_buffer_copy(one[3].tobytes()).status
    assert status == (_lib.STATUS_ZERO_DIVISION if noop else 0)
    snap = one[1][:len(before)]
    assert np.array_equal(snap, before) == noop
    check_image(dtype, len(before), one[2], model.image(snap, dtype, nonce))


def learner_round(dtype, guard):
    """tests/test_gpu_pack_emit.learner_round in stochastic mode with salt SALT: (packs by publish, by average, guard
    hits, image 1 is the model's image of the published slot with nonce SALT ^ 2)."""
    import torch
    from dpwa_amd import _lib
    from dpwa_amd.devview import device_tensor
    n, dev, s = RAGGED[dtype], torch.device("cuda", 0), _lib.stream_handle(None)
    nbytes = n * ref.SIZE[dtype]
    cfg, h, lib = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.25, 0.0), ctypes.c_void_p(), _lib.load()
    _lib.call("dpwa_learner_create", ctypes.byref(h), 0, n, CODE[dtype], ctypes.byref(cfg))
    try:
        assert lib.dpwa_learner_set_pack_rounding(h, 1, SALT) == _lib.ERR_STATE      # before pack_enable
        _lib.call("dpwa_learner_pack_enable", h)
        assert lib.dpwa_learner_set_pack_rounding(h, 2, SALT) == _lib.ERR_ARG
        _lib.call("dpwa_learner_set_pack_rounding", h, 1, SALT)
        _lib.call("dpwa_learner_set_reuse_guard", h, int(guard))
        _lib.call("dpwa_learner_attach_local", h, 0, h)
        flat = torch.from_numpy(ref.narrow(np.random.default_rng(n).standard_normal(n), dtype)).to(dev)
        at = ctypes.c_void_p(flat.data_ptr())
        _lib.call("dpwa_learner_publish", h, at, 1.0, None, s)
        flat.view(torch.int16)[1::2] += 64          # the parameters move on: the average has something to do
        _lib.call("dpwa_learner_fetch", h, 0, 1, 0, s)
        _lib.call("dpwa_learner_average_through", h, at, 1.0, None, s)
        if guard:                                   # the guard's fix-up: the conditional repack rounds it too
            flat[:ref.SIZE[dtype]] = torch.from_numpy(ref.narrow([-3.0], dtype)).to(dev)
        _lib.call("dpwa_learner_publish_reuse", h, at, 1.0, None, s)
        torch.cuda.synchronize()
        by_publish, by_average, hits = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        _lib.call("dpwa_learner_pack_counts", h, ctypes.byref(by_publish), ctypes.byref(by_average))
        _lib.call("dpwa_learner_reuse_guard_hits", h, ctypes.byref(hits))
        image, size = ctypes.c_void_p(), ctypes.c_int64()
        _lib.call("dpwa_learner_pack_image", h, 1, ctypes.byref(image), ctypes.byref(size))
        got = device_tensor(image.value, size.value, torch.uint8, dev).cpu().numpy()
        slot, hdr, v = np.zeros(nbytes, np.uint8), ctypes.create_string_buffer(256), ctypes.c_uint64()
        _lib.call("dpwa_learner_read_snapshot", h, hdr, ctypes.c_void_p(slot.ctypes.data), nbytes, ctypes.byref(v))
        same = np.array_equal(got, model.image(slot, dtype, SALT ^ 2)) and np.array_equal(slot, flat.cpu().numpy())
        return by_publish.value, by_average.value, hits.value, bool(v.value == 2 and same)
    finally:
        _lib.call("dpwa_learner_destroy", h)


@pytest.mark.parametrize("guard", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_learner_rounds_every_image_of_a_publish_with_one_nonce(dtype, guard):
    assert learner_round(dtype, guard) == (1, 1, int(guard), True)


def knob_off_main(rank, world, shared, args):
    shared.reports.put((rank, "ok", [learner_round(dtype, guard) for dtype, guard in args]))


def test_knob_off_gives_the_same_image(monkeypatch):
    """DPWA_PACK_FUSED=0, read once, so in a fresh process: both images come from publishes and equal the model's."""
    from tests.test_gpu_group_dtypes import run_job
    monkeypatch.setenv("DPWA_PACK_FUSED", "0")
    reports = run_job("pack-sr-fused-off", 1, knob_off_main, [("f32", False), ("bf16", True)])
    assert reports == {0: ("ok", [(2, 0, 0, True), (2, 0, 1, True)])}, reports


def test_one_stochastic_rank_in_a_lockstep_round(tmp_path):
    """Two ranks, pull 'packed-avg', rank 0 alone rounding stochastically: rank 1 averages with the model's
    dequantised image of rank 0's snapshot (nonce: rank 0's salt ^ publish 1), rank 0 with pack_ref.roundtrip of
    rank 1's; the oracle's lerp, clocks and peers otherwise."""
    from oracle import gossip as ogossip
    from oracle import lerp as olerp
    from tests import dist_worker, pack_sr_worker as worker
    from tests.test_gpu_group_dtypes import free_port, run_job
    from dpwa_amd.dpwa import PACK_SALT
    cfg = str(tmp_path / "pack_sr.yaml")
    dist_worker.write_cfg(cfg, worker.NAMES, 1, "clock", 0.0)
    reports = run_job("packed-sr", 2, worker.round_main, (free_port(), cfg, str(tmp_path)))
    assert reports == {0: ("ok", 1), 1: ("ok", 1)}, reports
    calls = []

    def lerp(param, peer, factor):      # fetch_probability 1: rank 0 averages first, then rank 1
        raw = np.ascontiguousarray(peer).view(np.uint8)
        back = model.roundtrip(raw, "f32", PACK_SALT ^ 1) if len(calls) == 1 else ref.roundtrip(raw, "f32")
        calls.append(len(calls))
        return olerp.lerp_f32(param, back.view(np.float32), factor)

    init, deltas = worker.inputs()
    exp = ogossip.simulate(worker.NAMES, init, deltas, worker.SEND, worker.WAIT, "clock", None, 0.0, 1, worker.SEEDS,
                           lerp=lerp)
    assert calls == [0, 1]
    for g in range(2):
        got = np.load(tmp_path / ("rank%d.npz" % g))
        assert str(got["peer"]) == exp["picks"][0][g][0] and got["clock"] == exp["clocks"][0, g], g
        assert np.array_equal(got["params"].view(np.uint8), exp["params"][0, g].view(np.uint8)), g
