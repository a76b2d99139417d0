"""The write-through average that packs the snapshot it writes (dpwa_average_pack, and the learner's round that
runs it) against the host model: the project's host lerp of the dtype for the parameters and the snapshot,
tests/pack_ref.image of that snapshot for the image.  NaN positions equal, everything else bit-equal."""
import ctypes

import numpy as np
import pytest

from tests import pack_ref as ref
from tests.test_gpu_pack import CODE, GUARD, hard_payload
from tests.test_gpu_pack_avg import BITS, DTYPES, host_lerp, same

pytestmark = pytest.mark.gpu

SOURCES = ["payload", "image"]
RAGGED = {"f32": 2 * 1024 + 258 + 3, "bf16": 2 * (2 * 1024 + 258) + 5}   # elements: ragged, ends inside a block


def parameters(dtype, n32):
    """test_gpu_pack_avg's seeded draw with, where the payload has the groups, group 0 all zeros (the peer's is),
    group 2 zeros but for one value below 2^-100 (the peer's are signed zeros) and an inf in group 5: with
    hard_payload as the peer the snapshot's groups go through all three branches of the codec."""
    n = 4 * n32 // ref.SIZE[dtype]
    per = ref.GROUP // ref.SIZE[dtype]
    x = np.random.default_rng(7 * n32).standard_normal(n).astype(np.float32)
    for g, values in ((0, np.zeros(per)), (2, np.r_[np.zeros(per - 1), 2.0 ** -110]), (5, [1.0, np.inf])):
        if (g + 1) * per <= n:
            x[g * per:g * per + len(values)] = values
    return ref.narrow(x, dtype)


def planes(dtype, nbytes, image):
    """(q plane, scale plane, every other byte) of an image buffer."""
    at, q_end = ref.scale_offset(dtype, nbytes), ref.blocks(nbytes) * (ref.BLOCK // ref.SIZE[dtype])
    s_end = at + 64 * ref.blocks(nbytes)
    return image[:q_end], image[at:s_end], np.r_[image[q_end:at], image[s_end:]]


def round_(dtype, n32, cfg, loss, source, fused=True):
    """One write-through round on fresh guarded buffers: the parameters before and the peer's payload as the
    kernel sees it, then parameters, snapshot, image buffer, coef and new clock after.  `fused`:
    dpwa_average_pack; else dpwa_average / dpwa_average_packed and dpwa_pack of the snapshot."""
    import torch
    from dpwa_amd import _lib
    nbytes = 4 * n32
    n, dev, s = nbytes // ref.SIZE[dtype], torch.device("cuda", 0), _lib.stream_handle(None)
    payload, before = hard_payload(dtype, nbytes), parameters(dtype, n32)

    def guarded(size, body=b"", at=0):
        t = torch.full((size + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
        t[at:at + len(body)] = torch.from_numpy(np.frombuffer(body, np.uint8).copy()).to(dev)
        return t

    def ptr(t, at=0):
        return ctypes.c_void_p(t.data_ptr() + at)

    size = ctypes.c_int64()
    _lib.call("dpwa_pack_bytes", CODE[dtype], n, ctypes.byref(size))
    off = _lib.SLOT_PAYLOAD_OFFSET
    slot = guarded(off + nbytes, bytes(_lib.Header(5.0, 0.0, 1, n, CODE[dtype])))
    slot[off:off + nbytes] = torch.from_numpy(payload).to(dev)
    peer_img, out_img, p, snap = guarded(size.value), guarded(size.value), guarded(nbytes, before), guarded(nbytes)
    clock = torch.tensor([2.0, -1.0], dtype=torch.float64, device=dev)
    coef = torch.zeros(32, dtype=torch.uint8, device=dev)
    _lib.call("dpwa_pack", CODE[dtype], ptr(slot, off), n, ptr(peer_img), s, None, None)
    head = (ctypes.byref(cfg), ptr(clock), loss, ptr(coef), ptr(snap))
    if fused:
        operands = (ptr(slot, off), None) if source == "payload" else (None, ptr(peer_img))
        _lib.call("dpwa_average_pack", CODE[dtype], ptr(p), ptr(slot), *operands, n, *head, ptr(out_img), s, None, None)
    else:
        if source == "payload":
            _lib.call("dpwa_average", CODE[dtype], ptr(p), ptr(slot), n, *head, s, None, None)
        else:
            _lib.call("dpwa_average_packed", CODE[dtype], ptr(p), ptr(slot), ptr(peer_img), n, *head, s, None, None)
        _lib.call("dpwa_pack", CODE[dtype], ptr(snap), n, ptr(out_img), s, None, None)
    torch.cuda.synchronize()
    for t in (slot, peer_img, out_img, p, snap):
        assert (t.cpu().numpy()[-GUARD:] == 0xFF).all(), "bytes behind a buffer were written"
    peer = payload if source == "payload" else ref.roundtrip(payload, dtype)
    return (before, peer, p.cpu().numpy()[:nbytes], snap.cpu().numpy()[:nbytes], out_img.cpu().numpy()[:size.value],
            coef.cpu().numpy().tobytes(), clock[1].item())


def check_image(dtype, got, snapshot):
    """Both planes whole are pack_ref's of `snapshot`, and no other byte of the buffer was written."""
    want = planes(dtype, len(snapshot), ref.image(snapshot, dtype))
    q, scales, rest = planes(dtype, len(snapshot), got)
    assert np.array_equal(q, want[0]), "the q plane"
    assert np.array_equal(scales, want[1]), "the scale plane"
    assert (rest == 0xFF).all(), "bytes of no plane were written"


@pytest.mark.parametrize("factor", [0.5, 1.0 - 2.0 ** -20])
@pytest.mark.parametrize("n32", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 1])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_average_pack_is_the_host_model(dtype, source, n32, factor):
    from dpwa_amd import _lib
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, factor, 0.0)
    before, peer, got, snap, image, coef, clock = round_(dtype, n32, cfg, 1.0, source)
    with np.errstate(all="ignore"):
        want = host_lerp(dtype, before.view(BITS[dtype]), peer.view(BITS[dtype]), factor).view(np.uint8)
    assert same(dtype, got, want), "the parameters"
    assert np.array_equal(snap, got), "the write-through snapshot"
    check_image(dtype, image, want)
    assert _lib.Coef.from_buffer_copy(coef).status == 0 and clock == factor * 5.0 + (1.0 - factor) * 2.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_op_round_packs_the_parameters(dtype):
    """Loss interpolation with both losses 0: parameters and clock stay, the snapshot receives the parameters and
    the image is theirs."""
    from dpwa_amd import _lib
    cfg = _lib.Interp(_lib.INTERP_LOSS, 0, 0.0, 0.0)
    before, _, got, snap, image, coef, clock = round_(dtype, 1025, cfg, 0.0, "image")
    assert _lib.Coef.from_buffer_copy(coef).status == _lib.STATUS_ZERO_DIVISION and clock == 2.0
    assert np.array_equal(got, before) and np.array_equal(snap, before)
    check_image(dtype, image, before)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_launch_equals_the_two_it_replaces(dtype, source):
    """Byte for byte, NaN bits included: the average, then dpwa_pack of the snapshot."""
    from dpwa_amd import _lib
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 1.0 - 2.0 ** -20, 0.0)
    one, two = (round_(dtype, 3 * 1024 + 1, cfg, 1.0, source, f) for f in (True, False))
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(one, two))


def learner_round(dtype, guard):
    """A self-peer, pack-enabled learner: publish, fetch, average_through, [guard: one element written through the
    flat buffer, in the word every publish samples], publish_reuse.  Returns the pack counts (by publish, by
    average), the guard's hits, and whether image 1 is pack_ref's image of the published slot's payload, which
    is the flat buffer's."""
    import torch
    from dpwa_amd import _lib
    from dpwa_amd.devview import device_tensor
    n, dev, s = RAGGED[dtype], torch.device("cuda", 0), _lib.stream_handle(None)
    nbytes = n * ref.SIZE[dtype]
    assert nbytes % 16 and nbytes % ref.BLOCK
    cfg, h = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.25, 0.0), ctypes.c_void_p()
    _lib.call("dpwa_learner_create", ctypes.byref(h), 0, n, CODE[dtype], ctypes.byref(cfg))
    try:
        _lib.call("dpwa_learner_pack_enable", h)
        _lib.call("dpwa_learner_set_reuse_guard", h, int(guard))
        _lib.call("dpwa_learner_attach_local", h, 0, h)
        start = ref.narrow(np.random.default_rng(n).standard_normal(n), dtype)
        flat = torch.from_numpy(start).to(dev)
        at = ctypes.c_void_p(flat.data_ptr())
        _lib.call("dpwa_learner_publish", h, at, 1.0, None, s)
        flat.view(torch.int16)[1::2] += 64          # the parameters move on: the average has something to do
        _lib.call("dpwa_learner_fetch", h, 0, 1, 0, s)
        _lib.call("dpwa_learner_average_through", h, at, 1.0, None, s)
        if guard:
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
        moved = not np.array_equal(slot, start) and np.array_equal(slot, flat.cpu().numpy())
        want = ref.image(slot, dtype)
        return (by_publish.value, by_average.value, hits.value,
                bool(v.value == 2 and moved and size.value == want.size and np.array_equal(got, want)))
    finally:
        _lib.call("dpwa_learner_destroy", h)


@pytest.mark.parametrize("guard", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_learner_packs_in_the_average_not_in_the_publish(dtype, guard):
    """The first publish packs (a full copy); the round's image comes from its average, and with the guard's
    fix-up from the conditional repack behind it, which neither count sees."""
    assert learner_round(dtype, guard) == (1, 1, int(guard), True)


def knob_off_main(rank, world, shared, args):
    shared.reports.put((rank, "ok", [learner_round(dtype, guard) for dtype, guard in args]))


def test_knob_off_packs_at_every_publish(monkeypatch):
    """DPWA_PACK_FUSED=0, read once, so in a fresh process: the counts read the other way, the image is the same."""
    from tests.test_gpu_group_dtypes import run_job
    monkeypatch.setenv("DPWA_PACK_FUSED", "0")
    reports = run_job("pack-fused-off", 1, knob_off_main, [("f32", False), ("bf16", True)])
    assert reports == {0: ("ok", [(2, 0, 0, True), (2, 0, 1, True)])}, reports
