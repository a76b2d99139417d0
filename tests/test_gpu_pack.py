"""Packed snapshots on the GPU against tests/pack_ref.py, bit for bit: the stateless entries both ways, a
lock-step DistGroup of two ranks walking pull 'copy' -> 'packed' -> 'copy', and the refusals."""
import ctypes

import numpy as np
import pytest

from tests import helpers
from tests import pack_ref as ref

pytestmark = pytest.mark.gpu

CODE = {"f32": 0, "bf16": 1, "f16": 3}
GUARD = 4096                   # bytes behind every buffer, 0xFF: NaN patterns of all three types


def hard_payload(dtype, nbytes):
    """N(0,1) with, where the payload has the groups, one hard group each: all zeros (0), signed zeros (2),
    subnormals only (3), the ties 0.5 / 1.5 / 2.5 under amax = 127 (4), amax in the quad's first lane (5) and
    in its last element (6), the largest finite value (7), one NaN (9) and one inf (11); the groups between
    them stay normal, so a non-finite group's neighbours show."""
    rng = np.random.default_rng(nbytes)
    per = ref.GROUP // ref.SIZE[dtype]
    x = rng.standard_normal(nbytes // ref.SIZE[dtype]).astype(np.float32)
    big = {"f32": np.finfo(np.float32).max, "bf16": np.float32(3.3895314e38), "f16": np.float32(65504.0)}[dtype]

    def group(g, values, at=0):
        if (g + 1) * per <= x.size:
            x[g * per + at:g * per + at + len(values)] = values

    group(0, np.zeros(per))
    group(2, np.tile([0.0, -0.0], per // 2))
    group(4, np.zeros(per))
    group(4, [127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5])
    group(5, [9.0])
    group(6, [-9.0], at=per - 1)
    group(7, [big, -big], at=3)
    group(9, [np.nan], at=per // 2)
    group(11, [-np.inf], at=per - 2)
    raw = ref.narrow(x, dtype)
    if (3 + 1) * per <= x.size:    # subnormals of the payload's own type, as bits
        bits = np.arange(1, per + 1, dtype=np.uint32 if dtype == "f32" else np.uint16)
        raw[3 * ref.GROUP:4 * ref.GROUP] = bits.view(np.uint8)
    return raw


@pytest.mark.parametrize("n32,max_blocks", [(1, 512), (63, 512), (64, 512), (65, 512), (1023, 512), (1024, 512),
                                            (1025, 512), (3 * 1024 + 1, 2)])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_pack_then_unpack_is_the_model(dtype, n32, max_blocks):
    """dpwa_pack's two planes and dpwa_unpack's payload equal pack_ref's; NaN bytes behind the source's
    payload enter no amax, and the NaN bytes behind the destination's payload and around the planes stay."""
    import torch
    from dpwa_amd import _lib
    nbytes = 4 * n32
    n = nbytes // ref.SIZE[dtype]
    dev = torch.device("cuda", 0)
    payload = hard_payload(dtype, nbytes)
    want_image, want_back = ref.image(payload, dtype), ref.roundtrip(payload, dtype)
    size = ctypes.c_int64()
    _lib.call("dpwa_pack_bytes", CODE[dtype], n, ctypes.byref(size))
    assert size.value == want_image.size
    src = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    src[:nbytes] = torch.from_numpy(payload).to(dev)
    img = torch.full((size.value + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    dst = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    stream = _lib.stream_handle(None)
    _lib.call("dpwa_pack", CODE[dtype], ctypes.c_void_p(src.data_ptr()), n, ctypes.c_void_p(img.data_ptr()), stream,
              None, None)
    _lib.call("dpwa_unpack", CODE[dtype], ctypes.c_void_p(img.data_ptr()), n, ctypes.c_void_p(dst.data_ptr()),
              max_blocks, stream, None, None)
    torch.cuda.synchronize()
    got_image, got = img.cpu().numpy(), dst.cpu().numpy()
    at, q_end = ref.scale_offset(dtype, nbytes), ref.blocks(nbytes) * (ref.BLOCK // ref.SIZE[dtype])
    s_end = at + 64 * ref.blocks(nbytes)
    assert np.array_equal(got_image[:q_end], want_image[:q_end]), "the q plane"
    assert np.array_equal(got_image[at:s_end], want_image[at:s_end]), "the scale plane"
    assert (got_image[q_end:at] == 0xFF).all() and (got_image[s_end:] == 0xFF).all(), "bytes of no plane were written"
    assert np.array_equal(got[:nbytes], want_back), "the unpacked payload"
    assert (got[nbytes:] == 0xFF).all(), "bytes behind the payload were written"


@pytest.mark.parametrize("dtype,fds", [("f16", False), ("f32", False), ("f16", True)])
def test_lockstep_group_walks_copy_packed_copy(tmp_path, monkeypatch, dtype, fds):
    """Two ranks, four rounds, set_pull 'copy' -> 'packed' -> 'packed:2' -> 'copy': every round's parameters
    equal oracle.gossip.simulate's, whose fetched payload a packed round replaces by pack_ref.roundtrip of
    it; clocks and peers are the oracle's throughout.  `fds`: slots and images shared as file descriptors."""
    from oracle import gossip as ogossip
    from oracle import lerp as olerp
    from tests import dist_worker, group_ref, pack_worker as worker
    from tests.test_gpu_group_dtypes import free_port, run_job
    if fds:
        helpers.need_fd_sharing()
        monkeypatch.setenv("DPWA_VMM", "1")
    cfg = str(tmp_path / "pack.yaml")
    dist_worker.write_cfg(cfg, worker.NAMES, 1, "clock", 0.0)
    T = len(worker.PULLS)
    reports = run_job("packed-%s" % dtype, 2, worker.walk_main, (dtype, free_port(), cfg, str(tmp_path)))
    assert reports == {0: ("ok", T), 1: ("ok", T)}, reports
    plain = olerp.lerp_f32 if dtype == "f32" else group_ref.lerp("f16")
    calls = []

    def lerp(param, peer, factor):      # fetch_probability 1: both ranks average in every round, in order
        r = len(calls) // 2
        calls.append(r)
        if worker.PULLS[r].startswith("packed"):
            raw = ref.roundtrip(np.ascontiguousarray(peer).view(np.uint8), dtype)
            peer = raw.view(np.float32 if dtype == "f32" else np.uint16)
        return plain(param, peer, factor)

    init, deltas = worker.inputs(dtype)
    exp = ogossip.simulate(worker.NAMES, init, deltas, worker.SEND, worker.WAIT, "clock", None, 0.0, 1, worker.SEEDS,
                           lerp=lerp, add=None if dtype == "f32" else group_ref.add("f16"))
    assert len(calls) == 2 * T
    for g in range(2):
        got = np.load(tmp_path / ("rank%d.npz" % g))
        assert list(got["peers"]) == [exp["picks"][r][g][0] for r in range(T)], g
        assert np.array_equal(got["clocks"], exp["clocks"][:, g]), (g, got["clocks"], exp["clocks"][:, g])
        for r in range(T):
            assert np.array_equal(got["params"][r].view(np.uint8), exp["params"][r, g].view(np.uint8)), (
                "rank %d, round %d (%s)" % (g, r, worker.PULLS[r]))       # (finite values: bits)


@pytest.mark.parametrize("what", ["mixed", "local", "wire", "relay"])
def test_refused_by_name(tmp_path, what):
    """The packed pull where it is not built: a model that mixes dtypes, free-running and same-process
    groups, the wire transport, a relay-created connection and a learner with the relay enabled.  (What needs
    two processes is in tests/pack_worker.py: the unattached peer, a packed-created connection asked for the
    relay, and free-running ranks asked for the packed pull.)"""
    import torch
    from dpwa_amd import DpwaConnection, _lib
    from dpwa_amd.adapters.pytorch import DpwaPyTorchAdapter
    from dpwa_amd.dpwa import GROUP_PACKED, MIXED_PACKED, RELAY_PACKED
    from dpwa_amd.group import LocalGroup
    from dpwa_amd.learner import Learner
    from tests import dist_worker
    cfg = str(tmp_path / "pack.yaml")
    dist_worker.write_cfg(cfg, ["w1", "w2"], 1, "clock", 0.0)
    dev = torch.device("cuda", 0)
    interp = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    if what == "mixed":
        with pytest.raises(ValueError, match="mixes dtypes") as e:
            DpwaConnection("w1", cfg, group=LocalGroup(), pull="packed", layout=((torch.float32, 0, 4096),))
        assert str(e.value) == MIXED_PACKED
        lr = Learner(dev, 4096, torch.uint8, interp, layout=((torch.float32, 0, 4096),))
        with pytest.raises(_lib.DpwaError, match="DPWA_MIXED"):
            _lib.call("dpwa_learner_pack_enable", lr.handle)
        lr.close()
    elif what == "local":
        with pytest.raises(ValueError) as e:
            DpwaConnection("w1", cfg, group=LocalGroup(), pull="packed:8")
        assert str(e.value) == GROUP_PACKED
        conn = DpwaConnection("w1", cfg, group=LocalGroup())
        with pytest.raises(ValueError) as e:
            conn.set_pull("packed")
        assert str(e.value) == GROUP_PACKED and conn._pull == "copy"
        conn.close()
    elif what == "wire":
        with pytest.raises(ValueError, match="pull='packed' needs the device transport"):
            DpwaPyTorchAdapter(torch.nn.Linear(4, 4).to(dev), "w1", cfg, transport="wire", pull="packed")
    else:
        conn = DpwaConnection("w1", cfg, group=LocalGroup(), pull="relay:8")     # (refused before any bind)
        with pytest.raises(ValueError) as e:
            conn.set_pull("packed")
        assert str(e.value) == RELAY_PACKED and conn._pull == "relay:8"
        conn.close()
        lr = Learner(dev, 4096, torch.float32, interp)
        with pytest.raises(_lib.DpwaError, match="needs dpwa_learner_pack_enable"):
            _lib.call("dpwa_learner_set_pull", lr.handle, _lib.PULL_PACKED, 8)
        _lib.call("dpwa_learner_pack_enable", lr.handle)
        _lib.call("dpwa_learner_relay_enable", lr.handle, 2, 0)
        with pytest.raises(_lib.DpwaError, match="relay is enabled") as e:
            _lib.call("dpwa_learner_set_pull", lr.handle, _lib.PULL_PACKED, 8)
        assert e.value.code == _lib.ERR_STATE
        lr.close()
