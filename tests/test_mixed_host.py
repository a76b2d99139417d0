"""Mixed-dtype models on the host: the segmented flat buffer of dpwa_amd/flat.py (segment order,
4096-byte segments, zero padding, 256-byte tensor alignment, typed views aliasing one uint8
buffer, rehome / resync), the layout digest in Python against the C one, and the argument checks of
the new entry points that return before any HIP call.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from dpwa_amd import _lib
from dpwa_amd.flat import FlatParameters, c_layout, layout_digest
from tests import mixed_ref as ref

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


class Bag(torch.nn.Module):
    """Parameters of the given (dtype, shape)s, in that order, filled with distinct values."""

    def __init__(self, spec):
        super().__init__()
        for i, (dtype, shape) in enumerate(spec):
            t = (torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape) + 1 + 100 * i).to(dtype)
            self.register_parameter("p%d" % i, torch.nn.Parameter(t))


def bytes_of(t):
    return t.detach().contiguous().view(torch.uint8).reshape(-1)


def test_layout_of_a_three_dtype_model():
    """Segments in the order float32, bfloat16, float16 whatever the parameters' order; inside a
    segment named_parameters() order, 256-byte aligned; 4096-byte starts and lengths; everything
    no parameter occupies is zero; the parameters keep their values and are views of the buffer."""
    spec = [(F16, (3, 5)), (F32, (7,)), (BF16, (2049,)), (F32, (65,)), (F16, (1,)), (BF16, (2, 2))]
    net = Bag(spec)
    before = [p.detach().clone() for p in net.parameters()]
    flat = FlatParameters(net.named_parameters())
    assert flat.buffer.dtype == torch.uint8 and flat.buffer.dim() == 1 and flat.dtype == torch.uint8
    assert flat.names == ["p%d" % i for i in range(6)]
    # f32: 7*4 -> 256, 65*4 = 260 -> 512: 768 -> 4096;  bf16: 4098 -> 4352, 8 -> 256: 4608 -> 8192;
    # f16: 30 -> 256, 2 -> 256: 512 -> 4096
    assert flat.layout == ((F32, 0, 4096), (BF16, 4096, 8192), (F16, 12288, 4096))
    assert flat.numel == flat.buffer.numel() == 16384
    assert flat.offsets == [12288, 0, 4096, 256, 12288 + 256, 4096 + 4352]
    used = torch.zeros(flat.numel, dtype=torch.bool)
    for p, o, b, (dtype, shape) in zip(flat.params, flat.offsets, before, spec):
        assert o % 256 == 0
        assert p.dtype == dtype and tuple(p.shape) == tuple(shape) and torch.equal(p.detach(), b)
        assert p.data_ptr() == flat.buffer.data_ptr() + o
        nbytes = p.numel() * p.element_size()
        assert torch.equal(flat.buffer[o:o + nbytes], bytes_of(b))
        assert not used[o:o + nbytes].any()
        used[o:o + nbytes] = True
        seg = [s for s in flat.layout if s[0] == dtype][0]
        assert seg[1] <= o and o + nbytes <= seg[1] + seg[2]
    assert not flat.buffer[~used].any()                      # gaps and segment padding are zero
    for _, off, length in flat.layout:
        assert off % 4096 == 0 and length % 4096 == 0 and length > 0
    assert flat.layout_digest == layout_digest(flat.layout) != 0


def test_two_dtype_models_and_the_independent_restatement():
    """Any two of the three dtypes; the layout equals tests/mixed_ref.py's own arithmetic."""
    for a, b, names in ((F32, BF16, ("f32", "bf16")), (F32, F16, ("f32", "f16")), (BF16, F16, ("bf16", "f16"))):
        flat = FlatParameters(Bag([(b, (1025,)), (a, (1025,))]).named_parameters())
        segs, total = ref.segments([(names[1], 1025), (names[0], 1025)])
        assert [(ref.TORCH[d], o, n) for d, o, n, _ in segs] == list(flat.layout)
        assert flat.numel == total
        assert [d for d, _, _ in flat.layout] == [a, b]


def test_parameters_and_buffer_alias_each_other():
    net = Bag([(BF16, (4, 4)), (F32, (5,)), (F16, (9,))])
    flat = FlatParameters(net.named_parameters())
    with torch.no_grad():
        net.p1[2] = -7.5                                      # a parameter write shows in the bytes
    o = flat.offsets[1]
    assert flat.buffer[o + 8:o + 12].view(F32).item() == -7.5
    o = flat.offsets[2]
    flat.buffer[o:o + 2] = torch.tensor([1.5], dtype=F16).view(torch.uint8)   # and the reverse
    assert net.p2[0].item() == 1.5
    o = flat.offsets[0]
    flat.buffer[o + 30:o + 32] = torch.tensor([-2.0], dtype=BF16).view(torch.uint8)
    assert net.p0[3, 3].item() == -2.0
    assert torch.equal(flat.view("p1"), net.p1.detach()) and flat.view("p0").data_ptr() == net.p0.data_ptr()


def test_rehome_and_resync():
    net = Bag([(BF16, (4, 4)), (F32, (5,)), (F16, (9,))])
    flat = FlatParameters(net.named_parameters())
    values = [p.detach().clone() for p in net.parameters()]
    slots = [torch.empty(flat.numel, dtype=torch.uint8), torch.empty(flat.numel, dtype=torch.uint8)]
    for r in range(4):
        nxt = slots[r % 2]
        nxt.copy_(flat.buffer)
        flat.rehome(nxt)
        assert flat.buffer is nxt
        for p, o, v in zip(flat.params, flat.offsets, values):
            assert p.data_ptr() == nxt.data_ptr() + o and torch.equal(p.detach(), v)
    assert len(flat._homes) == 2 and flat.resync() == 0
    with pytest.raises(ValueError):
        flat.rehome(torch.empty(flat.numel, dtype=torch.float32))
    with pytest.raises(ValueError):
        flat.rehome(torch.empty(flat.numel + 4096, dtype=torch.uint8))
    # a caller re-homes one parameter: resync copies it back into its place, dtype kept
    net.p2.data = torch.full((9,), 3.0, dtype=F16)
    assert flat.resync() == 1
    assert net.p2.data_ptr() == flat.buffer.data_ptr() + flat.offsets[2]
    assert net.p2.dtype == F16 and bool((net.p2 == 3.0).all())
    assert torch.equal(net.p0.detach(), values[0]) and flat.resync() == 0
    # ... even when the caller's tensor has another dtype (a model cast after the adapter was made)
    net.p0.data = torch.full((4, 4), 0.5, dtype=F32)
    assert flat.resync() == 1
    assert net.p0.dtype == BF16 and net.p0.data_ptr() == flat.buffer.data_ptr() + flat.offsets[0]
    assert bool((net.p0 == 0.5).all()) and torch.equal(net.p1.detach(), values[1])


def test_single_dtype_models_are_laid_out_as_before():
    for dtype in (F32, BF16, F16):
        net = Bag([(dtype, (3, 5)), (dtype, (700,))])
        flat = FlatParameters(net.named_parameters())
        esize = torch.empty((), dtype=dtype).element_size()
        assert flat.layout is None and flat.layout_digest == 0
        assert flat.buffer.dtype == dtype == flat.dtype
        assert flat.offsets == [0, 256 // esize]
        assert flat.numel == 256 // esize + (700 * esize + 255) // 256 * 256 // esize
        assert net.p1.data_ptr() == flat.buffer.data_ptr() + 256


def test_a_dtype_outside_the_three_is_a_key_error():
    with pytest.raises(KeyError):
        FlatParameters(Bag([(F32, (3,)), (torch.float64, (3,))]).named_parameters())


def c_digest(layout, total=-1):
    d = ctypes.c_uint32()
    _lib.call("dpwa_layout_digest", ctypes.byref(c_layout(layout)), total, ctypes.byref(d))
    return d.value


def test_python_digest_is_the_c_digest():
    layouts = [
        ((F32, 0, 4096), (BF16, 4096, 8192), (F16, 12288, 4096)),
        ((F32, 0, 8192), (BF16, 8192, 4096), (F16, 12288, 4096)),     # the same total, other cuts
        ((F32, 0, 4096), (F16, 4096, 8192), (BF16, 12288, 4096)),
        ((F32, 0, 4096), (BF16, 4096, 12288)),
        ((BF16, 0, 4096), (F16, 4096, 12288)),
        ((F16, 0, 16384),),
        ((F32, 0, 1 << 40), (BF16, 1 << 40, 4096)),                   # offsets beyond 32 bits
    ]
    seen = set()
    for lay in layouts:
        assert layout_digest(lay) == c_digest(lay) != 0, lay
        seen.add(layout_digest(lay))
    assert len(seen) == len(layouts)
    flat = FlatParameters(Bag([(F16, (3, 5)), (F32, (7,)), (BF16, (2049,))]).named_parameters())
    assert flat.layout_digest == c_digest(flat.layout, flat.numel)


BAD_LAYOUTS = {
    "none": (),
    "unaligned begin": ((F32, 0, 4096), (BF16, 4096 + 256, 4096)),
    "unaligned length": ((F32, 0, 4096 + 1024),),
    "empty segment": ((F32, 0, 0),),
    "not at 0": ((F32, 4096, 4096),),
    "out of order": ((F32, 4096, 4096), (BF16, 0, 4096)),
    "overlapping": ((F32, 0, 8192), (BF16, 4096, 4096)),
    "hole": ((F32, 0, 4096), (BF16, 8192, 4096)),
    "repeated dtype": ((F32, 0, 4096), (F32, 4096, 4096)),
}


def raw_layout(count, segs):
    lay = _lib.Layout()
    lay.count = count
    for i, (code, off, length) in enumerate(segs):
        lay.seg[i] = _lib.Segment(code, 0, off, length)
    return lay


@pytest.mark.parametrize("name", sorted(BAD_LAYOUTS))
def test_malformed_layouts_are_refused_without_a_device(name):
    """dpwa_layout_digest and dpwa_average_mixed check the layout before any HIP call."""
    lay = c_layout(BAD_LAYOUTS[name])
    lib = _lib.load()
    d = ctypes.c_uint32()
    assert lib.dpwa_layout_digest(ctypes.byref(lay), -1, ctypes.byref(d)) == _lib.ERR_ARG
    assert b"dpwa_layout_digest" in lib.dpwa_last_error()
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: the layout is refused first
    rc = lib.dpwa_average_mixed(ctypes.byref(lay), fake, fake, ctypes.byref(cfg), fake, 1.0, fake, None, None, None, None)
    assert rc == _lib.ERR_ARG and b"dpwa_average_mixed" in lib.dpwa_last_error()


def test_more_argument_checks_without_a_device():
    lib = _lib.load()
    d = ctypes.c_uint32()
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    fake = ctypes.c_void_p(1 << 20)
    good = c_layout(((F32, 0, 4096), (BF16, 4096, 4096)))
    # four segments, an unknown dtype code, DPWA_MIXED as a segment's dtype
    assert lib.dpwa_layout_digest(ctypes.byref(raw_layout(4, [(0, 0, 4096), (1, 4096, 4096), (3, 8192, 4096)])), -1,
                                  ctypes.byref(d)) == _lib.ERR_ARG
    for code in (2, 4, 7, -1):
        assert lib.dpwa_layout_digest(ctypes.byref(raw_layout(1, [(code, 0, 4096)])), -1, ctypes.byref(d)) == _lib.ERR_ARG
    # a layout that does not cover the payload's bytes exactly
    assert lib.dpwa_layout_digest(ctypes.byref(good), 8192, ctypes.byref(d)) == _lib.OK
    assert lib.dpwa_layout_digest(ctypes.byref(good), 12288, ctypes.byref(d)) == _lib.ERR_ARG
    assert lib.dpwa_layout_digest(None, -1, ctypes.byref(d)) == _lib.ERR_ARG
    # unaligned pointers
    odd = ctypes.c_void_p((1 << 20) + 8)
    for args in ((odd, fake, None), (fake, odd, None), (fake, fake, odd)):
        rc = lib.dpwa_average_mixed(ctypes.byref(good), args[0], args[1], ctypes.byref(cfg), fake, 1.0, fake, args[2],
                                    None, None, None)
        assert rc == _lib.ERR_ARG and b"aligned" in lib.dpwa_last_error()
    # DPWA_MIXED has no meaning without a layout: the single-dtype entries refuse it
    rc = lib.dpwa_average(_lib.MIXED, fake, fake, 8192, ctypes.byref(cfg), fake, 1.0, fake, None, None, None, None)
    assert rc == _lib.ERR_ARG and b"dpwa_average_mixed" in lib.dpwa_last_error()
    desc = (_lib.AverageDesc * 1)(_lib.AverageDesc(fake, fake, 8192, fake, 1.0, fake, None))
    for fn in (lib.dpwa_average_many, lib.dpwa_average_many_resident):
        assert fn(_lib.MIXED, desc, 1, ctypes.byref(cfg), None, None, None) == _lib.ERR_ARG
        assert b"not batched" in lib.dpwa_last_error()
    assert lib.dpwa_learner_set_layout(None, ctypes.byref(good)) == _lib.ERR_ARG
    assert lib.dpwa_node_set_layout(None, ctypes.byref(good)) == _lib.ERR_STATE


def test_the_reference_tells_the_dtypes_apart():
    """tests/mixed_ref.py itself: each segment is averaged as its own dtype (the same bits read as
    another 16-bit type give another result), the padding stays zero, and `same` objects to a
    single changed bit, in an element or in the padding."""
    spec = ref.LAYOUTS["abutting"]
    segs, total = ref.segments(spec)
    assert [(d, o, n) for d, o, n, _ in segs] == [("f32", 0, 4096), ("bf16", 4096, 8192), ("f16", 12288, 4096)]
    p, q = ref.sample(spec, 5)
    want = ref.lerp(spec, p, q, 0.3)
    assert want.shape == (total,) and ref.same(spec, want, want) is None
    as_f16 = ref.f16_ref.torch_lerp(ref.elements(p, segs[1]), ref.elements(q, segs[1]), 0.3)
    assert not np.array_equal(ref.elements(want, segs[1]), as_f16)      # the bf16 segment read as fp16
    for seg in segs:
        d, off, length, n = seg
        assert not want[off + n * ref.SIZE[d]:off + length].any()
        w = ref.elements(want, seg)
        expo = {"f32": 0x7f800000, "bf16": 0x7f80, "f16": 0x7c00}[d]
        finite = int(np.flatnonzero((w & expo) != expo)[0])       # (a NaN's payload is not compared)
        for at in (off + finite * ref.SIZE[d], off + length - 1):
            got = want.copy()
            got[at] ^= 1
            assert ref.same(spec, got, want) is not None, (d, at)
    assert ref.same(spec, p, want) is not None


def test_binding_constants_match_the_header():
    import re
    text = open(_lib.HEADER_PATH).read()
    consts = dict(re.findall(r"#define (DPWA_\w+) \(?(-?\d+)\)?", text))
    assert int(consts["DPWA_MIXED"]) == _lib.MIXED and int(consts["DPWA_F16"]) == _lib.F16
    assert int(consts["DPWA_LAYOUT_MAX_SEGMENTS"]) == _lib.LAYOUT_MAX_SEGMENTS
    assert int(consts["DPWA_LAYOUT_ALIGN"]) == _lib.LAYOUT_ALIGN == 4096
    assert ctypes.sizeof(_lib.Segment) == 24 and ctypes.sizeof(_lib.Layout) == 8 + 3 * 24


def test_connection_and_learner_want_a_layout_for_a_uint8_buffer():
    from dpwa_amd.learner import native_dtype
    assert native_dtype(torch.uint8, ((F32, 0, 4096), (BF16, 4096, 4096))) == _lib.MIXED
    assert native_dtype(torch.bfloat16) == _lib.BF16
    with pytest.raises(KeyError):
        native_dtype(torch.uint8)
    with pytest.raises(ValueError):
        native_dtype(torch.float32, ((F32, 0, 4096), (BF16, 4096, 4096)))


def test_relay_avg_is_refused_for_a_mixed_model(tmp_path):
    from dpwa_amd import DpwaConnection
    from dpwa_amd.group import LocalGroup
    from dpwa_amd.launch import write_config
    cfg = write_config(str(tmp_path / "m.yaml"), ["a", "b"], interpolation="constant")
    lay = ((F32, 0, 4096), (BF16, 4096, 4096))
    with pytest.raises(ValueError, match="relay-avg"):
        DpwaConnection("a", cfg, seed=1, group=LocalGroup(), pull="relay-avg", layout=lay)
    conn = DpwaConnection("a", cfg, seed=1, group=LocalGroup(), layout=lay)
    with pytest.raises(ValueError, match="relay-avg"):
        conn.set_pull("relay-avg:8")
    conn.set_pull("kernel:8")                                 # moves bytes: fine (applied at bind)
    conn.close()


def test_wire_transport_refuses_a_mixed_model_like_a_16_bit_one(tmp_path):
    """The wire carries float32 blobs only: the KeyError a ``.half()`` model gets, at the first
    update_send, before anything touches a device."""
    from dpwa_amd import DpwaPyTorchAdapter
    from dpwa_amd.launch import write_config
    cfg = write_config(str(tmp_path / "w.yaml"), ["a", "b"], interpolation="constant")
    errors = []
    for net in (ref.mixed_net(torch.bfloat16), torch.nn.Linear(3, 2).half()):
        ad = DpwaPyTorchAdapter(net, "a", cfg, transport="wire", seed=1, serve=False)
        try:
            with pytest.raises(KeyError) as err:
                ad.update_send(1.0)
            errors.append(str(err.value))
        finally:
            ad.connection.close()
    assert errors[0] == errors[1] and "float32" in errors[0]
