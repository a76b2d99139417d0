"""What averaging a mixed-dtype (segmented) payload must compute, for tests/test_mixed_host.py and
tests/test_gpu_mixed.py.

A segmented payload is up to three segments -- float32, bfloat16, float16, in that order -- each a
whole number of 4096-byte blocks (include/dpwa_hip.h ``dpwa_layout``).  The expected bytes of an
average are, per segment, the project's host references for that dtype: ``oracle.lerp.lerp_f32``,
``oracle.lerp.lerp_bf16`` and ``tests.f16_ref.torch_lerp`` (torch-CPU eager on float16).  Nothing
here calls the GPU library or torch on a device; the layout arithmetic is restated here and not
taken from dpwa_amd/flat.py.

Comparison rule per segment: NaN positions coincide, every other element bit-equal
(``oracle.lerp.bits_equal`` for float32 and bfloat16, ``f16_ref.same`` for float16).
"""
import numpy as np
import torch

from oracle import lerp as olerp
from tests import f16_ref

BLOCK = 4096
ORDER = ("f32", "bf16", "f16")
CODE = {"f32": 0, "bf16": 1, "f16": 3}                      # DPWA_F32 / DPWA_BF16 / DPWA_F16
SIZE = {"f32": 4, "bf16": 2, "f16": 2}
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
NUMPY = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16}   # bit patterns

# signed zeros, smallest and largest subnormals, smallest normal, largest finite, infinities
HARD = {
    "f32": np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000,
                     0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000], dtype=np.uint32),
    "bf16": np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x007f, 0x807f, 0x0080, 0x7f7f, 0xff7f, 0x7f80, 0xff80],
                     dtype=np.uint16),
    "f16": np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x0400, 0x7bff, 0xfbff, 0x7c00, 0xfc00],
                    dtype=np.uint16),
}

# the layouts of the kernel tests: (dtype, elements) per segment
LAYOUTS = {
    "one-each": [("f32", 1), ("bf16", 1)],
    # the f32 segment is exactly one block (its last word abuts the bf16 segment), the bf16 segment
    # one element over a block
    "abutting": [("f32", 1024), ("bf16", 2049), ("f16", 5)],
    "no-bf16": [("f32", 3), ("f16", 4097)],
}


def round_up(x, a):
    return (x + a - 1) // a * a


def segments(spec):
    """[(dtype, byte offset, byte length, elements)] of a spec, and the total bytes."""
    out, off = [], 0
    for name in ORDER:
        for d, n in spec:
            if d == name:
                length = round_up(max(n * SIZE[d], 1), BLOCK)
                out.append((d, off, length, n))
                off += length
    return out, off


def sample(spec, seed):
    """(param bytes, peer bytes) of a segmented payload: random bit patterns in every element, the
    hard values in the first and last 16-byte word of every segment's elements, zero padding."""
    segs, total = segments(spec)
    rng = np.random.default_rng(seed)
    p, q = np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=np.uint8)
    for d, off, _, n in segs:
        per = 16 // SIZE[d]
        for buf in (p, q):
            bits = rng.integers(0, 1 << (8 * SIZE[d]), n, dtype=np.uint64).astype(NUMPY[d])
            for lo in sorted({0, max(0, (n - 1) // per * per)}):
                k = min(per, n - lo)
                bits[lo:lo + k] = HARD[d][rng.integers(0, HARD[d].size, k)]
            buf[off:off + n * SIZE[d]] = bits.view(np.uint8)
    return p, q


def elements(buf, seg):
    """The bit patterns of one segment's elements in a payload's bytes."""
    d, off, _, n = seg
    return np.ascontiguousarray(buf[off:off + n * SIZE[d]]).view(NUMPY[d])


def lerp(spec, p, q, f):
    """The averaged payload's bytes: per segment the host reference of its dtype; the padding
    stays zero (0*a + 0*b)."""
    segs, total = segments(spec)
    out = np.zeros(total, dtype=np.uint8)
    for seg in segs:
        d, off, _, n = seg
        pe, qe = elements(p, seg), elements(q, seg)
        if d == "f32":
            r = olerp.lerp_f32(pe.view(np.float32), qe.view(np.float32), f).view(np.uint32)
        elif d == "bf16":
            r = olerp.lerp_bf16(pe, qe, f)
        else:
            r = f16_ref.torch_lerp(pe, qe, f)
        out[off:off + n * SIZE[d]] = np.ascontiguousarray(r).view(np.uint8)
    return out


def same(spec, got, want):
    """None when `got` equals `want` under the rule above (padding byte for byte), else what differs."""
    segs, total = segments(spec)
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != (total,) or want.shape != (total,) or got.dtype != np.uint8:
        return "shape %s / %s, %d bytes expected" % (got.shape, want.shape, total)
    for seg in segs:
        d, off, length, n = seg
        g, w = elements(got, seg), elements(want, seg)
        if d == "f32":
            ok = olerp.bits_equal(g.view(np.float32), w.view(np.float32))
        elif d == "bf16":
            ok = olerp.bits_equal(g, w)
        else:
            ok = f16_ref.same(g, w)
        if not ok:
            bad = np.flatnonzero(g != w)[:5]
            return "%s segment: %s" % (d, [(int(i), hex(int(g[i])), hex(int(w[i]))) for i in bad])
        pad_g, pad_w = got[off + n * SIZE[d]:off + length], want[off + n * SIZE[d]:off + length]
        if not np.array_equal(pad_g, pad_w):
            return "%s segment: padding byte %d differs" % (d, int(np.flatnonzero(pad_g != pad_w)[0]))
    return None


def torch_eager(p, q, f):
    """torch-CPU eager `f * t + (1 - f) * param.data` (pytorch.py:68) on one tensor of any dtype."""
    f = float(f)
    return f * q + (1 - f) * p


def tensor_bits(t):
    """A float32 / bfloat16 / float16 tensor (any device) -> its bit patterns on the host."""
    t = t.detach().contiguous().cpu().reshape(-1)
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def tensors_same(got, want):
    """Two tensors of one dtype under the rule above."""
    g, w = tensor_bits(got), tensor_bits(want)
    if got.dtype == torch.float32:
        return olerp.bits_equal(g.view(np.float32), w.view(np.float32))
    if got.dtype == torch.bfloat16:
        return olerp.bits_equal(g, w)
    return f16_ref.same(g, w)


def mixed_net(body, seed=6):
    """A handful of small layers with fp32 norms in a `body`-dtype body (CPU)."""
    g = torch.Generator().manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.LayerNorm(17), torch.nn.Linear(17, 9),
                              torch.nn.LayerNorm(9), torch.nn.Linear(9, 5))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    for m in net:
        if isinstance(m, torch.nn.Linear):
            m.to(body)
    return net
