"""What the float16 averaging must compute, for tests/test_f16_host.py and tests/test_gpu_f16.py.

There is no reference float16 path (the reference maps only FloatTensor, pytorch.py:11-14), so the
expected values are torch-CPU eager's on ``torch.float16`` tensors: ``f * q + (1 - f) * p`` with
``f`` a Python float (pytorch.py:68).  ``numpy_lerp`` restates it -- each product an fp32 product
of the fp32 coefficient rounded to fp16, then the fp16 sum -- and test_f16_host.py pins the
restatement to torch eager over every fp16 bit pattern.  All arrays here are ``uint16`` bit
patterns; nothing is ever compared against the GPU library or torch on the device.

Comparison rule (``same``): NaN positions coincide, every other element is bit-equal.
(oracle.lerp.bits_equal is not usable on these bits: it decodes uint16 as bf16.)
"""
import numpy as np
import torch

# every fp16 bit pattern as the peer, a fixed permutation of them as the parameters
PATTERNS = np.arange(65536, dtype=np.uint32).astype(np.uint16)
PERM = PATTERNS[np.random.default_rng(16).permutation(65536)]
for _fixed in (0x7c00, 0x8000):      # +inf meets +inf (inf - inf at the last two factors), -0 meets -0
    _at = int(np.flatnonzero(PERM == _fixed)[0])
    PERM[_at], PERM[_fixed] = PERM[_fixed], PERM[_at]
# 1.5 and -0.25 overflow to inf and produce inf - inf
FACTORS = [0.0, 1.0, 0.5, 0.3, 1.0 / 3.0, 1e-5, 0.9999, 1.5, -0.25]

NEG_ZERO = 0x8000


def as_half(u16):
    """uint16 bit patterns -> a torch.float16 CPU tensor over a copy."""
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16).copy()).view(torch.float16)


def as_u16(t):
    """A float16 tensor (any device) -> uint16 bit patterns on the host."""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def torch_lerp(p_u16, q_u16, f):
    """torch-CPU eager `f * t + (1 - f) * param.data` (pytorch.py:68) on float16."""
    f = float(f)
    p, q = as_half(p_u16), as_half(q_u16)
    return as_u16(f * q + (1 - f) * p)


def numpy_lerp(p_u16, q_u16, f):
    """f16(f16(a*q) + f16(b*p)), a = f32(f), b = f32(1 - f) with the subtraction in double."""
    f = float(f)
    a, b = np.float32(f), np.float32(1.0 - f)
    p = np.ascontiguousarray(p_u16).view(np.float16).astype(np.float32)
    q = np.ascontiguousarray(q_u16).view(np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        x = (a * q).astype(np.float16)
        y = (b * p).astype(np.float16)
        return (x.astype(np.float32) + y.astype(np.float32)).astype(np.float16).view(np.uint16)


def is_nan(u16):
    u16 = np.asarray(u16)
    return ((u16 & 0x7c00) == 0x7c00) & ((u16 & 0x03ff) != 0)


def same(got_u16, want_u16):
    got_u16, want_u16 = np.asarray(got_u16), np.asarray(want_u16)
    if got_u16.shape != want_u16.shape or got_u16.dtype != np.uint16 or want_u16.dtype != np.uint16:
        return False
    gn, wn = is_nan(got_u16), is_nan(want_u16)
    return bool(np.array_equal(gn, wn) and np.array_equal(got_u16[~gn], want_u16[~wn]))


def mismatches(got_u16, want_u16, limit=5):
    """(index, got, want) of the first few elements `same` objects to (for assertion messages)."""
    got_u16, want_u16 = np.asarray(got_u16), np.asarray(want_u16)
    gn, wn = is_nan(got_u16), is_nan(want_u16)
    bad = np.flatnonzero((gn != wn) | (~gn & ~wn & (got_u16 != want_u16)))
    return [(int(i), hex(int(got_u16[i])), hex(int(want_u16[i]))) for i in bad[:limit]]


def sample(n, seed):
    """(param, peer) bit patterns of n elements that put the hard cases everywhere a kernel
    treats differently (vector body and ragged tail alike): random bit patterns (subnormals,
    infinities and NaNs among them), with every fourth pair drawn from signed zeros and the
    smallest subnormals, whose products are exact zeros and sums of signed zeros."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 65536, n, dtype=np.uint32).astype(np.uint16)
    q = rng.integers(0, 65536, n, dtype=np.uint32).astype(np.uint16)
    special = np.array([0x0000, NEG_ZERO, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x0400, 0x7bff, 0xfbff], dtype=np.uint16)
    idx = np.arange(n)
    hard = idx[(idx % 4) == (seed % 4)]
    p[hard] = special[rng.integers(0, 2 + 7 * (hard % 3 == 0), hard.size) % special.size]
    q[hard] = special[rng.integers(0, 2 + 7 * (hard % 5 == 0), hard.size) % special.size]
    return p, q
