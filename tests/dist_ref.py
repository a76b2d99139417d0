"""What the distance to the peer must be, for tests/test_distance_host.py and
tests/test_gpu_distance.py.

The quantity (include/dpwa_hip.h ``dpwa_distance``): over the parameters p and the peer snapshot q as
they were before the average, ``dist2 = sum (double(q) - double(p))**2`` and
``norm2 = sum double(p)**2``.  The reference widens the bit patterns to float64 with numpy, takes the
terms ``(q - p)**2`` and ``p**2`` in float64 and sums them with ``math.fsum`` (exactly rounded).
Nothing here calls the GPU library or torch on a device.

Tolerance, derived: each term carries at most three roundings; a sum of n non-negative terms taken
in any order is within (n - 1) * 2**-53 relative of the exact sum; the reference's sum is exactly
rounded.  So ``|got - ref| <= (n + 4) * 2**-53 * ref``; where ``ref == 0`` the result is exactly 0,
where it is NaN or infinite the result is NaN or that infinity.  tests/test_distance_host.py checks
numpy's own ``np.sum`` of the same terms against this bound for every input set below.
"""
import math

import numpy as np

DTYPES = ("f32", "bf16", "f16")
CODE = {"f32": 0, "bf16": 1, "f16": 3}                    # DPWA_F32 / DPWA_BF16 / DPWA_F16
SIZE = {"f32": 4, "bf16": 2, "f16": 2}
BITS = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16}
SPAN = {"f32": 256, "bf16": 512, "f16": 512}              # elements of a one-wave 1-KiB span
ITEM = {"f32": 4, "bf16": 8, "f16": 8}                    # elements of a lane's 16-byte item
HUGE = {"f32": 3e38, "bf16": 3e38, "f16": 65504.0}
SUBNORMAL = {"f32": 0x00000001, "bf16": 0x0001, "f16": 0x0001}   # the smallest one
NEG_ZERO = {"f32": 0x80000000, "bf16": 0x8000, "f16": 0x8000}
NAN = {"f32": 0x7fc00000, "bf16": 0x7fc0, "f16": 0x7e00}
INF = {"f32": 0x7f800000, "bf16": 0x7f80, "f16": 0x7c00}

# sizes in elements: a tail alone, under / exactly / over one span, many spans with a ragged tail
SIZES = {"f32": [1, 3, 255, 256, 257, 100_003], "bf16": [7, 511, 512, 513, 100_005], "f16": [7, 511, 512, 513, 100_005]}


def many_spans(dtype, accumulators):
    """A size with at least three times as many spans as there are accumulators, plus a tail."""
    return (3 * accumulators + 2) * SPAN[dtype] + ITEM[dtype] + 1


def to_bits(dtype, values):
    """float64/float32 values -> bit patterns of `dtype` (round-to-nearest-even)."""
    v32 = np.asarray(values, dtype=np.float32)
    if dtype == "f32":
        return v32.view(np.uint32).copy()
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return v32.astype(np.float16).view(np.uint16).copy()
    u = v32.view(np.uint32)
    return ((u + np.uint32(0x7fff) + ((u >> 16) & np.uint32(1))) >> 16).astype(np.uint16)


def widen(dtype, bits):
    """Bit patterns -> float64, exactly."""
    bits = np.ascontiguousarray(bits, dtype=BITS[dtype])
    if dtype == "f32":
        return bits.view(np.float32).astype(np.float64)
    if dtype == "f16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def terms(dtype, p_bits, q_bits):
    """(the (q - p)**2 terms, the p**2 terms), float64."""
    p, q = widen(dtype, p_bits), widen(dtype, q_bits)
    with np.errstate(all="ignore"):
        d = q - p
        return d * d, p * p


def fsum(x):
    """math.fsum that gives NaN / inf where a term is (fsum raises on inf - inf only, and every term
    here is >= 0 or NaN)."""
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).any():
        return math.nan
    if np.isinf(x).any():
        return math.inf
    return math.fsum(x.tolist())


def reference(dtype, p_bits, q_bits):
    """(dist2, norm2), exactly rounded."""
    d, n = terms(dtype, p_bits, q_bits)
    return fsum(d), fsum(n)


def reference_many(parts):
    """The same over several (dtype, p_bits, q_bits) pieces (a segmented payload, a model's tensors)."""
    ds, ns = [], []
    for dtype, p_bits, q_bits in parts:
        d, n = terms(dtype, p_bits, q_bits)
        ds.append(d)
        ns.append(n)
    return fsum(np.concatenate(ds)), fsum(np.concatenate(ns))


def bound(n):
    return (n + 4) * 2.0 ** -53


def problem(got, ref, n):
    """None when `got` meets the rule above for a sum of n terms whose reference is `ref`, else why not."""
    if math.isnan(ref):
        return None if math.isnan(got) else "%r where the reference is NaN" % got
    if math.isinf(ref):
        return None if got == ref else "%r where the reference is %r" % (got, ref)
    if ref == 0.0:
        return None if got == 0.0 else "%r where the reference is exactly 0" % got
    err = abs(got - ref)
    if not err <= bound(n) * ref:
        return "%r against %r: relative error %.3g over the bound %.3g" % (got, ref, err / ref, bound(n))
    return None


def cases(dtype, n, accumulators=None, seed=0):
    """[(name, p_bits, q_bits)]: the input sets of one (dtype, n).  `accumulators`: the
    implementation's accumulator count, for the case whose only difference lies in a span beyond it
    (left out where n has no such span)."""
    rng = np.random.default_rng(1000 * n + seed)
    span, item = SPAN[dtype], ITEM[dtype]
    p = to_bits(dtype, rng.standard_normal(n))
    q = to_bits(dtype, rng.standard_normal(n))
    out = [("normal", p, q), ("equal", p, p.copy())]

    def one_difference(name, at):
        qq = p.copy()
        qq[at] = q[at] if q[at] != p[at] else to_bits(dtype, [widen(dtype, p[at:at + 1])[0] + 1.0])[0]
        out.append((name, p, qq))
    one_difference("last-element", n - 1)                  # the last tail element where n has a tail
    if n >= span:
        one_difference("last-lane-of-last-full-span", n // span * span - 1)
    if accumulators is not None and n > (accumulators + 1) * span + 5:
        one_difference("span-beyond-the-accumulators", (accumulators + 1) * span + 5)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    out.append(("huge-opposite-signs", to_bits(dtype, HUGE[dtype] * sign), to_bits(dtype, -HUGE[dtype] * sign)))
    at = sorted({0, n // 2, n - 1})
    ps, qs = p.copy(), p.copy()
    ps[at] = 0
    qs[at] = SUBNORMAL[dtype]
    out.append(("subnormal-differences", ps, qs))
    zp = np.where(np.arange(n) % 2 == 0, 0, NEG_ZERO[dtype]).astype(BITS[dtype])
    zq = np.where(np.arange(n) % 3 == 0, NEG_ZERO[dtype], 0).astype(BITS[dtype])
    out.append(("signed-zeros", zp, zq))
    pn = p.copy()
    pn[n // 2] = NAN[dtype]
    out.append(("one-nan", pn, q))
    qi = q.copy()
    qi[n - 1] = INF[dtype]
    out.append(("one-inf", p, qi))
    return out
