"""What the non-finite check of a peer payload must say, for tests/test_finite_host.py and
tests/test_gpu_finite.py.

The quantity (include/dpwa_hip.h ``dpwa_check_finite``): a payload vetoes its round when any of its
first ``n`` elements has an exponent field of all ones -- a NaN of either kind or an infinity.
``vetoes`` / ``vetoes_mixed`` say so from the bit patterns with numpy; tests/test_finite_host.py
checks them against ``np.isfinite``.

``model`` is the pass as the kernels are specified (16-byte items, the ragged tail, the test on
both halves of every dword), and ``rounds`` the stamp rule of a learner's veto word; with a
``mutant`` each is one of the wrong kernels the tests must be able to tell from the right one.
``cases`` / ``mixed_cases`` are the inputs the GPU test runs, so the host test can show that every
mutant is told by one of them.  Nothing here calls the GPU library or torch on a device.
"""
import numpy as np

from tests import mixed_ref

DTYPES = ("f32", "bf16", "f16")
CODE = mixed_ref.CODE
SIZE = mixed_ref.SIZE
NUMPY = mixed_ref.NUMPY
PER = {d: 16 // SIZE[d] for d in DTYPES}              # elements of a lane's 16-byte item
SPAN = {d: 1024 // SIZE[d] for d in DTYPES}           # elements of a one-wave span
EXP = {"f32": 0x7f800000, "bf16": 0x7f80, "f16": 0x7c00}
MANT = {"f32": 0x007fffff, "bf16": 0x007f, "f16": 0x03ff}
SIGN = {"f32": 0x80000000, "bf16": 0x8000, "f16": 0x8000}
BAD = {                                               # quiet NaN, signalling NaN, +inf, -inf
    "f32": {"qnan": 0x7fc00000, "snan": 0x7f800001, "+inf": 0x7f800000, "-inf": 0xff800000},
    "bf16": {"qnan": 0x7fc0, "snan": 0x7f81, "+inf": 0x7f80, "-inf": 0xff80},
    "f16": {"qnan": 0x7e00, "snan": 0x7c01, "+inf": 0x7c00, "-inf": 0xfc00},
}
LARGEST = {"f32": 0x7f7fffff, "bf16": 0x7f7f, "f16": 0x7bff}
GUARD = 16                                            # elements behind n that a case's buffer carries
MUTANTS = ("tail-ignored", "past-the-end", "16-bit-test-on-f32", "high-half-only", "inf-not-counted", "stale-veto")


def sizes(dtype):
    """1, an item less one, an item, a span less one, a span, a span and one, three spans and five,
    and a size of many spans with a tail."""
    per, span = PER[dtype], SPAN[dtype]
    return [1, per - 1, per, span - 1, span, span + 1, 3 * span + 5, 100_003]


def nonfinite(dtype, bits):
    """Per element: the exponent field is all ones."""
    bits = np.asarray(bits, dtype=NUMPY[dtype])
    return (bits & NUMPY[dtype](EXP[dtype])) == NUMPY[dtype](EXP[dtype])


def vetoes(dtype, bits):
    return bool(nonfinite(dtype, bits).any())


def vetoes_mixed(segs, payload):
    """`segs`: mixed_ref.segments' [(dtype, byte offset, byte length, elements)]; every byte of a
    segment is looked at as its type, the padding included."""
    payload = np.asarray(payload, dtype=np.uint8)
    return any(vetoes(d, np.ascontiguousarray(payload[off:off + length]).view(NUMPY[d])) for d, off, length, _ in segs)


def as_float(dtype, bits):
    """The values, for np.isfinite: bf16 widened exactly by << 16."""
    bits = np.asarray(bits, dtype=NUMPY[dtype])
    if dtype == "f32":
        return bits.view(np.float32)
    if dtype == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.view(np.float16)


# ---------------------------------------------------------------- the pass, and the wrong ones
def _test(dtype, look, mutant):
    if mutant == "16-bit-test-on-f32" and dtype == "f32":
        return nonfinite("bf16", np.ascontiguousarray(look).view(np.uint16))
    if mutant == "high-half-only" and dtype != "f32":
        return nonfinite(dtype, look[1::2])          # (a case's buffer begins on a dword)
    bad = nonfinite(dtype, look)
    if mutant == "inf-not-counted":
        bad = bad & ((look & NUMPY[dtype](MANT[dtype])) != 0)
    return bad


def model(dtype, buf, n, mutant=None):
    """Does the pass over the first n elements of `buf` (which goes on behind them) veto?"""
    per = PER[dtype]
    if mutant == "tail-ignored":
        look = buf[:n // per * per]
    elif mutant == "past-the-end":
        look = buf[:min(len(buf), -(-n // per) * per)]
    else:
        look = buf[:n]
    return bool(_test(dtype, np.asarray(look, dtype=NUMPY[dtype]), mutant).any())


def model_mixed(segs, payload, mutant=None):
    payload = np.asarray(payload, dtype=np.uint8)
    out = False
    for d, off, length, _ in segs:
        bits = np.ascontiguousarray(payload[off:off + length]).view(NUMPY[d])
        out = out or model(d, bits, len(bits), mutant)
    return out


def rounds(bad, mutant=None):
    """A learner's rounds, round i (from 1) carrying stamp i: which of them are skipped.  The veto
    word is never cleared and counts only while it equals the round's stamp."""
    word, out = 0, []
    for stamp, b in enumerate(bad, 1):
        if b:
            word = stamp
        out.append(word != 0 and (word == stamp or (mutant == "stale-veto" and word == stamp - 1)))
    return out


# ---------------------------------------------------------------- the inputs of the GPU test
def finite_noise(dtype, count, seed):
    """Random bit patterns with every non-finite one made finite (its lowest exponent bit cleared)."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << (8 * SIZE[dtype]), count, dtype=np.uint64).astype(NUMPY[dtype])
    low = NUMPY[dtype](EXP[dtype] & -EXP[dtype])
    return np.where(nonfinite(dtype, bits), bits & ~low, bits).astype(NUMPY[dtype])


def positions(dtype, n):
    """Where a bad element is put: first, last of the last full span, last (of the tail), and an odd
    and an even half of a dword in the middle."""
    span = SPAN[dtype]
    out = {"first": 0, "last": n - 1}
    if n >= span:
        out["last-of-last-full-span"] = n // span * span - 1
    mid = n // 2
    if n >= 2:
        out["odd-half"] = (mid | 1) if (mid | 1) < n else 1
        out["even-half"] = mid & ~1
    return out


def cases(dtype, n, seed=0):
    """[(name, bits of n + GUARD elements, vetoes)]: the buffer's first n elements are the payload."""
    np_t = NUMPY[dtype]
    base = finite_noise(dtype, n + GUARD, seed + n)
    assert not vetoes(dtype, base)
    out = [("finite-noise", base, False)]
    for kind, pattern in BAD[dtype].items():
        for where, i in positions(dtype, n).items():
            b = base.copy()
            b[i] = pattern
            out.append(("%s-%s" % (kind, where), b, True))
    past = base.copy()
    past[n:] = BAD[dtype]["qnan"]
    out.append(("nan-just-past-n", past, False))
    past = base.copy()
    past[n:] = BAD[dtype]["+inf"]
    out.append(("inf-just-past-n", past, False))
    fill = lambda *v: np.resize(np.array(v, dtype=np_t), n + GUARD)        # noqa: E731
    out.append(("largest-finite", fill(LARGEST[dtype], LARGEST[dtype] | SIGN[dtype]), False))
    out.append(("subnormals", fill(1, MANT[dtype], SIGN[dtype] | 1, SIGN[dtype] | MANT[dtype]), False))
    out.append(("signed-zeros", fill(0, SIGN[dtype]), False))
    if dtype == "f32":      # low halves that look like a 16-bit infinity or NaN
        out.append(("16-bit-inf-in-low-half", fill(0x00007f80, 0x3f807f80, 0x00007c00, 0x3f80ffff, 0x0000ff80), False))
    if dtype == "bf16":     # fp16's infinity is a finite bf16
        out.append(("f16-inf-pattern", fill(0x7c00, 0xfc00), False))
    for name, bits, want in out:
        assert vetoes(dtype, bits[:n]) == want, (dtype, n, name)
    return out


MIXED = {
    "three-types": [("f32", 1024), ("bf16", 2049), ("f16", 2048)],     # bf16: one block and one element, padded
    "f32-and-f16": [("f32", 3), ("f16", 4097)],
}


def mixed_cases(spec, seed=0):
    """[(name, payload bytes, vetoes)] of a segmented payload: a bad element in the first and the last
    element of every segment, and the patterns that must not veto."""
    segs, total = mixed_ref.segments(spec)
    base = np.zeros(total, dtype=np.uint8)
    for k, (d, off, _, n) in enumerate(segs):
        base[off:off + n * SIZE[d]] = finite_noise(d, n, seed + 31 * k).view(np.uint8)
    out = [("finite-noise", base, False), ("all-zero", np.zeros(total, dtype=np.uint8), False)]

    def put(payload, seg, i, pattern):
        d, off = seg[0], seg[1]
        payload[off + i * SIZE[d]:off + (i + 1) * SIZE[d]] = np.array([pattern], dtype=NUMPY[d]).view(np.uint8)

    for seg in segs:
        d, _, _, n = seg
        for kind, pattern in BAD[d].items():
            for where, i in (("first", 0), ("last", n - 1)):
                b = base.copy()
                put(b, seg, i, pattern)
                out.append(("%s-%s-%s" % (d, kind, where), b, True))
        if d == "f32":
            b = base.copy()
            for i, pattern in enumerate((0x00007f80, 0x3f807f80, 0x00007c00, 0x0000ff80)):
                put(b, seg, min(i, n - 1), pattern)
            out.append(("16-bit-inf-in-f32-low-halves", b, False))
    for name, payload, want in out:
        assert vetoes_mixed(segs, payload) == want, (spec, name)
    return segs, total, out
