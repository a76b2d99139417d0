"""What the consensus of a group must be, for tests/test_consensus_host.py and
tests/test_gpu_consensus.py: the host model of include/dpwa_hip.h ``dpwa_consensus``.

The arithmetic, restated in numpy.  Members x_0 .. x_{G-1} of one dtype and n, in member order:
    s = ((x_0 + x_1) + ...) + x_{G-1}     every operand widened exactly to float64, float64 adds
    m = s * (1.0 / G)                      a multiplication by the float64 reciprocal, no division
    out = m.astype(float32)                round to nearest even, subnormals kept; a bfloat16 /
                                           float16 payload rounds that float32 once more, through
                                           torch-CPU ``.to()`` -- two roundings, on purpose
    norm2 = sum m*m       spread2_i = sum (x_i - m)*(x_i - m)       spread2 = sum_i spread2_i
the terms formed in numpy float64 with the same operations and summed with ``math.fsum``.

Tolerance, derived as tests/dist_ref.py derives it: the device forms bit-identical terms (separate
float64 multiplies and adds, contraction off), so only the order of the summation differs; a sum of
T non-negative terms taken in any order is within (T - 1) * 2**-53 relative of the exact sum and the
reference is exactly rounded: ``|got - ref| <= (T + 4) * 2**-53 * ref`` with T = n for norm2 and for
each spread2_i and T = G*n for spread2; exactly 0 where the reference is 0, NaN or that infinity
where it is NaN or infinite.  The means are compared bit for bit (NaN positions equal).

Nothing here calls the GPU library or torch on a device.
"""
import functools
import math

import numpy as np
import torch

from tests import dist_ref as dr

DTYPES = dr.DTYPES
GROUPS = (1, 2, 3, 5, 8)
ROWS = 1024                                    # accumulator rows of the workspace (128 KiB / 128 B)
POISON = {"f32": 0xa5a5a5a5, "bf16": 0xa5a5, "f16": 0xa5a5}     # what a test fills `out` with
# sizes in elements: a tail alone, one under / exactly / one over a span
SMALL = {"f32": [1, 3, 255, 256, 257], "bf16": [1, 3, 511, 512, 513], "f16": [1, 3, 511, 512, 513]}
BIG = 100_003


def many(dtype):
    """3 * 1024 + 2 spans and a tail: every accumulator row takes three adds and more."""
    return dr.many_spans(dtype, ROWS)


def round16(dtype, m32):
    """float32 values -> the payload's bits, as the stored mean is rounded."""
    m32 = np.ascontiguousarray(m32, dtype=np.float32)
    if dtype == "f32":
        return m32.view(np.uint32).copy()
    t = torch.from_numpy(m32.copy()).to(torch.bfloat16 if dtype == "bf16" else torch.float16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def direct16(dtype, m):
    """float64 values rounded ONCE to the 16-bit type (what the model must not do).  The two-step
    rounding differs from it only where the float32 value is a tie of the 16-bit type and the float64
    value was not: there the one-step rounding goes to the side the float64 value lies on."""
    with np.errstate(all="ignore"):
        m32 = m.astype(np.float32)
    if dtype == "f32":
        return m32.view(np.uint32).copy()
    if dtype == "f16":
        with np.errstate(all="ignore"):
            return m.astype(np.float16).view(np.uint16).copy()
    bits = round16(dtype, m32)
    u = m32.view(np.uint32)
    rest = m - m32.astype(np.float64)
    tie = ((u & np.uint32(0xffff)) == np.uint32(0x8000)) & (rest != 0) & np.isfinite(m)
    away = tie & (np.sign(rest) == np.sign(m))
    return np.where(tie, (u >> 16).astype(np.uint16) + away.astype(np.uint16), bits).astype(np.uint16)


def model(dtype, members, mutant=None, carry=None):
    """(mean bits, m as float64, {"norm2", "spread2", "member": [..]}) of the members' bit patterns.
    `mutant`: one of MUTANTS, the wrong implementations the tests must tell from this one; `carry`:
    the sums of the call before on the same workspace (what "rows-not-zeroed" adds)."""
    G = len(members)
    x = [dr.widen(dtype, b) for b in members]
    n = len(x[0])
    order = list(range(G))
    if mutant == "reverse-order":
        order.reverse()
    if mutant == "last-member-dropped" and G > 1:
        order = order[:-1]
    with np.errstate(all="ignore"):
        if mutant == "fp32-accumulation":
            s = x[order[0]].astype(np.float32)
            for i in order[1:]:
                s = s + x[i].astype(np.float32)
            s = s.astype(np.float64)
        else:
            s = x[order[0]].copy()
            for i in order[1:]:
                s = s + x[i]
        m = s / float(G) if mutant == "divide" else s * (1.0 / G)
        m32 = m.astype(np.float32)
        bits = direct16(dtype, m) if mutant == "direct-16-bit-rounding" else round16(dtype, m32)
        stored = dr.widen(dtype, bits)
        ms = stored if mutant == "spread-against-stored-mean" else m
        mn = stored if mutant == "norm-of-stored-mean" else m
        norm = mn * mn
        spread = [(xi - ms) * (xi - ms) for xi in x]
    if mutant == "tail-dropped":
        whole = n // dr.ITEM[dtype] * dr.ITEM[dtype]
        bits[whole:] = POISON[dtype]
        norm = norm[:whole]
        spread = [t[:whole] for t in spread]
    sums = {"norm2": dr.fsum(norm), "member": [dr.fsum(t) for t in spread],
            "spread2": dr.fsum(np.concatenate(spread))}
    if mutant == "rows-not-zeroed" and carry is not None:
        sums = {"norm2": sums["norm2"] + carry["norm2"], "spread2": sums["spread2"] + carry["spread2"],
                "member": [a + b for a, b in zip(sums["member"], carry["member"])]}
    return bits, m, sums


MUTANTS = ("fp32-accumulation", "divide", "reverse-order", "direct-16-bit-rounding", "spread-against-stored-mean",
           "norm-of-stored-mean", "tail-dropped", "last-member-dropped", "rows-not-zeroed")


def same_mean(dtype, got, want):
    """Bit equality of two means, NaN positions equal (a NaN's payload is not compared)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(dr.widen(dtype, got)), np.isnan(dr.widen(dtype, want))
    return bool(np.array_equal(gn, wn) and np.array_equal(got[~gn], want[~wn]))


def sums_problem(got, want, n, G):
    """None when the sums `got` meet the bound against `want`, else why not."""
    checks = [("norm2", got["norm2"], want["norm2"], n), ("spread2", got["spread2"], want["spread2"], G * n)]
    checks += [("spread2_%d" % i, g, w, n) for i, (g, w) in enumerate(zip(got["member"], want["member"]))]
    for name, g, w, terms in checks:
        why = dr.problem(g, w, terms)
        if why is not None:
            return "%s: %s" % (name, why)
    return None


def differs(dtype, a, b, n, G):
    """Would a device that computed `b` fail the checks against the model's `a`?"""
    return not same_mean(dtype, b[0], a[0]) or sums_problem(b[2], a[2], n, G) is not None


@functools.lru_cache(maxsize=None)
def tie_columns(dtype, G):
    """Columns (G values each, as bits) whose float32 mean sits exactly on a rounding tie of the 16-bit
    type while the float64 mean does not, so that rounding once and rounding twice give different
    bits.  Found by a seeded search: members in [1, 2), one odd multiple of the type's ulp there or of
    a half, a quarter or an eighth of it (what puts the mean on a tie) and one far smaller member of either sign (what takes the float64
    mean off it).  Empty for float32, for G = 1 (the mean of one member is that member) and for
    G = 2: the set bits of a sum of two p-bit values lie in two windows of p <= 11 bits, and a value
    that float32 rounds onto a tie without being it has the tie's bit, 24 - p - 1 >= 12 clear bits
    below it and a set bit below those -- no window of p bits holds both ends."""
    if dtype == "f32" or G <= 2:
        return np.zeros((G, 0), dtype=dr.BITS[dtype])
    rng = np.random.default_rng(77 + G)
    ulp = 2.0 ** (-7 if dtype == "bf16" else -10)
    count = 1 << 16
    vals = 1.0 + ulp * rng.integers(0, int(1 / ulp), size=(G, count))
    vals[G - 2] = ulp * 2.0 ** -rng.integers(0, 4, size=count) * (2 * rng.integers(0, 64, size=count) + 1)
    # (float16 has nothing below 2**-24: its smallest subnormals are small enough against a mean near 1)
    tiny = 2.0 ** rng.integers(-24, -21, size=count) if dtype == "f16" else ulp * 2.0 ** rng.integers(-24, -17, size=count)
    vals[G - 1] = rng.choice([-1.0, 1.0], size=count) * tiny
    cols = np.stack([dr.to_bits(dtype, v) for v in vals])
    x = [dr.widen(dtype, c) for c in cols]
    s = x[0].copy()
    for xi in x[1:]:
        s = s + xi
    m = s * (1.0 / G)
    hit = round16(dtype, m.astype(np.float32)) != direct16(dtype, m)
    return cols[:, hit]


def cases(dtype, G, n, only=None):
    """[(name, [member bits] * G)]: the input sets of one (dtype, G, n); `only`: the names wanted."""
    rng = np.random.default_rng(100_000 * G + n)
    bits_t = dr.BITS[dtype]
    span = dr.SPAN[dtype]
    normal = [dr.to_bits(dtype, rng.standard_normal(n)) for _ in range(G)]
    out = [("normal", normal), ("equal", [normal[0].copy() for _ in range(G)])]
    j = np.arange(n)
    big = 1e30 if dtype != "f16" else 60000.0
    pattern = np.array([big, -big, 1.0])
    out.append(("cancellation", [dr.to_bits(dtype, pattern[(i + j) % 3]) for i in range(G)]))
    sign_at = 31 if dtype == "f32" else 15
    out.append(("subnormals", [(rng.integers(1, 0x400 if dtype == "f16" else 0x80, size=n)
                                | (rng.integers(0, 2, size=n) << sign_at)).astype(bits_t) for _ in range(G)]))
    out.append(("negative-zeros", [np.full(n, dr.NEG_ZERO[dtype], dtype=bits_t) for _ in range(G)]))
    out.append(("mixed-zeros", [np.where((i + j) % 2 == 0, 0, dr.NEG_ZERO[dtype]).astype(bits_t) for i in range(G)]))
    ties = tie_columns(dtype, G)
    if ties.shape[1]:
        out.append(("ties", [np.resize(ties[i], n).astype(bits_t) for i in range(G)]))
    with_nan = [m.copy() for m in normal]
    with_nan[G - 1][n // 2] = dr.NAN[dtype]
    out.append(("one-nan", with_nan))
    with_inf = [m.copy() for m in normal]
    with_inf[0][n - 1] = dr.INF[dtype]
    out.append(("one-inf", with_inf))
    if G >= 2:
        both = [m.copy() for m in normal]
        both[0][n // 2] = dr.INF[dtype]
        both[G - 1][n // 2] = dr.INF[dtype] | dr.NEG_ZERO[dtype]
        out.append(("inf-and-minus-inf", both))

    def one_difference(name, at):
        members = [normal[0].copy() for _ in range(G)]
        other = normal[0][at] ^ bits_t(1 << 6)        # a finite neighbour of the same sign and exponent
        members[G - 1][at] = other
        out.append((name, members))
    one_difference("difference-in-the-last-tail-element", n - 1)
    if n >= span:
        one_difference("difference-in-the-last-lane-of-the-last-full-span", n // span * span - 1)
    if n > (ROWS + 1) * span + 5:
        one_difference("difference-in-a-span-beyond-row-1024", (ROWS + 1) * span + 5)
    return [c for c in out if only is None or c[0] in only]


# What the GPU test runs.  Every input set for every G at the small sizes (a tail alone, a partial span,
# exactly one, a second workgroup) and at 100,003 elements (hundreds of workgroups, a ragged tail).  At
# 3 * 1024 + 2 spans the host model is what costs: math.fsum over (2 G + 1) n terms of 0.79M / 1.57M
# elements, measured where the suite runs at 0.1 s (G = 1, float32) to 0.85 s (G = 8, 16-bit) per input set
# and twice that on a slower host, so all thirteen sets for every (dtype, G) there would take longer than
# the rest of the module together.  At that size every G runs the sets whose answer depends on the size --
# `normal` (every row takes three adds and more) and the three positional differences, the one beyond row
# 1024 among them -- and G = 3 also runs the value sets on the wrapped rows (float32: cancellation,
# subnormals, zeros, NaN and the infinities; the 16-bit types their ties), split so that no case takes more
# than a few seconds.
MANY_SETS = ("normal", "difference-in-the-last-tail-element", "difference-in-the-last-lane-of-the-last-full-span",
             "difference-in-a-span-beyond-row-1024")
MANY_VALUES = (("cancellation", "subnormals", "mixed-zeros"), ("one-nan", "one-inf", "inf-and-minus-inf"))


def grid():
    """[(dtype, G, n, only)] of the stateless single-dtype GPU test."""
    out = []
    for dtype in DTYPES:
        for G in GROUPS:
            for n in SMALL[dtype] + [BIG]:
                out.append((dtype, G, n, None))
            out.append((dtype, G, many(dtype), MANY_SETS))
        if dtype == "f32":
            out += [(dtype, 3, many(dtype), sets) for sets in MANY_VALUES]
        else:
            out.append((dtype, 3, many(dtype), ("ties",)))
    return out


# The segmented payload of the mixed test: float32 exactly one 4-KiB block, bfloat16 a block and one
# element, float16 five elements (elements, then zero padding up to whole blocks).
MIXED_ELEMENTS = (("f32", 1024), ("bf16", 2049), ("f16", 5))


def mixed_layout():
    """[(dtype, byte offset, byte length, elements)]."""
    out, off = [], 0
    for dtype, count in MIXED_ELEMENTS:
        length = -(-count * dr.SIZE[dtype] // 4096) * 4096
        out.append((dtype, off, length, count))
        off += length
    return out
