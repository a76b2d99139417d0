"""What the guarded (healing) average must leave, for tests/test_heal_host.py and tests/test_gpu_heal.py.

The rule (include/dpwa_hip.h "Healing"), per element, "bad" = exponent field all ones:
    p good, q good: the lerp's bits      q bad: p (refused)      p bad, q good: q (healed)
``heal`` is that in numpy over the host lerp of each dtype (tests/forms_ref.py: the oracle for fp32 and
bf16, tests/f16_ref.py for fp16); with a ``mutant`` it is one of the wrong selects a kernel could make.
``inputs`` are the operands the GPU test runs, so the host test can show each mutant told by one of them.
"""
import numpy as np

from tests import forms_ref
from tests.finite_ref import BAD, DTYPES, LARGEST, MANT, NUMPY, PER, SIGN, SIZE, SPAN, nonfinite  # noqa: F401

MUTANTS = ("per-item", "per-dword", "both-bad-takes-q", "mantissa-only")
VARIANTS = ("q", "p", "both", "clean")      # where the bad elements of an input are planted


def sizes(dtype):
    """The tail alone; exactly one span; a second span of one item and a one-element tail; the longest tail."""
    per = PER[dtype]
    return [per - 1, 64 * per, 64 * per + per + 1, 3 * 64 * per + per - 1]


def heal(dtype, p, q, f, mutant=None):
    """(result bits, healed, refused) of one round with factor f."""
    t = NUMPY[dtype]
    p, q = np.asarray(p, dtype=t), np.asarray(q, dtype=t)
    pb, qb = nonfinite(dtype, p), nonfinite(dtype, q)
    if mutant == "mantissa-only":                       # infinities pass for good
        pb, qb = pb & ((p & t(MANT[dtype])) != 0), qb & ((q & t(MANT[dtype])) != 0)
    group = {"per-item": PER[dtype], "per-dword": 4 // SIZE[dtype]}.get(mutant, 1)
    whole = len(p) // PER[dtype] * PER[dtype]           # (the ragged tail is per element in any kernel)
    for m in (pb, qb):                                  # one decision for a whole item / dword
        v = m[:whole].reshape(-1, group)
        v |= v.any(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        r = forms_ref.lerp(dtype, p, q, f)
    take_q = pb if mutant == "both-bad-takes-q" else pb & ~qb
    keep_p = qb & ~take_q
    return np.where(take_q, q, np.where(keep_p, p, r)).astype(t), int(take_q.sum()), int(keep_p.sum())


def normal(dtype, n, seed):
    """Bits of n finite N(0,1) values."""
    x = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    if dtype == "f16":
        return x.astype(np.float16).view(np.uint16)
    return x.view(np.uint32) if dtype == "f32" else (x.view(np.uint32) >> 16).astype(np.uint16)


def inputs(dtype, n, variant, seed=0):
    """(p bits, q bits): N(0,1) with NaN / +inf / -inf planted by bit pattern in `variant`'s operand(s) at
    element 0, the last element of the last full span and the last (tail) element; in every variant -0.0 in
    q opposite a NaN p at element 1, the three bad rows of the table in the low and in the high half of six
    dwords whose other half is good (elements 2..13), and a subnormal and the largest finite value (good) in
    both operands at 14 and 15 -- wherever n has those elements."""
    p, q = normal(dtype, n, seed + 2 * n), normal(dtype, n, seed + 2 * n + 1)
    if variant == "clean":
        return p, q
    kinds, span = list(BAD[dtype].values()), SPAN[dtype]

    def put(i, pv=None, qv=None):
        if 0 <= i < n:
            p[i], q[i] = (p[i] if pv is None else pv), (q[i] if qv is None else qv)

    for k, i in enumerate((0, n // span * span - 1, n - 1)):
        put(i, kinds[(k + 1) % 4] if variant != "q" else None, kinds[k % 4] if variant != "p" else None)
    put(1, kinds[0], SIGN[dtype])
    rows = [(h, r) for h in (0, 1) for r in ((False, True), (True, False), (True, True))]      # (p bad, q bad)
    for j, (half, (p_bad, q_bad)) in enumerate(rows):
        put(2 * (j + 1) + half, kinds[j % 4] if p_bad else None, kinds[(j + 2) % 4] if q_bad else None)
    put(14, LARGEST[dtype], 1)
    put(15, SIGN[dtype] | MANT[dtype], LARGEST[dtype] | SIGN[dtype])
    return p, q
