"""What every form of the averaging kernel must compute on hard values, for the three parameter
dtypes: the host-side reference, the samples, the case list and the guard bands shared by
tests/test_forms_host.py (no GPU), tests/test_gpu_forms.py and tests/forms_worker.py.

Expected values come from the project's host references only -- ``oracle.lerp.lerp_f32``,
``oracle.lerp.lerp_bf16`` and ``tests.f16_ref.torch_lerp`` (torch-CPU eager on float16) -- never
from the GPU library or torch on a device.  All arrays are bit patterns (``uint32`` for float32,
``uint16`` for bfloat16 and float16).

Comparison rule (``same``): NaN positions coincide, every other element is bit-equal.

``TUPLES`` lists every ``(dtype, n, seed, factor)`` the GPU tests average; the GPU code takes its
operands and expected values through ``case``, which refuses a tuple that is not listed, so the
host test's conditions on the list (the NaN cap, the mutants) hold for what the GPU runs.  A seed
is an int (``sample(dtype, n, seed)``) or, for resident learners that average each other's
parameters, a pair ``(a, b)``: the parameters of ``sample(dtype, n, a)`` meeting those of
``sample(dtype, n, b)``.

The "pull" form is tests/test_gpu_moves.py's: a snapshot pulled by the copy kernel or the copy
engine at the sizes of ``moves_ref.pull_sizes`` and then averaged with the constant factor 0.3.
"""
import functools

import numpy as np

from oracle import lerp as olerp
from oracle import policy as opolicy
from tests import f16_ref, moves_ref
from tests.mixed_ref import CODE, HARD, NUMPY, SIZE, TORCH, tensor_bits  # noqa: F401  (re-exported)
from tests.test_gpu_f16 import FUSED

DTYPES = ("f32", "bf16", "f16")
PER = {d: 16 // SIZE[d] for d in DTYPES}                      # elements of a 16-byte item
SIGN = {"f32": 0x80000000, "bf16": 0x8000, "f16": 0x8000}     # -0
INF = {"f32": 0x7f800000, "bf16": 0x7f80, "f16": 0x7c00}      # +inf = the exponent mask
# a subnormal pair whose average at f = 0.3 is a non-zero subnormal: half the smallest normal
# meets the largest subnormal (0.7 * 0.5 + 0.3 * ~1 = ~0.65 of the smallest normal)
SUBNORMAL_PAIR = {"f32": (0x00400000, 0x007fffff), "bf16": (0x0040, 0x007f), "f16": (0x0200, 0x03ff)}
FACTORS = f16_ref.FACTORS                                      # the nine of the every-pattern tests

GUARD = 8192       # the widest span any instantiation stores: 512 lanes x 16 B
GUARD_BYTE = 0xA5


# ---------------------------------------------------------------- reference and comparison
def lerp(dtype, p_bits, q_bits, f):
    """The averaged parameters' bits: the host reference of `dtype`."""
    p = np.ascontiguousarray(p_bits, dtype=NUMPY[dtype])
    q = np.ascontiguousarray(q_bits, dtype=NUMPY[dtype])
    if dtype == "f32":
        return np.ascontiguousarray(olerp.lerp_f32(p.view(np.float32), q.view(np.float32), f)).view(np.uint32)
    if dtype == "bf16":
        return olerp.lerp_bf16(p, q, f)
    return f16_ref.torch_lerp(p, q, f)


def is_nan(dtype, bits):
    bits = np.asarray(bits)
    return (bits & (SIGN[dtype] - 1)) > INF[dtype]


def is_subnormal(dtype, bits):
    bits = np.asarray(bits)
    return ((bits & INF[dtype]) == 0) & ((bits & (SIGN[dtype] - 1)) != 0)


def is_finite(dtype, bits):
    return (np.asarray(bits) & INF[dtype]) != INF[dtype]


def _bad(dtype, got, want):
    gn, wn = is_nan(dtype, got), is_nan(dtype, want)
    return (gn != wn) | (~gn & ~wn & (got != want))


def same(dtype, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != NUMPY[dtype] or want.dtype != NUMPY[dtype]:
        return False
    return not _bad(dtype, got, want).any()


def mismatches(dtype, got, want, limit=5):
    """(index, got, want) of the first few elements `same` objects to (for assertion messages)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return [("shape/dtype", (got.shape, str(got.dtype)), (want.shape, str(want.dtype)))]
    return [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in np.flatnonzero(_bad(dtype, got, want))[:limit]]


def nan_share(dtype, want):
    """The share of expected elements that are NaN, and so exempt from bit comparison."""
    return float(is_nan(dtype, want).mean()) if len(want) else 0.0


# ---------------------------------------------------------------- samples
def hard_phase(seed):
    """Which element of every four is hard.  Seeds 16k .. 16k + 15 share it, so the learners of one
    dispatch (seeds base + i) have their hard values at the same places and they meet."""
    return (seed // 16) % 4


def sample(dtype, n, seed):
    """(param bits, peer bits) of n elements: random bit patterns (NaNs, infinities and subnormals
    among them); every fourth pair drawn from HARD[dtype] -- one time in four the same hard value on
    both sides, so that inf meets inf -- in the vector body and the ragged tail alike; of those,
    every eighth is -0 on both sides and the one behind it the subnormal pair, whatever the seed;
    the last element -0 meeting -0 (two products of exactly -0, which a +0 anywhere turns into
    +0); and, when the tail behind the last 16-byte item has at least 2 elements, the subnormal pair
    before it, whose average at f = 0.3 is a non-zero subnormal."""
    rng = np.random.default_rng([seed, CODE[dtype]])
    top = 1 << (8 * SIZE[dtype])
    p = rng.integers(0, top, n, dtype=np.uint64).astype(NUMPY[dtype])
    q = rng.integers(0, top, n, dtype=np.uint64).astype(NUMPY[dtype])
    hard = np.flatnonzero(np.arange(n) % 4 == hard_phase(seed))
    hp = HARD[dtype][rng.integers(0, HARD[dtype].size, hard.size)]
    hq = HARD[dtype][rng.integers(0, HARD[dtype].size, hard.size)]
    p[hard] = hp
    q[hard] = np.where(rng.integers(0, 4, hard.size) == 0, hp, hq)
    zeros, subs = hard[hard // 4 % 8 == 0], hard[hard // 4 % 8 == 1]
    p[zeros] = q[zeros] = SIGN[dtype]
    p[subs], q[subs] = SUBNORMAL_PAIR[dtype]
    if n:
        p[n - 1] = q[n - 1] = SIGN[dtype]
    if n % PER[dtype] >= 2:
        p[n - 2], q[n - 2] = SUBNORMAL_PAIR[dtype]
    return p, q


# every bf16 bit pattern as the peer, a fixed permutation of them as the parameters
PATTERNS_BF16 = np.arange(65536, dtype=np.uint32).astype(np.uint16)
PERM_BF16 = PATTERNS_BF16[np.random.default_rng(16).permutation(65536)]
for _fixed in (0x7f80, 0x8000):      # +inf meets +inf (inf - inf at the last two factors), -0 meets -0
    _at = int(np.flatnonzero(PERM_BF16 == _fixed)[0])
    PERM_BF16[_at], PERM_BF16[_fixed] = PERM_BF16[_fixed], PERM_BF16[_at]
PATTERNS_BF16.setflags(write=False)
PERM_BF16.setflags(write=False)


@functools.lru_cache(maxsize=None)
def every_bf16_pattern_expected(f):
    want = olerp.lerp_bf16(PERM_BF16, PATTERNS_BF16, f)
    want.setflags(write=False)
    return want


# ---------------------------------------------------------------- the cases of the GPU tests
def sizes(dtype):
    """The smallest shapes that reach every path of a one-wave span of 64 items: the tail alone,
    one item and a tail, one full span (the grid's last span is empty), one element over, three
    spans and the longest tail."""
    per = PER[dtype]
    return [per - 1, per + 1, 64 * per, 64 * per + 1, 3 * 64 * per + per - 1]


def resident_sizes(dtype):
    """And a whole and a partial XCD group of eight spans."""
    per = PER[dtype]
    return sizes(dtype) + [8 * 64 * per, 9 * 64 * per + 1]


def multi_span(dtype):
    return sizes(dtype)[-1]


def worker_sizes(dtype, wide=False):
    """tests/forms_worker.py: one span and one element, nine and one; `wide`: a full 512-lane span."""
    per = PER[dtype]
    return [64 * per + 1, 9 * 64 * per + 1] + ([512 * per + 1] if wide else [])


PLAIN_FACTORS = (0.3, 0.0, 1.0, 1.5)
PULL_FACTOR = 0.3
UNALIGNED_N = 1003
UNALIGNED_OFFSETS = [(1, 0), (0, 3), (2, 2), (7, 5)]          # (parameters, peer / snapshot), in elements
UNALIGNED_CASE = FUSED[1]                                      # clock interpolation, 3 and 7
ZERO_DIVISION = ("clock", None, 0.0, 0.0, 0.0, 1.0, 1.0)       # interpolation.py:22-24 with both clocks 0


def pull_elements(dtype):
    """Elements of the payloads of moves_ref.pull_sizes, over every cap of the pull's grid."""
    return sorted({b // SIZE[dtype] for cap in moves_ref.PULL_BLOCKS for b in moves_ref.pull_sizes(cap)})


def ragged_publish_elements(dtype):
    """tests/forms_worker.py run_publish: the element counts nearest (on both sides) to the payload
    byte counts of moves_ref.PUBLISH_BYTES that leave tail bytes behind the last 16-byte word."""
    s = SIZE[dtype]
    counts = {m for b in moves_ref.PUBLISH_BYTES for m in (b // s, -(-b // s)) if m > 0}
    return sorted(m for m in counts if (m * s) & 15)


def fused_factor(case):
    method, value, thr, my_clock, peer_clock, loss, peer_loss = case
    return opolicy.factor_and_clock(method, value, thr, my_clock, peer_clock, loss, peer_loss)


def many_sizes(dtype):
    """dpwa_average_many: two and three entries of different sizes (the begin[] scan), two of equal
    size (the round-robin order); "nine": the two sizes of tests/forms_worker.py."""
    per = PER[dtype]
    big = multi_span(dtype)
    return {"two": (big, per + 1), "three": (64 * per, big, per - 1), "equal": (64 * per + 1, 64 * per + 1),
            "nine": (9 * 64 * per + 1, 64 * per + 1)}


def many_case(i):
    """Entry i of a dpwa_average_many dispatch: clock interpolation, its own clocks and losses."""
    return ("clock", None, 0.0, float(i + 1), float(3 * i + 2), 0.5 + 0.1 * i, 0.25 + 0.2 * i)


# dpwa_average_many_resident: (me, peer) per descriptor; learners beyond the entries are peers
# outside the dispatch.  Uk: k_lerp_group with k source buffers (the closed and open groups of
# tests/test_gpu_pairs.py).
RESIDENT = {
    "one": [(0, 1)],                                               # the single kernel, out of place
    "two-apart": [(0, 1), (2, 3)],                                 # k_lerp_batch: no read is shared
    "mutual-pair": [(0, 1), (1, 0)],                               # k_lerp_pair
    "U3": [(0, 1), (1, 2), (2, 0)],                                # 3-cycle
    "U4": [(0, 3), (1, 3), (2, 0)],                                # 3-outside-peer
    "U5": [(0, 1), (1, 0), (2, 4), (3, 4)],                        # 4-pairs-and-outside
    "U6": [(5, 0), (0, 5), (1, 2), (2, 1), (3, 4), (4, 3)],
    "U7": [(0, 5), (1, 6), (2, 5), (3, 0), (4, 6)],                # 5-outside-peers
    "U8": [(2, 6), (0, 3), (6, 2), (4, 0), (3, 0), (7, 2), (1, 4), (5, 0)],
    "eleven-buffers": [(0, 6), (1, 7), (2, 8), (3, 9), (4, 10), (5, 6)],   # beyond eight: the XCD-grouped batch
    "zero-division": [(0, 1), (1, 0), (2, 3), (3, 2)],             # loss interpolation, entries 0 and 1 divide by zero
}
RESIDENT_LEARNERS = 11


def resident_learner(i, name):
    """(clock, published loss) of resident learner i."""
    if name == "zero-division":
        return 2.0 + i, (0.0 if i < 2 else 0.3 * i)
    return 1.0 + 0.5 * i, 0.2 + 0.1 * i


def resident_entry(name, j):
    """(method, my loss) of descriptor j."""
    if name == "zero-division":
        return "loss", [0.0, 0.0, 0.4, 0.7][j]
    return "clock", 0.5 + 0.1 * j


def resident_factor(name, j):
    """(factor, new clock) of descriptor j, or None where the reference raises ZeroDivisionError."""
    a, b = RESIDENT[name][j]
    method, loss = resident_entry(name, j)
    (clock, _), (peer_clock, peer_loss) = resident_learner(a, name), resident_learner(b, name)
    try:
        return opolicy.factor_and_clock(method, None, 0.0, clock, peer_clock, loss, peer_loss)
    except ZeroDivisionError:
        return None


def _tuples_at(dtype, n, base, forms):
    out = []
    if "plain" in forms:
        out += [(dtype, n, base, f) for f in PLAIN_FACTORS]
    if "average" in forms:
        out += [(dtype, n, base, fused_factor(c)[0]) for c in FUSED]
    if "unaligned" in forms:
        for k in range(len(UNALIGNED_OFFSETS)):
            out += [(dtype, n, base + k, 0.3), (dtype, n, base + k, fused_factor(UNALIGNED_CASE)[0])]
    if "many" in forms:
        for group in many_sizes(dtype).values():
            out += [(dtype, n, base + i, fused_factor(many_case(i))[0]) for i, m in enumerate(group) if m == n]
    if "resident" in forms:
        for name, picks in RESIDENT.items():
            for j, (a, b) in enumerate(picks):
                res = resident_factor(name, j)
                if res is not None:
                    out.append((dtype, n, (base + a, base + b), res[0]))
    if "pull" in forms:
        out.append((dtype, n, base, PULL_FACTOR))
    return out


def forms_at(dtype, n):
    """Which forms run at n elements of dtype (the worker's two extra sizes among them)."""
    forms = set()
    if n in sizes(dtype) or n in worker_sizes(dtype, wide=True):
        forms |= {"plain", "average"}
    if n == UNALIGNED_N:
        forms.add("unaligned")
    if any(n in group for group in many_sizes(dtype).values()):
        forms.add("many")
    if n in resident_sizes(dtype):
        forms.add("resident")
    if n in pull_elements(dtype):
        forms.add("pull")
    return forms


def all_sizes(dtype):
    return sorted(set(resident_sizes(dtype) + worker_sizes(dtype, wide=True) + [UNALIGNED_N] + pull_elements(dtype)))


# sample seeds per (dtype, n); entry or learner i of a dispatch uses the seed plus i.  1 unless the
# NaN cap of tests/test_forms_host.py fails with it for some tuple below (one NaN among 5 or 7
# elements exempts too much from comparison): then the next of 17, 33, ... that keeps the cap.
_RESEEDED = {("f32", 5): 17, ("f16", 7): 17, ("f16", 9): 17}
SEEDS = {(d, n): _RESEEDED.get((d, n), 1) for d in DTYPES for n in all_sizes(d)}


def _tuples(seeds):
    out = []
    for dtype in DTYPES:
        for n in all_sizes(dtype):
            out += _tuples_at(dtype, n, seeds[(dtype, n)], forms_at(dtype, n))
    return out


TUPLES = list(dict.fromkeys(_tuples(SEEDS)))
_LISTED = frozenset(TUPLES)


@functools.lru_cache(maxsize=None)
def operands(dtype, n, seed):
    """(param bits, peer bits) of a tuple's seed, read-only and shared."""
    if isinstance(seed, tuple):
        p, q = sample(dtype, n, seed[0])[0], sample(dtype, n, seed[1])[0]
    else:
        p, q = sample(dtype, n, seed)
    p.setflags(write=False)
    q.setflags(write=False)
    return p, q


@functools.lru_cache(maxsize=None)
def case(dtype, n, seed, f):
    """(param bits, peer bits, expected bits) of a listed tuple, computed once and shared."""
    assert (dtype, n, seed, f) in _LISTED, "not in forms_ref.TUPLES: %r" % ((dtype, n, seed, f),)
    p, q = operands(dtype, n, seed)
    want = lerp(dtype, p, q, f)
    want.setflags(write=False)
    return p, q, want


def seed_of(dtype, n, i=0):
    return SEEDS[(dtype, n)] + i


# ---------------------------------------------------------------- guard bands
def guarded(nbytes, offset=0):
    """(payload, check): a uint8 device tensor of `nbytes` that begins `offset` bytes behind a
    16-byte boundary, inside an allocation that holds GUARD bytes of 0xA5 (and the offset and
    alignment bytes) on each side of it; check() asserts that both bands still hold 0xA5
    everywhere.  The payload itself is 0xA5 too until written."""
    import torch
    whole = torch.full((GUARD + 16 + offset + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8,
                       device=torch.device("cuda", 0))
    start = GUARD + (-(whole.data_ptr() + GUARD)) % 16 + offset
    payload = whole[start:start + nbytes]
    assert (payload.data_ptr() - offset) % 16 == 0

    def check(what=None):
        for name, band in (("before", whole[:start]), ("behind", whole[start + nbytes:])):
            bad = torch.nonzero(band != GUARD_BYTE).reshape(-1)
            assert bad.numel() == 0, ("%d bytes written %s the payload, the first at band offset %d of %d"
                                      % (bad.numel(), name, int(bad[0]), band.numel()), what)
    return payload, check


# ---------------------------------------------------------------- mutants: plausible wrong kernels
def _decode(dtype, bits):
    bits = np.ascontiguousarray(bits, dtype=NUMPY[dtype])
    if dtype == "f32":
        return bits.view(np.float32)
    if dtype == "bf16":
        return olerp.bf16_to_f32(bits)
    return bits.view(np.float16).astype(np.float32)


def _round(dtype, x, truncate=False):
    """float32 (or float64) values -> bits of dtype, round-to-nearest-even."""
    x32 = np.asarray(x).astype(np.float32)
    if dtype == "f32":
        return x32.view(np.uint32)
    if dtype == "bf16":
        return (x32.view(np.uint32) >> 16).astype(np.uint16) if truncate else olerp.f32_to_bf16(x32)
    return x32.astype(np.float16).view(np.uint16)


def _flush(dtype, bits):
    bits = np.asarray(bits)
    return np.where((bits & INF[dtype]) == 0, bits & SIGN[dtype], bits).astype(NUMPY[dtype])


MUTANTS = {"f32": ("fma", "ftz", "neg-zero"),
           "bf16": ("fma", "ftz", "neg-zero", "one-rounding", "truncation"),
           "f16": ("fma", "ftz", "neg-zero", "one-rounding")}


def mutant(dtype, name, p_bits, q_bits, f):
    """`lerp` as a plausible wrong kernel would compute it.
    fma: the sum contracted with the first product (a * q unrounded); ftz: subnormal inputs,
    products and results flushed to zero; neg-zero: a product of -0 turned into +0; one-rounding:
    the fp32 sum of the fp32 products rounded once; truncation: bf16 by dropping the low half."""
    a, b = olerp.coefficients(f)
    ident = lambda bits: bits                                   # noqa: E731
    fz = (lambda bits: _flush(dtype, bits)) if name == "ftz" else ident
    rnd = lambda x: fz(_round(dtype, x, truncate=name == "truncation"))       # noqa: E731
    p, q = _decode(dtype, fz(p_bits)), _decode(dtype, fz(q_bits))
    with np.errstate(all="ignore"):
        if name == "one-rounding":
            return rnd(a * q + b * p)
        x, y = rnd(a * q), rnd(b * p)
        if name == "neg-zero":
            x, y = np.where(x == SIGN[dtype], 0, x), np.where(y == SIGN[dtype], 0, y)
        if name == "fma":
            return rnd(np.float64(a) * q.astype(np.float64) + _decode(dtype, y).astype(np.float64))
        return rnd(_decode(dtype, x) + _decode(dtype, y))
