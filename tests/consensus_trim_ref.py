"""What the trimmed consensus of a group must be, for tests/test_consensus_trim_host.py and
tests/test_gpu_consensus_trim.py: the host model of include/dpwa_hip.h ``dpwa_consensus_trimmed`` (the
rule of the comment above ``k_consensus_trimmed``), the wrong implementations the inputs must tell from
it (MUTANTS), and the input sets that reach every path of the kernels.

The rule, restated in numpy.  Members x_0 .. x_{G-1} of one dtype and n, a trim t, for every element:
    key(x) = bits ^ (sign ? all-ones : sign-bit), compared unsigned (-NaN < -inf < .. < -0 < +0 < .. < +NaN)
    y_0 <= .. <= y_{G-1}                    the G values in key order
    s = ((-0.0 + y_t) + y_{t+1}) + .. + y_{G-t-1}    widened exactly to float64, float64 adds, ascending
    m = s * (1.0 / (G - 2t))                out = float32(m), then consensus_ref.round16: two roundings
    norm2 = sum m*m       spread2_i = sum (x_i - m)*(x_i - m) for EVERY member       spread2 = sum_i spread2_i
the terms formed in numpy float64 and summed with ``math.fsum``.  Comparisons and their tolerance are
consensus_ref's, unchanged (``same_mean``, ``sums_problem``): the device forms bit-identical terms and only
the order of the summation differs.

Nothing here calls the GPU library or torch on a device.
"""
import functools
import itertools
import math

import numpy as np

from tests import consensus_ref as ref
from tests import dist_ref as dr

# every (G, t) the entries accept: 1 <= t <= (G - 1) // 2 for G = 3..8
PAIRS = tuple((G, t) for G in range(3, 9) for t in range(1, (G - 1) // 2 + 1))

MUTANTS = ("trim-one-less", "trim-one-more", "always-median", "value-order", "descending-sum", "sum-from-plus-zero",
           "divide", "spread-over-kept", "last-member-unsorted", "halves-crossed", "direct-16-bit-rounding")


def exempt(mutant, dtype, G, t):
    """Why `mutant` computes what the model computes for every input of this (dtype, G, t), or None."""
    kept = G - 2 * t
    if mutant == "trim-one-more" and 2 * (t + 1) >= G:
        return "no value would be left"
    if mutant == "always-median" and t == (G - 1) // 2:
        return "t is the largest trim"
    if mutant == "divide" and kept & (kept - 1) == 0:
        return "the reciprocal of a power of two is exact"
    if mutant == "descending-sum":
        if kept < 3:
            return "float64 addition of one or two kept values is commutative"
        if dtype == "f16":        # multiples of 2**-24 below 2**16: a sum of eight needs 43 bits
            return "every partial sum of float16 values is exact in float64"
    if mutant in ("halves-crossed", "direct-16-bit-rounding") and dtype == "f32":
        return "16-bit only"
    if mutant == "direct-16-bit-rounding" and kept < 3:
        return "one kept value is not rounded and two have no such tie (consensus_ref.tie_columns)"
    return None


def model(dtype, members, t, mutant=None):
    """(centre bits, sums) of the members' bit patterns: the header's rule in numpy.  `mutant`: one of
    MUTANTS, a plausible wrong kernel the tests must tell from the rule."""
    G, top = len(members), 8 * dr.SIZE[dtype] - 1
    ones, sign_bit = (1 << (top + 1)) - 1, 1 << top
    b = np.stack(members).astype(np.uint64)
    n = b.shape[1]
    key = b ^ np.where(b >> top, ones, sign_bit).astype(np.uint64)
    with np.errstate(invalid="ignore"):         # (widening a signalling NaN)
        x = np.stack([dr.widen(dtype, m) for m in members])
    order = np.argsort(key, axis=0, kind="stable")
    if mutant == "value-order":                 # float comparison: -0 == +0, every NaN unordered and last
        order = np.argsort(x, axis=0, kind="stable")
    if mutant == "last-member-unsorted":
        order = np.concatenate([np.argsort(key[:G - 1], axis=0, kind="stable"), np.full((1, n), G - 1)])
    y = np.take_along_axis(x, order, axis=0)
    if mutant == "halves-crossed" and dtype != "f32":
        # a dword's high element (odd index of a lane's whole items; the tail goes one element a dword) keyed
        # with the low element's sign, the inverse taken from the key's own top bit as trim_unkey16 does
        sign = (b >> top).astype(bool)
        odd = np.arange(1, n // dr.ITEM[dtype] * dr.ITEM[dtype], 2)
        sign[:, odd] = sign[:, odd - 1]
        k = np.sort(b ^ np.where(sign, ones, sign_bit).astype(np.uint64), axis=0)
        y = np.stack([dr.widen(dtype, row) for row in k ^ np.where(k >> top, sign_bit, ones).astype(np.uint64)])
    lo = {"trim-one-less": t - 1, "trim-one-more": t + 1, "always-median": (G - 1) // 2}.get(mutant, t)
    hi = G - lo
    assert lo < hi, (mutant, G, t)
    with np.errstate(all="ignore"):
        s = np.full(n, 0.0 if mutant == "sum-from-plus-zero" else -0.0)
        for i in (reversed(range(lo, hi)) if mutant == "descending-sum" else range(lo, hi)):
            s = s + y[i]
        m = s / float(hi - lo) if mutant == "divide" else s * (1.0 / (hi - lo))
        bits = ref.direct16(dtype, m) if mutant == "direct-16-bit-rounding" else ref.round16(dtype, m.astype(np.float32))
        spread = [(xi - m) * (xi - m) for xi in x]
        if mutant == "spread-over-kept":
            rank = np.argsort(order, axis=0, kind="stable")         # where member i's value went
            spread = [np.where((r >= lo) & (r < hi), v, 0.0) for r, v in zip(rank, spread)]
        sums = {"norm2": dr.fsum(m * m), "member": [dr.fsum(v) for v in spread], "spread2": fsum_all(spread)}
    return bits, sums


def fsum_all(parts):
    """dist_ref.fsum of the parts' concatenation, fed a part at a time: at G * n of a million and more one
    list of all the terms costs several times what the sum does."""
    if any(np.isnan(p).any() for p in parts):
        return math.nan
    if any(np.isinf(p).any() for p in parts):
        return math.inf
    return math.fsum(itertools.chain.from_iterable(p.tolist() for p in parts))


def differs(dtype, a, b, n, G):
    """consensus_ref.differs over this model's (bits, sums) pairs."""
    return ref.differs(dtype, (a[0], None, a[1]), (b[0], None, b[1]), n, G)


def members_of(dtype, G, t, n, finite=False):
    """One seeded normal draw; member 1 scaled by 2**20; then, in fixed columns -- the last full lane and
    the tail element among them -- duplicates, +0 against -0, a subnormal, one NaN member, +inf and -inf
    in two members, and t + 1 NaNs of one sign (one of them is kept: the centre must be NaN, and with it
    every sum).  `finite`: without the NaNs and infinities, so that the sums are numbers to compare."""
    rng = np.random.default_rng(1000 * G + 10 * t + n)
    vals = rng.standard_normal((G, n))
    vals[1] *= 2.0 ** 20
    with np.errstate(over="ignore"):
        B = np.stack([dr.to_bits(dtype, v) for v in vals])
    neg, nan, inf, sub = dr.NEG_ZERO[dtype], dr.NAN[dtype], dr.INF[dtype], dr.SUBNORMAL[dtype]
    plants = [(slice(0, t + 1), nan), ([0, 2], [inf, inf | neg]), (G - 1, nan), ([0, 1], [sub, sub | neg]),
              (slice(None), np.where(np.arange(G) % 2 == 0, 0, neg)), None]        # (rows, their bits); None: duplicates
    whole = n // dr.ITEM[dtype] * dr.ITEM[dtype]
    for k in reversed(range(3 if finite else 0, 6)):            # (plant 0 last: it wins the tail element and the last full lane)
        for j in {(5 + 37 * k) % n, (whole - 1 - k) % n, (n - 1 - k) % n}:
            if plants[k] is None:
                B[1:3, j] = B[0, j]
            else:
                B[plants[k][0], j] = plants[k][1]
    return list(B)


# ---------------------------------------------------------------- the input sets
# eight distinct finite values of both signs, ascending; G members take the middle G of them
LADDER = (-520.0, -1.5, -0.0078125, 0.001953125, 0.75, 3.0, 96.0, 40960.0)


@functools.lru_cache(maxsize=None)
def order_ranks(G):
    """(G, C) ranks: every permutation of 0..G-1 down the columns, then every weak ordering with exactly
    one tie pair (members i < j share the rank of i), that whole set once more behind one column of
    zeros -- the set has an even number of columns, so every column of the second copy lies in the other
    half of a 16-bit dword than it does in the first, next to another neighbour."""
    strict = np.array(list(itertools.permutations(range(G))), dtype=np.int8).T
    ties = []
    for i, j in itertools.combinations(range(G), 2):
        less = np.array(list(itertools.permutations(range(G - 1))), dtype=np.int8).T      # ranks of all but j
        ties.append(np.insert(less, j, less[i], axis=0))
    once = np.concatenate([strict] + ties, axis=1)
    assert once.shape[1] % 2 == 0
    return np.concatenate([once, np.zeros((G, 1), dtype=np.int8), once], axis=1)


def orders_size(G):
    """The n that holds all of `orders`: 2 * (G! + C(G, 2) * (G - 1)!) + 1."""
    return 2 * (math.factorial(G) + G * (G - 1) // 2 * math.factorial(G - 1)) + 1


def landmarks(dtype):
    """The key order's landmarks as bits, 17 of them: -NaN, -inf, -max, -1, -min normal, -largest subnormal,
    -smallest subnormal, -0, their positive twins from +0 up to +NaN, and a second +NaN with another payload."""
    one = {"f32": 0x3f800000, "bf16": 0x3f80, "f16": 0x3c00}[dtype]
    normal = {"f32": 0x00800000, "bf16": 0x0080, "f16": 0x0400}[dtype]
    up = [0, dr.SUBNORMAL[dtype], normal - 1, normal, one, dr.INF[dtype] - 1, dr.INF[dtype], dr.NAN[dtype]]
    return np.array([v | dr.NEG_ZERO[dtype] for v in reversed(up)] + up + [dr.NAN[dtype] | 1], dtype=dr.BITS[dtype])


SPECIAL_DRAW = 4096


@functools.lru_cache(maxsize=None)
def special_columns(dtype, G):
    """(G, C) bits: every triple of the landmarks for G = 3 (float32: all of the v_med3_u32 path), a seeded
    draw of 4,096 columns beyond."""
    marks = landmarks(dtype)
    if G == 3:
        return marks[np.indices((len(marks),) * 3).reshape(3, -1)]
    return marks[np.random.default_rng(500 + G).integers(0, len(marks), size=(G, SPECIAL_DRAW))]


@functools.lru_cache(maxsize=None)
def reciprocal_columns(dtype, G, t):
    """(G, C) bits: columns of members a few ulps apart whose kept sum times the float64 reciprocal is not
    that sum divided.  The two centres are then one float64 ulp apart, which a member at a third of its
    own ulp from the centre turns into a relative 2**-28 (float32) or 2**-43 (16-bit) of its term."""
    kept = G - 2 * t
    if kept & (kept - 1) == 0:
        return np.zeros((G, 0), dtype=dr.BITS[dtype])
    rng = np.random.default_rng(900 + 10 * G + t)
    count = 1 << 12
    base = dr.to_bits(dtype, 1.0 + rng.random(count))
    cols = np.stack([base + rng.integers(0, 4, size=count).astype(dr.BITS[dtype]) for _ in range(G)])
    y = np.sort(np.stack([dr.widen(dtype, c) for c in cols]), axis=0)
    s = np.full(count, -0.0)
    for i in range(t, G - t):
        s = s + y[i]
    return cols[:, s * (1.0 / kept) != s / float(kept)]


def tie_columns(dtype, G, t):
    """(G, C) bits: consensus_ref.tie_columns of the G - 2t kept values (all inside (-1, 2)), t members of
    -4 below and t of +4 above them, the rows rotated so that no member is trimmed by its position."""
    kept = ref.tie_columns(dtype, G - 2 * t)
    if not kept.shape[1]:
        return np.zeros((G, 0), dtype=dr.BITS[dtype])
    low, high = (np.full((t, kept.shape[1]), dr.to_bits(dtype, [v])[0], dtype=dr.BITS[dtype]) for v in (-4.0, 4.0))
    return np.roll(np.concatenate([low, kept, high]), 1, axis=0)


def cancellation_columns(dtype, G, t):
    """(G, 2) bits: kept values -2**54, 2 (or -2) G - 2t - 2 times, 2**54, whose float64 sum depends on the
    order: ascending -2**54 + 2 is exact and leaves 2, descending 2**54 + 2 is a tie that rounds to 2**54 and
    leaves 0.  Trimmed: t members of -2**60 and t of 2**60; rows rotated.  None where fewer than three
    values are kept, and for float16, which has no 2**54."""
    kept = G - 2 * t
    if kept < 3 or dtype == "f16":
        return None
    cols = [[-2.0 ** 60] * t + [-2.0 ** 54] + [small] * (kept - 2) + [2.0 ** 54] + [2.0 ** 60] * t for small in (2.0, -2.0)]
    return np.roll(np.stack([dr.to_bits(dtype, c) for c in cols], axis=1), 1, axis=0)


POSITIONS = ("difference-in-the-last-tail-element", "difference-in-the-last-lane-of-the-last-full-span",
             "difference-in-a-span-beyond-row-1024")
PATTERNS = "all-16-bit-patterns"
NAMES = ("hard", "finite", "normal", "orders", "specials", PATTERNS, "negative-zeros", "cancellation", "ties", "reciprocal") + POSITIONS


def cases(dtype, G, t, n, only=None):
    """[(name, [member bits] * G)]: the input sets of one (dtype, G, t, n) that fit it; `only`: the names
    wanted.  A set with fewer columns than n is repeated, one with more gives its first n."""
    bits_t, span = dr.BITS[dtype], dr.SPAN[dtype]

    def fit(cols):
        return [np.resize(c, n).astype(bits_t) for c in cols]

    def normal():
        rng = np.random.default_rng(100_000 * G + n)
        return [dr.to_bits(dtype, rng.standard_normal(n)) for _ in range(G)]

    def orders():
        values = dr.to_bits(dtype, LADDER[(8 - G) // 2:(8 - G) // 2 + G])
        return fit(values[order_ranks(G)])

    def patterns():
        # member 0 every pattern in turn; member k (a_k j + c_k) mod 2**16 with a_k and c_k odd: a bijection
        # of the patterns, whose two halves of a dword differ by the odd a_k
        j = np.arange(n, dtype=np.uint64)
        return [(j if k == 0 else (2 * (7919 * k % 32768) + 1) * j + 2 * (104729 * k % 32768) + 1).astype(np.uint16)
                for k in range(G)]

    def difference(at):
        # every member equal but t + 1 of them, which hold a finite neighbour at `at`: above or below the
        # others, exactly one of the t + 1 is kept there
        def build():
            base = normal()[0]
            members = [base.copy() for _ in range(G)]
            for m in members[G - t - 1:]:
                m[at] = base[at] ^ bits_t(1 << 6)
            return members
        return build

    sets = {"hard": lambda: members_of(dtype, G, t, n), "finite": lambda: members_of(dtype, G, t, n, finite=True),
            "normal": normal, "orders": orders, "specials": lambda: fit(special_columns(dtype, G)),
            "negative-zeros": lambda: [np.full(n, dr.NEG_ZERO[dtype], dtype=bits_t) for _ in range(G)]}
    if dtype != "f32" and n >= 1 << 16:
        sets[PATTERNS] = patterns
    for name, cols in (("cancellation", cancellation_columns(dtype, G, t)), ("reciprocal", reciprocal_columns(dtype, G, t)),
                       ("ties", tie_columns(dtype, G, t) if dtype != "f32" else None)):
        if cols is not None and cols.shape[1]:
            sets[name] = lambda cols=cols: fit(cols)
    sets[POSITIONS[0]] = difference(n - 1)
    if n >= span:
        sets[POSITIONS[1]] = difference(n // span * span - 1)
    if n > (ref.ROWS + 1) * span + 5:
        sets[POSITIONS[2]] = difference((ref.ROWS + 1) * span + 5)
    return [(name, sets[name]()) for name in NAMES if name in sets and (only is None or name in only)]


# What the GPU test runs.  Every set that fits for every (dtype, G, t) at consensus_ref's small sizes and at
# 100,003 elements (all 65,536 patterns of a 16-bit type among them).  At 3 * 1024 + 2 spans the host model is
# what costs, as consensus_ref.MANY_SETS says of the mean, and here it also sorts: every pair runs `normal` and
# the three positional differences there, two sets a case up to G = 5 and one beyond, and (5, 2) also the value
# sets on the wrapped rows.
MANY_SETS = ("normal",) + POSITIONS
MANY_VALUES = (("hard", "finite"), ("orders", "negative-zeros"), ("specials",))


def grid():
    """[(dtype, G, t, n, only)] of the stateless single-dtype GPU test."""
    out = []
    for dtype in ref.DTYPES:
        for G, t in PAIRS:
            out += [(dtype, G, t, n, None) for n in ref.SMALL[dtype] + [ref.BIG]]
            per = 2 if G <= 5 else 1
            out += [(dtype, G, t, ref.many(dtype), MANY_SETS[k:k + per]) for k in range(0, len(MANY_SETS), per)]
            if (G, t) == (5, 2):
                out += [(dtype, G, t, ref.many(dtype), sets) for sets in MANY_VALUES]
    return out
