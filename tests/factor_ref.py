"""What the device factor (factor_math / factor_commit / read_loss in dpwa_amd/csrc/kernels.hip) must
compute on hard values: the case table, the reference, the wrong variants the table must tell from
it, and which cases every kernel form runs -- shared by tests/test_factor_host.py (no GPU),
tests/test_gpu_factor.py and tests/factor_worker.py.  Nothing here touches a GPU.

Reference: ``oracle.policy.factor_and_clock`` -- plain Python double arithmetic, which is the
semantics the kernels claim (dpwa.py:139-155 + interpolation.py, every operation separately
rounded).  A case is ``(method, value, threshold, clock, peer_clock, loss, peer_loss)``; its
expectation (``evaluate``) is ``ZD`` where the reference raises ZeroDivisionError (status
DPWA_STATUS_ZERO_DIVISION, clock kept, a = 0, b = 1) or ``(factor, new_clock, np.float32(factor),
np.float32(1.0 - factor))``.  Comparison (``same_result``) is bit for bit; where the reference value
is a NaN only "is a NaN" is required.

The table is written down as hex-float literals (``FAMILIES``).  The searched cases -- contraction,
b-rounding, four of association and the clocks of three device-loss cases -- are what ``search()``
finds with its fixed seed, which tests/test_factor_host.py re-runs; the others are written by hand.
``MUTANTS`` restates the math with one plausible mistake each (fp32 operations through
``np.float32``, fused ones through ``fractions.Fraction``); the host test requires every mutant to
differ from the reference on at least three cases and on at least one case of every form's set
(``form_sets``), which is what keeps the table from going soft.
"""
import functools
import math
import random
import struct
from fractions import Fraction

import numpy as np

from oracle import policy as opolicy

ZD = "zero-division"
INF, NAN = math.inf, math.nan
H = float.fromhex

THRESHOLD = H("0x1.6a09e667f3bcdp+1")      # the divergence threshold of the scaled cases (2.83)
VALUE = H("0x1.3c6ef372fe95p-2")           # the constant factor of the constant-method cases (0.309)
ULP_BELOW_THRESHOLD = H("0x1.6a09e667f3bccp+1")


# ---------------------------------------------------------------- bits, reference, comparison
def bits64(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f32(x):
    with np.errstate(all="ignore"):
        return np.float32(x)


def evaluate(case):
    """ZD, or (factor, new_clock, a, b) as the reference and torch's scalar conversion give them."""
    try:
        f, new_clock = opolicy.factor_and_clock(*case)
    except ZeroDivisionError:
        return ZD
    return f, new_clock, f32(f), f32(1.0 - f)


def _same_number(got, want, bits):
    got, want = float(got), float(want)
    if want != want:
        return got != got
    return bits(got) == bits(want)


def same_result(got, want):
    """Bit for bit, NaN payloads excepted; ZD only equals ZD."""
    if got == ZD or want == ZD:
        return got == ZD and want == ZD
    return (_same_number(got[0], want[0], bits64) and _same_number(got[1], want[1], bits64) and
            _same_number(got[2], want[2], bits32) and _same_number(got[3], want[3], bits32))


def is_finite_case(case):
    """An OK case whose factor and clock are finite (every parameter bit is then compared)."""
    want = evaluate(case)
    return want != ZD and math.isfinite(want[0]) and math.isfinite(want[1])


def kind(case):
    want = evaluate(case)
    return "zd" if want == ZD else "finite" if math.isfinite(want[0]) and math.isfinite(want[1]) else "non-finite"


def is_f32_subnormal(x):
    return x != 0.0 and abs(x) < 2.0 ** -126 and float(f32(x)) == x


def f32_tie(x):
    """x lies exactly half-way between two neighbouring float32 values."""
    lo = float(f32(x))
    other = float(np.nextafter(f32(x), f32(INF if x > lo else -INF)))
    return lo != x and Fraction(x) - Fraction(lo) == Fraction(other) - Fraction(x)


# ---------------------------------------------------------------- the restatement and its mutants
def _fma(a, b, c):
    """a * b + c rounded once (the operands finite; otherwise separately rounded is all there is)."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _div(x, y):
    """IEEE division: what a kernel that lost its zero test would compute."""
    if y != 0.0:
        return x / y
    if x != x or x == 0.0:
        return NAN
    return math.copysign(INF, x) * math.copysign(1.0, y)


MUTANTS = (
    "contract-first-product",       # new_clock = fma(f, pc, (1 - f) * c)
    "contract-second-product",      # new_clock = fma(1 - f, c, f * pc)
    "b-from-a",                     # b = 1.0f - a
    "scale-reassociated",           # (f * loss) / thr
    "loss-le-threshold",            # loss <= thr
    "signed-zero-test",             # x == 0 tested so that -0.0 passes as non-zero
    "clock-as-lerp",                # new_clock = c + f * (pc - c)
    "factor-in-fp32",               # interpolation and scaling in fp32, then widened
    "flush-subnormal-a",            # an fp32-subnormal a flushed to zero
    "flush-subnormal-f32-loss",     # a subnormal float32 device loss read as zero
    "threshold-first",              # the threshold branch runs first and the interpolation's
)                                   # zero test then overwrites its status (a lost ZeroDivisionError)
# Checking the threshold before the interpolation changes nothing observable by itself: either
# order ends in the same ZeroDivisionError or the same product.  "threshold-first" is the form of
# that reordering that does show: the status the threshold branch set is overwritten.

LOSS_READ_MUTANTS = ("flush-subnormal-f32-loss",)     # only a form that reads a float32 device loss can show it


def restate(case, m=None):
    """factor_math restated operation for operation; `m` names the one mistake made."""
    method, value, thr, c, pc, loss, pl = case
    if m == "flush-subnormal-f32-loss" and is_f32_subnormal(loss):
        loss = math.copysign(0.0, loss)

    def zero(x):
        return x == 0.0 and (m != "signed-zero-test" or math.copysign(1.0, x) > 0)

    status, f = "ok", 0.0
    below = loss <= thr if m == "loss-le-threshold" else loss < thr
    if m == "threshold-first" and below and zero(thr):
        status = ZD
    if method == "constant":
        f = float(f32(value)) if m == "factor-in-fp32" else value
    else:
        num, x, y = (pc, c, pc) if method == "clock" else (loss, loss, pl)
        den = x + y
        if m == "threshold-first":
            status = "ok"
        if zero(den):
            status = ZD
        elif m == "factor-in-fp32":
            with np.errstate(all="ignore"):
                f = float(f32(num) / (f32(x) + f32(y))) if float(f32(x) + f32(y)) != 0.0 else NAN
        else:
            f = _div(num, den)
    if status == "ok" and below:
        if zero(thr):
            if m != "threshold-first":      # (there the interpolation has overwritten it: lost)
                status = ZD
        elif m == "scale-reassociated":
            f = _div(f * loss, thr)
        elif m == "factor-in-fp32":
            with np.errstate(all="ignore"):
                f = float(f32(f) * (f32(loss) / f32(thr)))
        else:
            f = f * _div(loss, thr)
    if status == ZD:
        return ZD
    if m == "contract-first-product":
        new_clock = _fma(f, pc, (1.0 - f) * c)
    elif m == "contract-second-product":
        new_clock = _fma(1.0 - f, c, f * pc)
    elif m == "clock-as-lerp":
        new_clock = c + f * (pc - c)
    else:
        new_clock = f * pc + (1.0 - f) * c
    a = f32(f)
    if m == "flush-subnormal-a" and is_f32_subnormal(float(a)):
        a = f32(math.copysign(0.0, float(a)))
    b = f32(1.0) - a if m == "b-from-a" else f32(1.0 - f)
    return f, new_clock, a, b


def catches(case, m):
    return not same_result(restate(case, m), evaluate(case))


# ---------------------------------------------------------------- family properties
def contraction_sensitive(case):
    """Both placements of a fused multiply-add in f * pc + (1 - f) * c differ from the three
    separately rounded operations (exact rational arithmetic, one rounding)."""
    want = evaluate(case)
    if want == ZD:
        return False
    f, new_clock = want[0], want[1]
    c, pc = case[3], case[4]
    return _fma(f, pc, (1.0 - f) * c) != new_clock and _fma(1.0 - f, c, f * pc) != new_clock


def b_double_rounds(case):
    want = evaluate(case)
    return want != ZD and bits32(f32(1.0 - want[0])) != bits32(f32(1.0) - f32(want[0]))


def scaled(case):
    return case[5] < case[2] and case[2] != 0.0


def association_sensitive(case):
    method, value, thr, c, pc, loss, pl = case
    if not scaled(case):
        return False
    f = opolicy.interpolation(method, value, c, pc, loss, pl)
    return f * (loss / thr) != (f * loss) / thr


# ---------------------------------------------------------------- the search (fixed seed)
SEARCH_SEED = 20
# (loss, peer loss) of the first three device-read cases: 0.7f against 1.5, 1e-3f against 0.37f, and
# the fp32 subnormal 2^-140 against the fp32 subnormal 3 * 2^-149
DEVICE_LOSSES = ((H("0x1.666666p-1"), 1.5), (H("0x1.0624dep-10"), H("0x1.7ae148p-2")), (2.0 ** -140, 3 * 2.0 ** -149))


def search():
    """The searched cases, found again from SEARCH_SEED: {family: [case, ...]} in the order of
    FAMILIES.  Clocks are full-mantissa doubles in [1, 1000) (a learner's publish reaches exactly
    such a peer clock: (pc - 1) + 1 == pc), losses in (0.1, threshold)."""
    rng = random.Random(SEARCH_SEED)

    def draw(method, value, thr):
        return (method, value, thr, rng.uniform(1.0, 1000.0), rng.uniform(1.0, 1000.0),
                rng.uniform(0.1, THRESHOLD), rng.uniform(0.1, THRESHOLD))

    def find(count, cfg, wanted):
        out = []
        while len(out) < count:
            case = draw(*cfg)
            if wanted(case):
                out.append(case)
        return out

    plain = [("clock", None, 0.0), ("loss", None, 0.0), ("constant", VALUE, 0.0)]
    scaling = [("clock", None, THRESHOLD), ("loss", None, THRESHOLD), ("constant", VALUE, THRESHOLD)]
    found = {"contraction": [], "b-rounding": [], "association": []}
    for cfg in plain:
        found["contraction"] += find(2, cfg, contraction_sensitive)
    for cfg in scaling:
        found["contraction"] += find(2, cfg, lambda case: contraction_sensitive(case) and scaled(case))
    found["b-rounding"] += find(2, plain[0], b_double_rounds)
    found["b-rounding"] += find(1, plain[1], b_double_rounds)
    found["b-rounding"] += find(1, scaling[0], lambda case: b_double_rounds(case) and scaled(case))
    found["association"] += find(2, scaling[0], association_sensitive)
    found["association"] += find(1, scaling[1], association_sensitive)
    found["association"] += find(1, scaling[2], association_sensitive)
    found["device-loss"] = []
    for loss, peer_loss in DEVICE_LOSSES:          # the losses are given: clocks that make the round
        while True:                                # contraction-sensitive too
            case = ("loss", None, 0.0, rng.uniform(1.0, 1000.0), rng.uniform(1.0, 1000.0), loss, peer_loss)
            if contraction_sensitive(case):
                found["device-loss"].append(case)
                break
    return found


def to_literal(case):
    return tuple(x.hex() if isinstance(x, float) else x for x in case)


def from_literal(lit):
    return tuple(H(x) if isinstance(x, str) and x not in opolicy.METHODS else x for x in lit)


# ---------------------------------------------------------------- the case table
# (method, value, threshold, clock, peer_clock, loss, peer_loss), floats as float.hex literals.
# contraction, b-rounding, the first four of association and the first three of device-loss are
# search()'s (SEARCHED); the rest by hand.
_Z, _1, _3, _7, _75 = "0x0.0p+0", "0x1.0p+0", "0x1.8p+1", "0x1.cp+2", "0x1.ep+2"
_T, _V = "0x1.6a09e667f3bcdp+1", "0x1.3c6ef372fe950p-2"
FAMILIES = {
    # 1. both FMA placements in f * pc + (1 - f) * c change the clock: clock, loss, constant, and
    #    each with the threshold scaling active
    "contraction": [
        ("clock", None, _Z, "0x1.c4ddf4e8713bdp+9", "0x1.5748b10a8e480p+9", "0x1.187ea30102e49p+1", "0x1.48ba1af00240ep+1"),
        ("clock", None, _Z, "0x1.2c1120f46926cp+9", "0x1.bff0f00cf3242p+8", "0x1.08f3df9835a01p-1", "0x1.d7b26dcf36592p+0"),
        ("loss", None, _Z, "0x1.4e3183f4f5200p+8", "0x1.281de5eaa01f4p+6", "0x1.11c3c0c89171dp+1", "0x1.6af7987a96246p-2"),
        ("loss", None, _Z, "0x1.08de6fb30eb09p+9", "0x1.cd548c1ae63eep+9", "0x1.97b7bf24f1d2fp+0", "0x1.5e68b618ae9abp+1"),
        ("constant", _V, _Z, "0x1.84c038687ca5ap+8", "0x1.0c43293d00dc4p+9", "0x1.02085583889c2p+1", "0x1.c92d1c1cd6f25p-1"),
        ("constant", _V, _Z, "0x1.6a325640d6d78p+6", "0x1.81a73ed356903p+7", "0x1.311d6f9b003eep+1", "0x1.f805d72f007a1p+0"),
        ("clock", None, _T, "0x1.1f39552269e83p+8", "0x1.a831478d9c593p+9", "0x1.5ded7d345ca0bp+0", "0x1.005d7a76cf01bp+1"),
        ("clock", None, _T, "0x1.a0be2849d4b34p+7", "0x1.9a0928c8f48c1p+9", "0x1.32e282d01a2c2p+0", "0x1.6a6a785d637f2p+0"),
        ("loss", None, _T, "0x1.3dd22a4e11c63p+9", "0x1.83be613c15b38p+9", "0x1.a2037f47f9939p+0", "0x1.46c2260a5040fp-1"),
        ("loss", None, _T, "0x1.a70520f3539f6p+8", "0x1.5062087a3f303p+9", "0x1.24c51049100fdp+1", "0x1.4544610ff071ap+0"),
        ("constant", _V, _T, "0x1.464ac227c4759p+8", "0x1.452113112a59bp+9", "0x1.188547dd5ea0ap+1", "0x1.bedef60a83c32p+0"),
        ("constant", _V, _T, "0x1.293b4c26d3b41p+9", "0x1.ea0a70b765f37p+8", "0x1.42d57cfb4a1dcp+1", "0x1.6bfe85b5f066ap+0"),
    ],
    # 2. np.float32(1.0 - f) != np.float32(1) - np.float32(f)
    "b-rounding": [
        ("clock", None, _Z, "0x1.39e8215b5a8b7p+6", "0x1.61f5597df8437p+9", "0x1.1a65eaa00fa4dp+0", "0x1.276bcec8060aap+1"),
        ("clock", None, _Z, "0x1.cf8567bb189dcp+6", "0x1.78b10aeefc8c9p+8", "0x1.38cf514919d12p-2", "0x1.8bf2caff4a69ap+0"),
        ("loss", None, _Z, "0x1.d99ae82fcf48ep+8", "0x1.3557cb05e77fap+9", "0x1.208ed354acec2p+0", "0x1.0c698cbb42adbp-1"),
        ("clock", None, _T, "0x1.a8b2d016a931ap+8", "0x1.1bd18e18e5218p+6", "0x1.51327d2d4984dp+1", "0x1.a8cc229272756p+0"),
    ],
    # 3. f * (loss / thr) != (f * loss) / thr; then loss == thr exactly (no scaling) and loss one
    #    ulp below thr (scaling by the largest quotient below 1)
    "association": [
        ("clock", None, _T, "0x1.3993b9b05c810p+9", "0x1.6a11d0ec81edcp+8", "0x1.c01a2a7bf3ed6p+0", "0x1.01222b20d4158p+1"),
        ("clock", None, _T, "0x1.13b0fcffba19ep+9", "0x1.483a0a5d448e5p+8", "0x1.850713862fc06p+0", "0x1.f2eb0c7ad5968p+0"),
        ("loss", None, _T, "0x1.36ae7cc16d655p+9", "0x1.8ca1d0727a3bap+5", "0x1.11be63bd4da09p+0", "0x1.1800f42b46c68p+0"),
        ("constant", _V, _T, "0x1.c18040d871b2ap+8", "0x1.8fed7f77b5444p+9", "0x1.042561d1aa248p+1", "0x1.6787b183a45e0p+1"),
        ("clock", None, _T, _3, _7, _T, _1),
        ("clock", None, _T, _3, _7, "0x1.6a09e667f3bccp+1", _1),
    ],
    # 4. fp32 edges of a: 1e-40 (a subnormal); 2^-151 (a == 0, b == 1); a round-to-nearest-even tie
    #    of the conversion (0.5 + 2^-25 -> 0.5) and one ulp to either side; 1 - f on such a tie
    #    (0.75 + 2^-25 -> 0.75); and subnormal a from clock interpolation (a tiny peer clock)
    "fp32-a": [
        ("constant", "0x1.16c262777579cp-133", _Z, _3, _75, _1, _1),
        ("constant", "0x1.0p-151", _Z, _3, _75, _1, _1),
        ("constant", "0x1.0000010000000p-1", _Z, _3, _75, _1, _1),
        ("constant", "0x1.000000fffffffp-1", _Z, _3, _75, _1, _1),
        ("constant", "0x1.0000010000001p-1", _Z, _3, _75, _1, _1),
        ("constant", "0x1.fffffc0000000p-3", _Z, _3, _75, _1, _1),
        ("clock", None, _Z, _1, "0x1.0p-140", _1, _1),
        ("clock", None, _Z, _3, "0x1.16c262777579cp-133", _1, _1),
        ("clock", None, _Z, "0x1.0p+20", "0x1.0p-125", _1, _1),
    ],
    # 5. fp64 edges: c + pc overflows (f == 0); subnormal clocks (5e-324 and 1e-323) and losses;
    #    new_clock at 2^53, where new_clock + 1.0 == new_clock; a new_clock with a fraction
    "fp64": [
        ("clock", None, _Z, "0x1.fffffffffffffp+1023", "0x1.fffffffffffffp+1023", _1, _1),
        ("clock", None, _Z, "0x0.0000000000001p-1022", "0x0.0000000000002p-1022", _1, _1),
        ("loss", None, _Z, _3, _75, "0x0.0000000000001p-1022", "0x0.0000000000001p-1022"),
        ("loss", None, _Z, "0x1.0p+1", "0x1.2p+3", "0x0.0000000004000p-1022", "0x0.000000000c000p-1022"),
        ("clock", None, _Z, "0x1.0p+53", "0x1.0p+53", _1, _1),
        ("constant", _1, _Z, "0x1.4p+2", "0x1.0p+53", _1, _1),
        ("clock", None, _Z, _3, _75, _1, _1),
    ],
    # 6. ZeroDivisionError in every spelling: c == -pc; both clocks -0.0 (the denominator is
    #    -0.0); loss == -peer_loss; both losses -0.0; thr == 0.0 with loss < 0 (loss / threshold
    #    raises) for each method; thr == -0.0 with loss < 0; the three that do NOT raise (thr == 0.0
    #    with loss == -0.0 and 0.0, thr == -0.0 with loss == 0.0: x < y is false); and the
    #    interpolation raising where the threshold branch would raise too
    "zero-division": [
        ("clock", None, _Z, "0x1.cp+1", "-0x1.cp+1", _1, _1),
        ("clock", None, _Z, "-0x0.0p+0", "-0x0.0p+0", _1, _1),
        ("loss", None, _Z, _3, _7, "0x1.8p-1", "-0x1.8p-1"),
        ("loss", None, _Z, _3, _7, "-0x0.0p+0", "-0x0.0p+0"),
        ("clock", None, _Z, _3, _7, "-0x1.0p+0", _1),
        ("loss", None, _Z, _3, _7, "-0x1.0p+0", _3),
        ("constant", _V, _Z, _3, _7, "-0x1.0p+1", _1),
        ("clock", None, "-0x0.0p+0", _3, _7, "-0x1.0p+0", _1),
        ("loss", None, "-0x0.0p+0", _3, _7, "-0x1.0p+0", _3),
        ("clock", None, _Z, _3, _7, "-0x0.0p+0", _1),
        ("clock", None, _Z, _3, _7, _Z, _1),
        ("clock", None, "-0x0.0p+0", _3, _7, _Z, _1),
        ("clock", None, _Z, "0x1.0p+1", "-0x1.0p+1", "-0x1.0p+0", _1),
    ],
    # 7. non-finite: NaN loss, NaN peer loss, inf peer clock (inf / inf), inf own clock (f == 0,
    #    new_clock == inf), thr == inf (scaled by loss / inf == 0), thr == NaN (no scaling), and
    #    loss == thr == inf (not below: no scaling).  None raises: the status is OK.
    "non-finite": [
        ("loss", None, _Z, _3, _7, "nan", _1),
        ("loss", None, _Z, _3, _7, _1, "nan"),
        ("clock", None, _Z, _3, "inf", _1, _1),
        ("clock", None, _Z, "inf", _7, _1, _1),
        ("clock", None, "inf", _3, _7, _1, _1),
        ("clock", None, "nan", _3, _7, _1, _1),
        ("clock", None, "inf", _3, _7, "inf", _1),
    ],
    # 8. losses that a float32 holds exactly, given as a host double, a device float64 and a device
    #    float32: 0.7f and 1e-3f; fp32-subnormal losses (2^-140, 1.5 * 2^-130, 2^-149) against an
    #    fp32-subnormal, a double-subnormal and an equal peer loss -- widened exactly, not flushed.
    #    The first three have search()'s clocks: the round is contraction-sensitive too (the other
    #    two cannot be: f is 1.0 and 0.5, and both products are exact)
    "device-loss": [
        ("loss", None, _Z, "0x1.2eba04a8a6e20p+9", "0x1.d7faa8c1093fcp+8", "0x1.6666660000000p-1", "0x1.8p+0"),
        ("loss", None, _Z, "0x1.0764afad92787p+5", "0x1.70e433bba099ep+9", "0x1.0624de0000000p-10", "0x1.7ae1480000000p-2"),
        ("loss", None, _Z, "0x1.59d0c30c7a523p+9", "0x1.85566dbdcebdbp+9", "0x1.0p-140", "0x1.8p-148"),
        ("loss", None, _Z, _3, _7, "0x1.8p-130", "0x0.0000000000001p-1022"),
        ("loss", None, _Z, _3, _7, "0x1.0p-149", "0x1.0p-149"),
    ],
}
SEARCHED = {"contraction": 12, "b-rounding": 4, "association": 4, "device-loss": 3}     # how many search() found

CASES = [from_literal(lit) for fam in FAMILIES.values() for lit in fam]
FAMILY_OF = [name for name, fam in FAMILIES.items() for _ in fam]


def family(name):
    return [from_literal(lit) for lit in FAMILIES[name]]


# ---------------------------------------------------------------- which cases every form runs
def cfg_of(case):
    """What one dispatch shares: (method, value, threshold), the doubles by their bits."""
    return case[0], None if case[1] is None else bits64(case[1]), bits64(case[2])


def learner_ok(case):
    """A learner's publish writes clock + 1.0, so through a learner the peer clock must be reachable
    that way exactly (not -0.0, a subnormal or NaN)."""
    pc = case[4]
    return bits64((pc - 1.0) + 1.0) == bits64(pc)


KERNEL_MUTANTS = tuple(m for m in MUTANTS if m not in LOSS_READ_MUTANTS)


def catching(cases, mutants=KERNEL_MUTANTS):
    """The catching subset of `cases`: for every mutant in turn the first case that catches it
    (unless one already chosen does), then the first zero-division, NaN-factor and finite case."""
    chosen = []
    for m in mutants:
        if not any(catches(c, m) for c in chosen):
            chosen.append(next(c for c in cases if catches(c, m)))
    for wanted in ("zd", "non-finite", "finite"):
        if not any(kind(c) == wanted for c in chosen):
            chosen.append(next(c for c in cases if kind(c) == wanted))
    return chosen


CATCHING = catching(CASES)
LEARNER_CATCHING = catching([c for c in CASES if learner_ok(c)])


def groups():
    """The table's cases that share (method, value, threshold) with another: cfg is per dispatch,
    so these are what one dpwa_average_many[_resident] call can hold; clocks and losses vary."""
    by = {}
    for case in CASES:
        by.setdefault(cfg_of(case), []).append(case)
    return [g for g in by.values() if len(g) >= 2]


def isolation(method):
    """[finite, zero-division, finite, NaN factor, finite] of one cfg: the neighbours of an entry
    that does not average, and of one that averages to NaN, must be exactly their own references."""
    g = [c for c in CASES if cfg_of(c) == cfg_of((method, None, 0.0))]
    fin = [c for c in g if kind(c) == "finite"]
    zd = next(c for c in g if kind(c) == "zd")
    nan = next(c for c in g if kind(c) == "non-finite" and evaluate(c)[0] != evaluate(c)[0])
    return [fin[0], zd, fin[1], nan, fin[2]]


MANY_MAX = 8


def many_dispatches():
    """dpwa_average_many: [(name, sizes, cases)], sizes "unequal" (big, 1, big, ...: the begin[]
    scan) or "equal" (all big: the round-robin order), alternating; every group in chunks of at most
    8 entries (the first chunk of the largest group has the maximum, 8), then the isolation rows."""
    out = []
    for g in groups():
        for lo in range(0, len(g), MANY_MAX):
            out.append(("%s/%d" % (g[0][0], len(out)), "unequal" if len(out) % 2 == 0 else "equal", g[lo:lo + MANY_MAX]))
    for method in ("clock", "loss"):
        for sizes in ("unequal", "equal"):
            out.append(("isolation-%s-%s" % (method, sizes), sizes, isolation(method)))
    return out


TOPOLOGIES = {
    "mutual-pair": [(0, 1), (1, 0)],                                               # k_lerp_pair
    "3-cycle": [(0, 1), (1, 2), (2, 0)],                                           # k_lerp_group, 3 buffers
    "four-pairs": [(0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4), (6, 7), (7, 6)],   # k_lerp_group, 8 buffers
    "two-apart": [(0, 1), (2, 3)],                                                 # k_lerp_batch: nothing shared
    "eleven-buffers": [(0, 6), (1, 7), (2, 8), (3, 9), (4, 10), (5, 6)],           # beyond 8: the XCD-grouped batch
}


def resident_plan(picks, cases, start=0):
    """One dpwa_average_many_resident dispatch over `picks` [(me, peer)].  A resident learner has
    one clock and one published loss, so an entry whose two learners are both new takes the next
    case of `cases` exactly; an entry that meets a learner again keeps that learner's clock (and
    published loss) and takes the rest from the next case without using it up.  Returns
    (learners [(clock, published loss)], entries [(me, peer, loss)], the cases the entries really
    are, the index of the first case not used up)."""
    count = 1 + max(max(p) for p in picks)
    clock, pub = [None] * count, [None] * count
    k, entries = start, []
    for a, b in picks:
        g = cases[k % len(cases)]
        if clock[a] is None and clock[b] is None and a != b:
            k += 1
        if clock[a] is None:
            clock[a] = g[3]
        if clock[b] is None:
            clock[b] = g[4]
        if pub[b] is None:
            pub[b] = g[6]
        entries.append((a, b, g[5]))
    pub = [1.0 if x is None else x for x in pub]
    real = [cases[0][:3] + (clock[a], clock[b], loss, pub[b]) for a, b, loss in entries]
    return list(zip(clock, pub)), entries, real, k


def resident_dispatches(name):
    """[(label, learners, entries, cases)] of topology `name`: every group walked until each of its
    cases has been an entry exactly; for the eleven-buffer batch also the isolation rows."""
    picks, out = TOPOLOGIES[name], []
    for g in groups():
        k = 0
        while k < len(g):
            learners, entries, real, k = resident_plan(picks, g, k)
            out.append(("%s/%s/%d" % (name, g[0][0], len(out)), learners, entries, real))
    if name == "eleven-buffers":       # its first five entries share no learner: the isolation row as it is
        learners, entries, real, _ = resident_plan(picks, isolation("clock"))
        out.append((name + "/isolation", learners, entries, real))
    return out


def device_loss_cases():
    return family("device-loss")


@functools.lru_cache(maxsize=None)
def form_sets():
    """{form: (cases it runs, the mutants it can show)} -- tests/test_factor_host.py requires a
    catching case for each of those mutants in each of these sets."""
    sets = {
        "dpwa_factor": (CASES, KERNEL_MUTANTS),
        "dpwa_average f32": (CASES, KERNEL_MUTANTS),
        "dpwa_average bf16, f16, unaligned; dpwa_average_mixed; the worker's dpwa_average": (CATCHING, KERNEL_MUTANTS),
        "dpwa_average_many": ([c for _, _, cases in many_dispatches() for c in cases], KERNEL_MUTANTS),
        "learner, tracked": (LEARNER_CATCHING, KERNEL_MUTANTS),
        "learner, device loss": (device_loss_cases(), LOSS_READ_MUTANTS),
    }
    for name in TOPOLOGIES:
        sets["dpwa_average_many_resident " + name] = ([c for _, _, _, real in resident_dispatches(name) for c in real],
                                                      KERNEL_MUTANTS)
    return sets
