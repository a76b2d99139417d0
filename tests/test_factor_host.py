"""Host side (no GPU) of tests/test_gpu_factor.py and tests/factor_worker.py: the case table of
tests/factor_ref.py still is what it says -- every literal evaluates, every case has its family's
property, the search reproduces the searched literals -- and it has teeth: every plausible wrong
factor_math restated there (``MUTANTS``) differs from the reference on at least three cases and on
at least one case of the set that each kernel form runs.  These are conditions on the table, checked
against ``oracle.policy.factor_and_clock`` and exact rational arithmetic, never on the code under
test."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import policy as opolicy
from tests import factor_ref as ref

ONE_HALF_ULP_F32 = Fraction(1, 2 ** 25)


def test_table_size_and_shape():
    assert 40 <= len(ref.CASES) <= 64
    assert len({repr(ref.to_literal(c)) for c in ref.CASES}) == len(ref.CASES)       # no case twice
    for name, fam in ref.FAMILIES.items():
        assert 4 <= len(fam) <= 13, name
        for lit in fam:
            assert len(lit) == 7 and lit[0] in opolicy.METHODS, lit
            assert all(x is None or isinstance(x, str) for x in lit[1:]), lit       # hex literals only
            assert (lit[1] is None) == (lit[0] != "constant"), lit
            assert ref.to_literal(ref.from_literal(lit))[0] == lit[0]


@pytest.mark.parametrize("i", range(len(ref.CASES)))
def test_case_evaluates_and_the_restatement_is_the_reference(i):
    """No exception but ZeroDivisionError; the expectation is factor_and_clock recomputed here; and
    factor_math restated without a mistake equals it, so a mutant's difference is its own."""
    case = ref.CASES[i]
    method, value, thr, c, pc, loss, pl = case
    want = ref.evaluate(case)
    try:
        f = opolicy.interpolation(method, value, c, pc, loss, pl)
        if loss < thr:
            f = f * (loss / thr)
        again = (f, f * pc + (1 - f) * c, np.float32(f), np.float32(1.0 - f))
    except ZeroDivisionError:
        again = ref.ZD
    assert ref.same_result(again, want) and ref.same_result(want, again), case
    assert ref.same_result(ref.restate(case), want), case
    if want == ref.ZD:
        assert ref.kind(case) == "zd"


def test_same_result_rule():
    nan_a, nan_b = float.fromhex("nan"), -math.nan
    ok = (0.5, 3.0, np.float32(0.5), np.float32(0.5))
    assert ref.same_result(ok, ok) and not ref.same_result(ok, ref.ZD) and not ref.same_result(ref.ZD, ok)
    assert ref.same_result((nan_b, 3.0, np.float32(nan_b), ok[3]), (nan_a, 3.0, np.float32(nan_a), ok[3]))
    assert not ref.same_result((0.5, 3.0, ok[2], ok[3]), (nan_a, 3.0, ok[2], ok[3]))       # a number is not NaN
    assert not ref.same_result((-0.0, 3.0, ok[2], ok[3]), (0.0, 3.0, ok[2], ok[3]))        # -0 is not +0
    assert not ref.same_result((math.inf, 3.0, ok[2], ok[3]), (nan_a, 3.0, ok[2], ok[3]))  # inf is not NaN
    assert not ref.same_result((0.5, 3.0, ok[2], np.float32(-0.0)), (0.5, 3.0, ok[2], np.float32(0.0)))


# ---------------------------------------------------------------- the families' properties
def test_contraction_family():
    """Both FMA placements change the clock (Fraction arithmetic, one rounding), for clock, loss and
    constant interpolation, each without and with the threshold scaling active."""
    seen = set()
    for case in ref.family("contraction"):
        method, value, thr, c, pc, loss, pl = case
        f, new_clock = opolicy.factor_and_clock(*case)
        first = float(Fraction(f) * Fraction(pc) + Fraction((1.0 - f) * c))
        second = float(Fraction(1.0 - f) * Fraction(c) + Fraction(f * pc))
        assert first != new_clock and second != new_clock, case
        assert ref.catches(case, "contract-first-product") and ref.catches(case, "contract-second-product"), case
        seen.add((method, loss < thr))
    assert seen == {(m, s) for m in opolicy.METHODS for s in (False, True)}


def test_b_rounding_family():
    for case in ref.family("b-rounding"):
        f = opolicy.factor_and_clock(*case)[0]
        assert np.float32(1.0 - f) != np.float32(1) - np.float32(f), case
        assert ref.catches(case, "b-from-a"), case


def test_association_family():
    fam = ref.family("association")
    for case in fam[:4]:
        method, value, thr, c, pc, loss, pl = case
        f = opolicy.interpolation(method, value, c, pc, loss, pl)
        assert loss < thr and f * (loss / thr) != (f * loss) / thr, case
        assert ref.catches(case, "scale-reassociated"), case
    assert {c[0] for c in fam[:4]} == set(opolicy.METHODS)
    equal, below = fam[4], fam[5]
    assert equal[5] == equal[2] and opolicy.factor_and_clock(*equal)[0] == 0.7       # loss == thr: no scaling
    assert below[5] == math.nextafter(below[2], 0.0) and below[5] / below[2] == math.nextafter(1.0, 0.0)
    assert opolicy.factor_and_clock(*below)[0] == 0.7 * math.nextafter(1.0, 0.0) != 0.7


def test_fp32_edges_of_a():
    fam = ref.family("fp32-a")
    res = [ref.evaluate(c) for c in fam]
    f = [r[0] for r in res]
    assert all(ref.is_f32_subnormal(float(r[2])) for r in (res[0], res[6], res[7], res[8]))     # a is subnormal
    assert f[0] == 1e-40 and float(res[0][2]) != f[0]                                # and was rounded
    assert 0.0 < f[1] < 2.0 ** -150 and ref.bits32(res[1][2]) == 0 and res[1][3] == np.float32(1.0)
    assert ref.f32_tie(f[2]) and Fraction(f[2]) - Fraction(0.5) == ONE_HALF_ULP_F32
    assert res[2][2] == np.float32(0.5)                                              # the tie goes to even
    assert f[3] == math.nextafter(f[2], 0.0) and f[4] == math.nextafter(f[2], 1.0)
    assert res[3][2] == np.float32(0.5) and res[4][2] == np.nextafter(np.float32(0.5), np.float32(1))
    assert ref.f32_tie(1.0 - f[5]) and Fraction(1.0 - f[5]) == 1 - Fraction(f[5])    # 1 - f exact, on a tie
    assert res[5][3] == np.float32(0.75)
    for i in (0, 6, 7, 8):
        assert ref.catches(fam[i], "flush-subnormal-a"), fam[i]


def test_fp64_edges():
    fam = ref.family("fp64")
    res = [ref.evaluate(c) for c in fam]
    assert math.isinf(fam[0][3] + fam[0][4]) and ref.bits64(res[0][0]) == 0 and res[0][1] == fam[0][3]
    tiny = 5e-324
    assert (fam[1][3], fam[1][4]) == (tiny, 2 * tiny) and res[1][1] == tiny
    assert fam[2][5] == fam[2][6] == tiny and res[2][0] == 0.5
    assert 0.0 < fam[3][5] < 2.0 ** -1022 and 0.0 < fam[3][6] < 2.0 ** -1022 and res[3][0] == 0.25
    for r in (res[4], res[5]):
        assert r[1] == 2.0 ** 53 and r[1] + 1.0 == r[1]              # the written-ahead clock does not move
    assert res[6][1] != math.floor(res[6][1])                        # a clock with a fraction


def test_zero_division_family():
    fam = ref.family("zero-division")
    res = [ref.evaluate(c) for c in fam]
    raising = [0, 1, 2, 3, 4, 5, 6, 7, 8, 12]
    assert [i for i, r in enumerate(res) if r == ref.ZD] == raising
    assert fam[0][3] == -fam[0][4] != 0.0
    assert ref.bits64(fam[1][3] + fam[1][4]) == ref.bits64(-0.0)                     # the denominator is -0.0
    assert fam[2][5] == -fam[2][6] != 0.0
    assert ref.bits64(fam[3][5] + fam[3][6]) == ref.bits64(-0.0)
    for i in (4, 5, 6):                                              # thr == +0.0, loss < 0, every method
        assert ref.bits64(fam[i][2]) == 0 and fam[i][5] < 0.0
    assert {fam[i][0] for i in (4, 5, 6)} == set(opolicy.METHODS)
    for i in (7, 8):                                                 # thr == -0.0, loss < 0
        assert ref.bits64(fam[i][2]) == ref.bits64(-0.0) and fam[i][5] < 0.0
    for i, thr, loss in ((9, 0.0, -0.0), (10, 0.0, 0.0), (11, -0.0, 0.0)):           # x < y is false: no raise
        assert ref.bits64(fam[i][2]) == ref.bits64(thr) and ref.bits64(fam[i][5]) == ref.bits64(loss)
        assert res[i][0] == 0.7
    assert fam[12][3] == -fam[12][4] and fam[12][5] < fam[12][2] == 0.0              # both branches would raise
    for i in (1, 3, 7, 8):
        assert ref.catches(fam[i], "signed-zero-test"), fam[i]
    for i in (4, 5, 7, 8):
        assert ref.catches(fam[i], "threshold-first"), fam[i]
    for i in (9, 10, 11):
        assert ref.catches(fam[i], "loss-le-threshold"), fam[i]


def test_non_finite_family():
    fam = ref.family("non-finite")
    res = [ref.evaluate(c) for c in fam]
    assert ref.ZD not in res                                         # none raises: the status is OK
    for i in (0, 1, 2):
        assert math.isnan(res[i][0]) and math.isnan(res[i][1]) and np.isnan(res[i][2]) and np.isnan(res[i][3])
    assert math.isnan(fam[0][5]) and math.isnan(fam[1][6]) and math.isinf(fam[2][4])
    assert math.isinf(fam[3][3]) and res[3][0] == 0.0 and res[3][1] == math.inf
    assert math.isinf(fam[4][2]) and ref.bits64(res[4][0]) == 0 and res[4][1] == 3.0   # scaled by loss / inf == 0
    assert math.isnan(fam[5][2]) and res[5][0] == 0.7                                # thr NaN: no scaling
    assert fam[6][2] == fam[6][5] == math.inf and res[6][0] == 0.7                   # not below: no scaling
    assert ref.catches(fam[6], "loss-le-threshold")


def test_device_loss_family():
    """Every loss is a float32 exactly (the float32 spelling's reference input is
    float(np.float32(loss)) == loss); three are fp32 subnormals, which a flushing read loses."""
    fam = ref.device_loss_cases()
    for case in fam:
        assert case[0] == "loss" and float(np.float32(case[5])) == case[5], case
        assert ref.kind(case) == "finite" and ref.learner_ok(case), case
    assert [(c[5], c[6]) for c in fam[:3]] == list(ref.DEVICE_LOSSES)
    assert all(ref.contraction_sensitive(c) for c in fam[:3])        # a contracted clock shows here too
    sub = [c for c in fam if ref.is_f32_subnormal(c[5])]
    assert len(sub) == 3 and all(ref.catches(c, "flush-subnormal-f32-loss") for c in sub)
    assert any(0.0 < c[6] < 2.0 ** -1022 for c in sub) and any(ref.is_f32_subnormal(c[6]) for c in sub)


# ---------------------------------------------------------------- the table has teeth
@pytest.mark.parametrize("m", ref.MUTANTS)
def test_mutant_is_caught_by_three_cases(m):
    caught = [c for c in ref.CASES if ref.catches(c, m)]
    assert len(caught) >= 3, (m, len(caught))


@pytest.mark.parametrize("form", sorted(ref.form_sets()))
def test_every_form_runs_a_catching_case_for_every_mutant(form):
    """Per form -- the batch and group assignments as the GPU tests make them, the derived entries
    of the shared-learner topologies included."""
    cases, mutants = ref.form_sets()[form]
    for m in mutants:
        assert any(ref.catches(c, m) for c in cases), (form, m)
    kinds = {ref.kind(c) for c in cases}
    if mutants == ref.KERNEL_MUTANTS:
        assert kinds == {"finite", "zd", "non-finite"}, (form, kinds)


def test_dispatch_assignments():
    """One cfg per dispatch, at most 8 entries, the maximum reached, both size patterns, and the
    isolation rows: a zero-division and a NaN-factor entry, each between finite ones."""
    many = ref.many_dispatches()
    assert {s for _, s, _ in many} == {"unequal", "equal"} and max(len(c) for _, _, c in many) == ref.MANY_MAX
    for name, _, cases in many:
        assert 2 <= len(cases) <= ref.MANY_MAX and len({ref.cfg_of(c) for c in cases}) == 1, name
        if name.startswith("isolation"):
            assert [ref.kind(c) for c in cases] == ["finite", "zd", "finite", "non-finite", "finite"], name
            assert math.isnan(ref.evaluate(cases[3])[0])
    in_groups = [c for g in ref.groups() for c in g]
    for name, picks in ref.TOPOLOGIES.items():
        runs = ref.resident_dispatches(name)
        exact = set()
        for label, learners, entries, real in runs:
            assert [(a, b) for a, b, _ in entries] == picks and len({ref.cfg_of(c) for c in real}) == 1, label
            for (a, b, loss), case in zip(entries, real):
                assert case[3:] == (learners[a][0], learners[b][0], loss, learners[b][1]), label
            exact |= {repr(c) for c in real}
        assert all(repr(c) in exact for c in in_groups), name        # every grouped case is an entry exactly
    rows = [real for label, _, _, real in ref.resident_dispatches("eleven-buffers") if label.endswith("/isolation")][0]
    assert [ref.kind(c) for c in rows[:5]] == ["finite", "zd", "finite", "non-finite", "finite"]


def test_catching_subsets_are_small():
    assert len(ref.CATCHING) <= 12 and len(ref.LEARNER_CATCHING) <= 12
    assert all(ref.learner_ok(c) for c in ref.LEARNER_CATCHING)


# ---------------------------------------------------------------- the search reproduces the literals
def test_search_reproduces_the_literals():
    found = ref.search()
    assert set(found) == set(ref.SEARCHED)
    for name, count in ref.SEARCHED.items():
        assert len(found[name]) == count
        assert [ref.to_literal(c) for c in found[name]] == [ref.to_literal(c) for c in ref.family(name)[:count]], name
