"""Host side (no GPU) of tests/test_gpu_forms.py and tests/forms_worker.py: the references those
tests compare the kernels with agree with one another, and the samples have teeth -- few expected
values are NaN (and so exempt from bit comparison), and every plausible wrong kernel restated in
tests/forms_ref.py (``mutant``) differs from the reference where the GPU tests look."""
import numpy as np
import pytest
import torch

from oracle import lerp as olerp
from tests import forms_ref as ref
from tests.mixed_ref import TORCH, tensor_bits, torch_eager

NAN_CAP = 1.0 / 8.0


def torch_cpu(dtype, p_bits, q_bits, f):
    """torch-CPU eager `f * t + (1 - f) * param.data` (pytorch.py:68) on tensors of `dtype`."""
    signed = {4: np.int32, 2: np.int16}[p_bits.dtype.itemsize]
    p = torch.from_numpy(np.array(p_bits).view(signed)).view(TORCH[dtype])
    q = torch.from_numpy(np.array(q_bits).view(signed)).view(TORCH[dtype])
    return tensor_bits(torch_eager(p, q, f))


# ---------------------------------------------------------------- the references agree
@pytest.mark.parametrize("f", ref.FACTORS)
def test_bf16_references_agree_on_every_bit_pattern(f):
    """torch-CPU eager on torch.bfloat16, oracle.lerp.lerp_bf16 and the C oracle over all 65,536
    bf16 patterns against the fixed permutation."""
    want = ref.every_bf16_pattern_expected(f)
    assert ref.same("bf16", torch_cpu("bf16", ref.PERM_BF16, ref.PATTERNS_BF16, f), want)
    assert ref.same("bf16", olerp.c_lerp_bf16_(ref.PERM_BF16.copy(), np.array(ref.PATTERNS_BF16), f), want)
    assert ref.same("bf16", ref.lerp("bf16", ref.PERM_BF16, ref.PATTERNS_BF16, f), want)
    assert 400 < int(ref.is_nan("bf16", want).sum()) < 600


def test_fp32_references_agree_on_the_sample():
    """torch-CPU eager, oracle.lerp.lerp_f32 and the C oracle over 200,003 random fp32 bit patterns
    with every fourth pair hard."""
    p, q = ref.sample("f32", 200_003, 5)
    for f in ref.FACTORS:
        want = ref.lerp("f32", p, q, f)
        assert ref.same("f32", torch_cpu("f32", p, q, f), want), f
        c = olerp.c_lerp_f32_(p.view(np.float32).copy(), q.view(np.float32).copy(), f).view(np.uint32)
        assert ref.same("f32", c, want), f


def test_fp16_reference_is_torch_eager():
    p, q = ref.sample("f16", 4099, 5)
    for f in ref.FACTORS:
        assert ref.same("f16", torch_cpu("f16", p, q, f), ref.lerp("f16", p, q, f)), f


def test_same_rule():
    for d, one, nan_a, nan_b in (("f32", 0x3f800000, 0x7fc00000, 0x7f800001), ("bf16", 0x3f80, 0x7fc0, 0x7f81),
                                 ("f16", 0x3c00, 0x7e00, 0x7c01)):
        t = ref.NUMPY[d]
        a = np.array([one, nan_a, ref.SIGN[d]], t)
        assert ref.same(d, a, np.array([one, nan_b, ref.SIGN[d]], t))            # NaN payloads may differ
        assert not ref.same(d, a, np.array([one, nan_a, 0], t))                 # -0 is not +0
        assert not ref.same(d, a, np.array([one, ref.INF[d], ref.SIGN[d]], t))  # inf is not NaN
        assert ref.mismatches(d, a, np.array([one, nan_a, 0], t)) == [(2, hex(ref.SIGN[d]), "0x0")]


# ---------------------------------------------------------------- the sample
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_sample_puts_hard_values_everywhere(dtype):
    per = ref.PER[dtype]
    for n in ref.all_sizes(dtype):
        p, q = ref.sample(dtype, n, ref.seed_of(dtype, n))
        assert p[-1] == q[-1] == ref.SIGN[dtype]
        hard = np.flatnonzero(np.arange(n) % 4 == ref.hard_phase(ref.seed_of(dtype, n)))
        keep = hard[hard < n - 2]                                  # (the last two may be overwritten)
        values = np.append(ref.HARD[dtype], ref.SUBNORMAL_PAIR[dtype][0])
        assert np.isin(p[keep], values).all() and np.isin(q[keep], values).all()
        if n >= 64:                                                # -0 meets -0 in the body too
            assert ((p == ref.SIGN[dtype]) & (q == ref.SIGN[dtype]))[:n // per * per].any()
        if n % per >= 2:
            want = ref.lerp(dtype, p, q, 0.3)
            assert ref.is_subnormal(dtype, p[n - 2]) and ref.is_subnormal(dtype, q[n - 2])
            assert ref.is_subnormal(dtype, want[n - 2])            # a non-zero subnormal result
            assert want[n - 1] == ref.SIGN[dtype]


def test_every_bf16_pattern_expected_contents():
    """The all-pattern expected arrays hold a result that overflowed from finite inputs, an
    inf - inf NaN, a non-zero subnormal result and a -0."""
    p, q = ref.PERM_BF16, ref.PATTERNS_BF16
    finite = ref.is_finite("bf16", p) & ref.is_finite("bf16", q)
    clean = ~ref.is_nan("bf16", p) & ~ref.is_nan("bf16", q)
    assert p[0x7f80] == 0x7f80 and p[0x8000] == 0x8000             # +inf meets +inf, -0 meets -0
    assert np.array_equal(np.sort(p), q)
    for f in ref.FACTORS:
        want = ref.every_bf16_pattern_expected(f)
        assert (ref.is_subnormal("bf16", want) & finite).any(), f
        if 0.0 <= f <= 1.0:                          # (a negative coefficient turns -0 * b into +0)
            assert want[0x8000] == 0x8000, f
        if f in (1.5, -0.25):
            assert (((want & 0x7fff) == 0x7f80) & finite).any(), f          # overflow of finite inputs
            assert (ref.is_nan("bf16", want) & clean).any(), f              # inf - inf
            assert ref.is_nan("bf16", want[0x7f80]), f


# ---------------------------------------------------------------- the tuples of the GPU tests
def test_tuple_list_covers_every_dtype_and_size():
    assert len(set(ref.TUPLES)) == len(ref.TUPLES) > 500
    for dtype in ref.DTYPES:
        assert {n for d, n, _, _ in ref.TUPLES if d == dtype} == set(ref.all_sizes(dtype))
    with pytest.raises(AssertionError):
        ref.case("f32", 771, 12345, 0.3)                           # an unlisted tuple is refused


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_nan_cap(dtype):
    """For every (dtype, n, seed, factor) the GPU tests use, at most 1/8 of the expected elements
    are NaN.  (A condition on the seeds of forms_ref.SEEDS, not a figure to widen.)"""
    worst = 0.0
    for d, n, seed, f in ref.TUPLES:
        if d == dtype:
            share = ref.nan_share(d, ref.case(d, n, seed, f)[2])
            assert share <= NAN_CAP, (d, n, seed, f, share)
            worst = max(worst, share)
    for f in ref.FACTORS:
        assert ref.nan_share("bf16", ref.every_bf16_pattern_expected(f)) <= NAN_CAP
    print("largest NaN share, %s: %.4f" % (dtype, worst))


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_mutants_differ_in_the_body_at_the_multi_span_size(dtype):
    """At three spans and a tail, for every listed tuple whose factor is neither 0 nor 1 (where
    a product vanishes and several mutants are right): every mutant differs from the reference in
    at least one non-NaN element of the vector body."""
    n = ref.multi_span(dtype)
    body = n // ref.PER[dtype] * ref.PER[dtype]
    seen = 0
    for d, m, seed, f in ref.TUPLES:
        if d != dtype or m != n or f in (0.0, 1.0):
            continue
        p, q, want = ref.case(d, m, seed, f)
        seen += 1
        for name in ref.MUTANTS[dtype]:
            got = ref.mutant(dtype, name, p, q, f)
            bad = ref._bad(dtype, got, want) & ~ref.is_nan(dtype, want)
            assert bad[:body].any(), (name, seed, f)
    assert seen >= 8


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_zero_and_flush_mutants_differ_inside_the_tail(dtype):
    """At every size with a tail of at least 2, for every listed tuple with a factor inside (0, 1)
    (both coefficients positive: a negative one turns the product of -0 into +0 in the reference
    too): the -0 and flush-to-zero mutants differ in the ragged tail (the -0 pair at the end, the
    subnormal pair before it)."""
    per = ref.PER[dtype]
    seen = 0
    for d, n, seed, f in ref.TUPLES:
        if d != dtype or n % per < 2 or not 0.0 < f < 1.0:
            continue
        p, q, want = ref.case(d, n, seed, f)
        seen += 1
        for name in ("neg-zero", "ftz"):
            got = ref.mutant(dtype, name, p, q, f)
            bad = ref._bad(dtype, got, want) & ~ref.is_nan(dtype, want)
            assert bad[n // per * per:].any(), (name, n, seed, f)
    assert seen >= 10


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_the_unmutated_restatement_is_the_reference(dtype):
    """`mutant` with no mutation applied is the reference, so a mutant's difference is its own."""
    n = ref.multi_span(dtype)
    p, q = ref.sample(dtype, n, 3)
    for f in ref.FACTORS:
        assert ref.same(dtype, ref.mutant(dtype, "none", p, q, f), ref.lerp(dtype, p, q, f)), f
