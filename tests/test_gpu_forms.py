"""Every form of the averaging kernel on hard values, with guard bands, for float32, bfloat16 and
float16: host and device coefficients, the ragged tail, the element-wise kernel for unaligned
views, the fused average plain and write-through, the batched dispatch in its span orders, the
pair and group kernels of resident learners for every source count, and the mixed-dtype kernel.

The operands are random bit patterns with signed zeros, subnormals, infinities and the largest
finite values in every fourth element of the vector body and the ragged tail alike
(tests/forms_ref.py); the expected values are the host references' (never the library's or torch's
on the device); tests/test_forms_host.py shows on the CPU that those references agree and that
plausible wrong kernels differ from them on exactly these operands.  Bar: NaN positions coincide,
every other element bit-equal.

Every destination lies between two 8-KiB bands of 0xA5 -- the widest span any instantiation
stores -- that must be intact after the call: the streaming kernels rely on the buffer
descriptor's range check to drop the lanes past the end, and an allocation of exactly n elements
would hide a lost check inside the allocator's rounding.  Every source is compared with its host
copy afterwards.

Shapes (per = elements of a 16-byte item, one-wave spans of 64 items): per - 1, per + 1, 64 per,
64 per + 1, 3 * 64 per + per - 1, and for the resident forms 8 * 64 per and 9 * 64 per + 1.  The
forms themselves are the functions of tests/forms_worker.py, which tests/test_gpu_variants.py runs
again under every environment knob."""
import numpy as np
import pytest
import torch

from dpwa_amd import _lib
from oracle import policy as opolicy
from tests import forms_ref as ref
from tests import forms_worker as forms
from tests import mixed_ref
from tests.test_gpu_f16 import FUSED
from tests.test_gpu_kernels import average_slot
from tests.test_gpu_mixed import average_mixed, expected, layout_of, payloads, tens

pytestmark = pytest.mark.gpu

OFF = _lib.SLOT_PAYLOAD_OFFSET


# ---------------------------------------------------------------- 1. every bf16 bit pattern
@pytest.mark.parametrize("f", ref.FACTORS)
def test_every_bf16_bit_pattern(f):
    """Peer: all 65,536 bf16 bit patterns; parameters: a fixed permutation of them (+inf meets
    +inf, -0 meets -0); nine factors, the last two overflowing to inf and producing inf - inf.
    Through dpwa_lerp_bf16_host and through dpwa_lerp_bf16 with dpwa_factor's coefficient block.
    bf16 subnormals are fp32 subnormals: every one of them must survive both products and the sum."""
    forms.run_every_bf16_pattern(f)


# ---------------------------------------------------------------- 2. plain lerp
@pytest.mark.parametrize("f", ref.PLAIN_FACTORS)
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_plain_lerp(dtype, f):
    """Host and device coefficients at every size: the ragged tail's scalar form meets -0 * -0 and a
    subnormal pair, the body every hard value; at 0 and 1 a product vanishes (0 * inf = NaN, 0 * -x
    = -0), at 1.5 one coefficient is negative."""
    for n in ref.sizes(dtype):
        forms.run_plain(dtype, n, f)


# ---------------------------------------------------------------- 3. unaligned views
@pytest.mark.parametrize("k", range(len(ref.UNALIGNED_OFFSETS)), ids=["%d-%d" % o for o in ref.UNALIGNED_OFFSETS])
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_unaligned_views(dtype, k):
    """1,003 elements at element offsets off the 16-byte alignment: the element-wise kernel with
    host, device and fused coefficients, with and without a write-through snapshot, and its
    zero-division branch; nothing outside the views changes.  (Offsets (0, 3) without a snapshot
    leave everything aligned: that call takes the streaming kernel.)"""
    forms.run_unaligned(dtype, k)


# ---------------------------------------------------------------- 4. dpwa_average
@pytest.mark.parametrize("write_through", [False, True], ids=["plain", "write-through"])
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_average(dtype, write_through):
    """dpwa_average at every size over the five policy cases of test_gpu_f16.FUSED and the
    zero-division no-op: parameters, new clock, dpwa_coef and status against the oracle policy,
    the write-through snapshot equal to the parameters (unchanged ones in the no-op round)."""
    for n in ref.sizes(dtype):
        forms.run_average(dtype, n, write_through)


# ---------------------------------------------------------------- 5. dpwa_average_many
@pytest.mark.parametrize("zero_division", [False, True], ids=["", "one-zero-division"])
@pytest.mark.parametrize("write_through", [False, True], ids=["plain", "write-through"])
@pytest.mark.parametrize("group", ["two", "three", "equal", "nine"])
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_average_many(dtype, group, write_through, zero_division):
    """Two and three entries of different sizes (the begin[] scan), two of equal size (the
    round-robin order) and the worker's nine spans beside one, each entry with its own clocks;
    optionally entry 0 divides by zero and stays while the others average."""
    forms.run_many(dtype, group, write_through, zero_division)


# ---------------------------------------------------------------- 6. dpwa_average_many_resident
@pytest.mark.parametrize("name", list(ref.RESIDENT))
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_average_many_resident(dtype, name):
    """One entry (the single kernel out of place), two sharing nothing (k_lerp_batch), the mutual
    pair (k_lerp_pair), k_lerp_group with 3 to 8 source buffers, eleven buffers (the XCD-grouped
    batch) and a group with zero-dividing entries, at every size up to a whole and a partial XCD
    group of eight spans: each entry equal to the reference and to the same average done alone."""
    for n in ref.resident_sizes(dtype):
        forms.run_resident(dtype, name, n)


# ---------------------------------------------------------------- 7. dpwa_average_mixed
@pytest.mark.parametrize("write_through", [False, True], ids=["plain", "write-through"])
@pytest.mark.parametrize("name", sorted(mixed_ref.LAYOUTS))
def test_average_mixed(name, write_through):
    """The layouts and payloads of tests/test_gpu_mixed.py (hard values in the first and last
    16-byte word of every segment) with guard bands round the parameters and the snapshot."""
    spec = mixed_ref.LAYOUTS[name]
    lay, total = layout_of(spec)
    p_h, q_h = payloads(name)
    for case in FUSED:
        method, value, thr, my_clock, peer_clock, loss, peer_loss = case
        f, new_clock = opolicy.factor_and_clock(method, value, thr, my_clock, peer_clock, loss, peer_loss)
        p, check = ref.guarded(total)
        p.copy_(tens(p_h))
        slot = average_slot(tens(q_h).to(forms.DEV), peer_clock, peer_loss)
        snap, check_snap = ref.guarded(total) if write_through else (None, None)
        c, got_clock = average_mixed(lay, p, slot, case, snap)
        problem = mixed_ref.same(spec, p.cpu().numpy(), expected(name, f))
        assert problem is None, (case, problem)
        forms.check_coef(c, f, new_clock, got_clock, case)
        check(case)
        if write_through:
            assert torch.equal(snap, p), case
            check_snap(case)
        assert np.array_equal(slot[OFF:].cpu().numpy(), q_h), "the peer's slot is only read"
