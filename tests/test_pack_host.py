"""tests/pack_ref.py against the codec's rule (include/dpwa_hip.h "packed snapshots") by construction,
and the stateless entries' refusals.  No GPU."""
import ctypes

import numpy as np
import pytest

from dpwa_amd import _lib
from tests import pack_ref as ref

FLT_MAX = np.finfo(np.float32).max


def f32_group(values, fill=0.0):
    """One fp32 group (64 elements) beginning with `values`, as payload bytes."""
    g = np.full(64, fill, dtype=np.float32)
    g[:len(values)] = values
    return g.view(np.uint8)


def test_ties_round_to_even_and_the_ends_reach_127():
    q, scale = ref.pack(f32_group([127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, -127.0]), "f32")
    assert scale[0] == np.float32(1.0)          # amax = 127: inv = 1
    assert q[:8].tolist() == [127, 0, 2, 2, 0, -2, -2, -127]


@pytest.mark.parametrize("amax", [FLT_MAX, np.float32(2.0 ** -100), np.float32(3.0), np.float32(1e-30)])
def test_normal_groups_follow_the_two_divisions(amax):
    payload = f32_group([amax, -amax, amax / np.float32(2)])
    q, scale = ref.pack(payload, "f32")
    assert scale[0] == np.float32(amax) / np.float32(127.0)
    assert q[:2].tolist() == [127, -127] and q[2] in (63, 64)
    back = ref.roundtrip(payload, "f32").view(np.float32)
    assert back[0] == np.float32(127.0) * scale[0] and back[1] == -back[0] and (back[3:] == 0).all()


def test_tiny_groups_flush_to_plus_zero():
    below = np.nextafter(np.float32(2.0 ** -100), np.float32(0))
    payload = np.concatenate([f32_group([below, -below]), f32_group([-0.0, 0.0]), f32_group([1e-45, -1e-45])])
    q, scale = ref.pack(payload, "f32")
    assert not q.any() and (scale.view(np.uint32) == 0).all()
    assert not ref.roundtrip(payload, "f32").any()          # +0.0 everywhere, the signed zeros too


def test_a_non_finite_group_is_nan_and_its_neighbours_are_not():
    payload = np.concatenate([f32_group([1.0, np.nan]), f32_group([1.0, 2.0]), f32_group([-np.inf]), f32_group([4.0])])
    q, scale = ref.pack(payload, "f32")
    assert scale.view(np.uint32)[[0, 2]].tolist() == [0x7FC00000] * 2 and not q[:64].any() and not q[128:192].any()
    back = ref.roundtrip(payload, "f32").view(np.float32).reshape(4, 64)
    assert np.isnan(back[[0, 2]]).all() and np.isfinite(back[[1, 3]]).all()
    assert abs(back[1, 0] - 1.0) <= 2.0 / 254 * (1 + 2.0 ** -22) and back[1, 1] > 1.99 and back[3, 0] > 3.99


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_error_bound_and_group_size_on_normal_values(dtype):
    """A group is 256 bytes whatever the element size, and the planes have the header's sizes, for all three
    dtypes.  On float32 N(0,1): |x' - x| <= amax/254 (1 + 2^-22), in float64 on the model itself (x' = q * scale
    before any rounding of the product).

    That figure leans on N(0,1) in float32 having no element near a tie of x * inv.  N(0,1) rounded to bf16 or
    fp16 has few mantissa bits and does land on exact ties, so for those payloads the bound is the rule's own
    reach, from its three roundings (u = 2^-24, all in units of the exact amax/127): inv = 127/amax (1 + e1),
    p = fl(x * inv) = x inv (1 + e2) with |p| < 127.5, q = rint(p) with |q - p| <= 0.5 and |q| <= 127,
    scale = amax/127 (1 + e3), every |e| <= u.  Then x' - x = q (1 + e3) - p / ((1 + e1)(1 + e2)), so
    |x' - x| <= 0.5 + 127 u + 127.5 * 2.001 u < 0.5 + 383 u."""
    rng = np.random.default_rng(7)
    n = 3 * 4096 // ref.SIZE[dtype] + 5 * (256 // ref.SIZE[dtype]) + 3
    payload = ref.narrow(rng.standard_normal(n).astype(np.float32), dtype)
    x = ref.widen(payload, dtype).astype(np.float64)
    q, scale = ref.pack(payload, dtype)
    per = 256 // ref.SIZE[dtype]
    assert scale.size == 16 * 4 and q.size == 4 * 4096 // ref.SIZE[dtype]
    assert ref.image(payload, dtype).size == ref.image_bytes(dtype, len(payload)) == 4096 * (2 if dtype == "f32" else 3)
    for g in range(-(-n // per)):
        xs = x[g * per:(g + 1) * per]
        amax = np.abs(xs).max()
        assert float(scale[g]) == float(np.float32(amax) / np.float32(127.0))
        back = q[g * per:g * per + xs.size].astype(np.float64) * float(scale[g])
        bound = amax / 254.0 * (1 + 2.0 ** -22) if dtype == "f32" else amax / 127.0 * (0.5 + 383 * 2.0 ** -24)
        assert np.abs(back - xs).max() <= bound, (g, np.abs(back - xs).max(), bound)
    assert not q[n:].any() and not scale[-(-n // per):].any()      # past the end: zeros


def test_stateless_entries_refuse_by_name():
    lib = _lib.load()
    out = ctypes.c_int64()
    assert lib.dpwa_pack_bytes(_lib.F32, 1025, ctypes.byref(out)) == 0 and out.value == 8192
    assert lib.dpwa_pack_bytes(_lib.BF16, 2 ** 26, ctypes.byref(out)) == 0
    assert out.value == ref.image_bytes("bf16", 2 ** 27)
    aligned, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    for call, why in [
            (lambda: lib.dpwa_pack_bytes(_lib.MIXED, 4096, ctypes.byref(out)), b"DPWA_MIXED"),
            (lambda: lib.dpwa_pack(_lib.MIXED, aligned, 4096, aligned, None, None, None), b"DPWA_MIXED"),
            (lambda: lib.dpwa_unpack(_lib.MIXED, aligned, 4096, aligned, 1, None, None, None), b"DPWA_MIXED"),
            (lambda: lib.dpwa_pack(_lib.F32, odd, 64, aligned, None, None, None), b"16-byte aligned"),
            (lambda: lib.dpwa_pack(_lib.F32, aligned, 64, odd, None, None, None), b"16-byte aligned"),
            (lambda: lib.dpwa_unpack(_lib.F16, odd, 64, aligned, 1, None, None, None), b"16-byte aligned"),
            (lambda: lib.dpwa_unpack(_lib.F16, aligned, 64, aligned, 0, None, None, None), b"max_blocks")]:
        assert call() == _lib.ERR_ARG and why in lib.dpwa_last_error(), lib.dpwa_last_error()
