"""Stochastically rounded packed images (include/dpwa_hip.h "stochastic rounding"): the rule restated in numpy on
top of tests/pack_ref.py, its stated properties, and the new entries' exports and refusals.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from dpwa_amd import _lib
from tests import pack_ref as ref
from tests.test_gpu_pack import hard_payload

NEW = ["dpwa_pack_stochastic", "dpwa_average_pack_stochastic", "dpwa_learner_set_pack_rounding"]
NONCES = [0x1234, (0xDEADBEEF << 32) | 5]          # one with a non-zero high word


def fmix32(h):
    h = (h ^ (h >> np.uint32(16))) * np.uint32(0x85EBCA6B)       # uint32 arrays: products wrap
    h = (h ^ (h >> np.uint32(13))) * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def pack(payload, dtype, nonce):
    """pack_ref.pack with the stochastic q step: groups, amax, scale and the two kinds of all-zero group are its."""
    _, scale = ref.pack(payload, dtype)
    per = ref.GROUP // ref.SIZE[dtype]
    x = np.zeros(scale.size * per, dtype=np.float32)
    x[:len(payload) // ref.SIZE[dtype]] = ref.widen(payload, dtype)
    g = x.reshape(-1, per)
    normal = scale > 0                               # a NaN scale and +0.0f: every q = 0
    with np.errstate(all="ignore"):
        amax = np.where(normal, np.abs(g).max(axis=1), np.float32(1.0)).astype(np.float32)
        t = (g * (ref.F127 / amax).astype(np.float32)[:, None]).astype(np.float32)
        f = np.floor(t)
        frac = (t - f).astype(np.float32)
        j = np.arange(x.size, dtype=np.uint64)
        lo = (j ^ np.uint64(nonce)).astype(np.uint32)
        hi = ((j >> np.uint64(32)) ^ np.uint64(nonce >> 32)).astype(np.uint32)
        u = (fmix32(fmix32(lo) ^ hi) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        q = np.clip(np.nan_to_num(f) + (u.reshape(g.shape) < frac), -127, 127)
    return np.where(normal[:, None], q, 0).astype(np.int8).reshape(-1), scale


def image(payload, dtype, nonce):
    """pack_ref.image with that q plane."""
    out = ref.image(payload, dtype)
    q, _ = pack(payload, dtype, nonce)
    out[:q.size] = q.view(np.uint8)
    return out


def roundtrip(payload, dtype, nonce):
    return ref.unpack(*pack(payload, dtype, nonce), dtype, len(payload))


def test_the_hash_is_murmur3s_finaliser():
    """Known values of fmix32 (0 is its fixed point; 1 and 0xFFFFFFFF from the published MurmurHash3)."""
    got = fmix32(np.array([0, 1, 0xFFFFFFFF], dtype=np.uint32))
    assert got.tolist() == [0, 0x514E28B7, 0x81F16F39]


def test_new_entries_are_exported_with_the_headers_arity():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "dpwa_hip.h")).read()
    for name in NEW:
        args = re.search(r"^int %s\(([^)]*)\);" % name, header, re.M).group(1)
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name]) == len(args.split(",")), name


def test_refusals_touch_no_device():
    lib = _lib.load()
    ok, odd, cfg = ctypes.c_void_p(4096), ctypes.c_void_p(4100), _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)

    def average(dtype=_lib.F32, param=ok, n=64, image_out=ok):
        return lib.dpwa_average_pack_stochastic(dtype, param, ok, ok, None, n, ctypes.byref(cfg), ok, 1.0, ok,
                                                ctypes.c_void_p(8192), image_out, None, None, None, 7)

    for call, why in [
            (lambda: lib.dpwa_pack_stochastic(_lib.MIXED, ok, 64, ok, 7, None, None, None), b"DPWA_MIXED"),
            (lambda: lib.dpwa_pack_stochastic(_lib.F32, ok, -1, ok, 7, None, None, None), b"n < 0"),
            (lambda: lib.dpwa_pack_stochastic(_lib.F32, odd, 64, ok, 7, None, None, None), b"16-byte aligned"),
            (lambda: lib.dpwa_pack_stochastic(_lib.F16, ok, 64, odd, 7, None, None, None), b"16-byte aligned"),
            (lambda: average(dtype=_lib.MIXED), b"DPWA_MIXED"), (lambda: average(n=-1), b"n < 0"),
            (lambda: average(param=odd), b"16-byte aligned"), (lambda: average(image_out=odd), b"16-byte aligned"),
            (lambda: lib.dpwa_learner_set_pack_rounding(None, 1, 7), b"NULL learner")]:
        assert call() == _lib.ERR_ARG and why in lib.dpwa_last_error(), lib.dpwa_last_error()
        assert b"stochastic" in lib.dpwa_last_error() or b"set_pack_rounding" in lib.dpwa_last_error()


@pytest.mark.parametrize("nonce", NONCES + [0, 2 ** 64 - 1])
def test_an_element_without_a_fraction_never_moves(nonce):
    """amax = 127 makes inv = 1: integers, zeros of both signs and the padding behind the payload stay."""
    values = np.array([127.0, 3.0, -5.0, 0.0, -0.0, 64.0, -127.0, -1.0, 126.0], dtype=np.float32)
    q, scale = pack(values.view(np.uint8), "f32", nonce)
    assert scale[0] == 1.0 and q[:9].tolist() == values.astype(int).tolist() and not q[9:].any()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_hard_values_stay_in_range_and_within_one_step(dtype):
    """On pack_ref's hard groups: |q| <= 127, the non-normal groups are pack_ref's, q is floor or ceil of what
    nearest rounding saw, and |x' - x| < amax / 127 (1 + 2^-15) in float64 on x' = q * scale (the header's bound)."""
    payload = hard_payload(dtype, 4 * (3 * 1024 + 1))
    x = ref.widen(payload, dtype).astype(np.float64)
    per = ref.GROUP // ref.SIZE[dtype]
    (q0, scale0), moved = ref.pack(payload, dtype), 0
    for nonce in NONCES:
        q, scale = pack(payload, dtype, nonce)
        assert np.array_equal(scale.view(np.uint32), scale0.view(np.uint32)) and q.min() >= -127
        assert np.abs(q.astype(int) - q0).max() == 1 and not q[x.size:].any()
        for g in np.flatnonzero(scale0 > 0):
            xs = x[g * per:(g + 1) * per]
            back = q[g * per:g * per + xs.size].astype(np.float64) * float(scale[g])
            assert np.abs(back - xs).max() < np.abs(xs).max() / 127.0 * (1 + 2.0 ** -15), (g, nonce)
        assert not q.reshape(-1, per)[~(scale0 > 0)].any()
        moved += int((q != q0).sum())
    assert moved > x.size // 4                      # it does round differently from nearest
