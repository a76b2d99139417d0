"""Skipping a non-finite peer, without a device: tests/finite_ref.py's bit-pattern rule against
``np.isfinite``; each of the six wrong kernels told from the right one by an input that
tests/test_gpu_finite.py runs; and the plumbing of the switch -- the new C-ABI entries with the
header's arities, ABI version 11, bad arguments reported before any device is touched, the Python
refusals of ``relay-avg`` by name, the adapter handing the switch to its connection."""
import ctypes
import re

import numpy as np
import pytest
import torch

from dpwa_amd import DpwaConnection, DpwaPyTorchAdapter, _lib
from dpwa_amd.group import LocalGroup
from tests import finite_ref as ref
from tests.test_distance_host import expect_arg_error, layout, write_cfg

NEW = ["dpwa_check_finite", "dpwa_check_finite_mixed", "dpwa_learner_set_finite_check", "dpwa_learner_finite_skips",
       "dpwa_node_set_finite_check"]


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_every_16_bit_pattern_against_numpy(dtype):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    assert np.array_equal(ref.nonfinite(dtype, bits), ~np.isfinite(ref.as_float(dtype, bits)))
    assert int(ref.nonfinite(dtype, bits).sum()) == (2 << 7 if dtype == "bf16" else 2 << 10)


def test_fp32_edges_against_numpy():
    """Every sign x {exponent 254, 255} x mantissa {0, 1, 2^22, 2^23 - 1}, the subnormals and zeros."""
    pats = [s << 31 | e << 23 | m for s in (0, 1) for e in (254, 255) for m in (0, 1, 1 << 22, (1 << 23) - 1)]
    pats += [s << 31 | m for s in (0, 1) for m in (0, 1, 1 << 22, (1 << 23) - 1)]
    pats += [0x00007f80, 0x00007c00, 0x3f807f80]
    bits = np.array(pats, dtype=np.uint32)
    got = ref.nonfinite("f32", bits)
    assert np.array_equal(got, ~np.isfinite(bits.view(np.float32)))
    assert int(got.sum()) == 8 and not got[16:].any()


def test_a_mixed_payload_is_judged_segment_by_segment():
    for spec in ref.MIXED.values():
        segs, total, cases = ref.mixed_cases(spec)
        for name, payload, want in cases:
            parts = [~np.isfinite(ref.as_float(d, np.ascontiguousarray(payload[off:off + length]).view(ref.NUMPY[d])))
                     for d, off, length, _ in segs]
            assert any(p.any() for p in parts) == want == ref.model_mixed(segs, payload), (spec, name)


def test_the_model_is_the_reference_on_every_gpu_input():
    for dtype in ref.DTYPES:
        for n in ref.sizes(dtype):
            for name, bits, want in ref.cases(dtype, n):
                assert ref.model(dtype, bits, n) == want, (dtype, n, name)


# ---------------------------------------------------------------- the wrong kernels
def told_by(mutant):
    """The GPU test's inputs on which the wrong kernel's answer is not the reference's."""
    out = []
    for dtype in ref.DTYPES:
        for n in ref.sizes(dtype):
            for name, bits, want in ref.cases(dtype, n):
                if ref.model(dtype, bits, n, mutant) != want:
                    out.append((dtype, n, name))
    for spec_name, spec in ref.MIXED.items():
        segs, _, cases = ref.mixed_cases(spec)
        for name, payload, want in cases:
            if ref.model_mixed(segs, payload, mutant) != want:
                out.append(("mixed", spec_name, name))
    return out


@pytest.mark.parametrize("mutant", [m for m in ref.MUTANTS if m != "stale-veto"])
def test_every_wrong_pass_is_told_by_a_gpu_input(mutant):
    told = told_by(mutant)
    print(mutant, len(told), told[:4])
    assert told, mutant
    if mutant == "tail-ignored":
        assert all("last" in name or "first" in name or "half" in name for _, _, name in told)
    if mutant == "past-the-end":
        assert {name for _, _, name in told} == {"nan-just-past-n", "inf-just-past-n"}
    if mutant == "16-bit-test-on-f32":
        assert {d for d, _, _ in told} == {"f32", "mixed"}
        assert any(name == "16-bit-inf-in-low-half" for _, _, name in told)
        assert any(name == "16-bit-inf-in-f32-low-halves" for _, _, name in told)
    if mutant == "high-half-only":
        assert {d for d, _, _ in told} >= {"bf16", "f16"} and all("even" in n or "first" in n or "last" in n for _, _, n in told)
    if mutant == "inf-not-counted":
        assert all("inf" in name for _, _, name in told)
        for dtype in ref.DTYPES:
            assert any(d == dtype for d, _, _ in told)


def test_a_stale_veto_is_told_by_the_round_after():
    """The GPU test's learner rounds: a non-finite peer, then a finite one.  The right rule skips the
    first only; a kernel that honours the word of the round before skips both."""
    assert ref.rounds([True, False]) == [True, False]
    assert ref.rounds([True, False], "stale-veto") == [True, True]
    assert ref.rounds([False] * 6) == ref.rounds([False] * 6, "stale-veto") == [False] * 6
    assert ref.rounds([False, True, True, False, False]) == [False, True, True, False, False]


# ---------------------------------------------------------------- plumbing
def test_new_symbols_exist_with_the_headers_arities():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    decls = dict(re.findall(r"\bint\s+(dpwa_\w+)\s*\(([^)]*)\)\s*;", text))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in decls and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name]) == decls[name].count(",") + 1, name
    assert lib.dpwa_abi_version() == 11 and _lib.ABI_VERSION == 11
    assert re.search(r"#define DPWA_STATUS_PEER_NONFINITE 2\b", open(_lib.HEADER_PATH).read())
    assert _lib.STATUS_PEER_NONFINITE == 2
    assert ctypes.sizeof(_lib.Coef) == 32 and ctypes.sizeof(_lib.Header) == 256


def test_bad_arguments_are_reported_without_a_device():
    """Non-NULL pointers here are host addresses no entry may touch: every call must fail first."""
    buf = (ctypes.c_char * 4096)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    a = ctypes.c_void_p(addr)
    expect_arg_error("dpwa_check_finite", _lib.F32, None, 8, a, 1, None, None, None)
    expect_arg_error("dpwa_check_finite", _lib.F32, a, 8, None, 1, None, None, None)
    expect_arg_error("dpwa_check_finite", _lib.F32, a, -1, a, 1, None, None, None)
    expect_arg_error("dpwa_check_finite", _lib.F32, a, 8, a, 0, None, None, None)                 # stamp 0
    expect_arg_error("dpwa_check_finite", _lib.F32, a, 8, ctypes.c_void_p(addr + 2), 1, None, None, None)
    expect_arg_error("dpwa_check_finite", _lib.F32, ctypes.c_void_p(addr + 2), 8, a, 1, None, None, None)
    expect_arg_error("dpwa_check_finite", _lib.F16, ctypes.c_void_p(addr + 1), 8, a, 1, None, None, None)
    expect_arg_error("dpwa_check_finite", 7, a, 8, a, 1, None, None, None)
    expect_arg_error("dpwa_check_finite", _lib.F64, a, 8, a, 1, None, None, None)
    expect_arg_error("dpwa_check_finite", _lib.MIXED, a, 8, a, 1, None, None, None)
    expect_arg_error("dpwa_check_finite", _lib.F32, a, 8, a, 1, None, a, None)                    # one event only
    good = layout((_lib.F32, 0, 4096), (_lib.F16, 4096, 8192))
    expect_arg_error("dpwa_check_finite_mixed", None, a, a, 1, None, None, None)
    expect_arg_error("dpwa_check_finite_mixed", ctypes.byref(good), None, a, 1, None, None, None)
    expect_arg_error("dpwa_check_finite_mixed", ctypes.byref(good), a, None, 1, None, None, None)
    expect_arg_error("dpwa_check_finite_mixed", ctypes.byref(good), a, a, 0, None, None, None)
    expect_arg_error("dpwa_check_finite_mixed", ctypes.byref(good), ctypes.c_void_p(addr + 4), a, 1, None, None, None)
    for bad in (layout(), layout((_lib.F32, 0, 100)), layout((_lib.F32, 4096, 4096)), layout((_lib.F64, 0, 4096))):
        expect_arg_error("dpwa_check_finite_mixed", ctypes.byref(bad), a, a, 1, None, None, None)
    expect_arg_error("dpwa_learner_set_finite_check", None, 1)
    expect_arg_error("dpwa_learner_finite_skips", None, None)
    lib = _lib.load()
    assert lib.dpwa_node_set_finite_check(None, 1) == _lib.ERR_STATE
    assert b"dpwa_node_set_finite_check" in lib.dpwa_last_error()


def test_connection_switch_without_a_device(tmp_path):
    """A connection is made without a device: the switch is off by default, counts 0 before its learner
    exists, and refuses relay-avg by name at construction and at set_pull (at bind: the GPU test)."""
    cfg = tmp_path / "f.yaml"
    write_cfg(cfg)
    conn = DpwaConnection("w1", str(cfg), seed=1, group=LocalGroup(), skip_nonfinite_peer=True)
    assert conn._skip_nonfinite is True and conn.nonfinite_skips == 0 and isinstance(conn.nonfinite_skips, int)
    with pytest.raises(ValueError) as err:
        conn.set_pull("relay-avg")
    assert "relay-avg" in str(err.value) and "skip_nonfinite_peer" in str(err.value)
    with pytest.raises(ValueError):
        conn.set_pull("relay-avg:32")
    conn.set_pull("kernel")                     # every other transport stays available
    conn.close()
    with pytest.raises(ValueError) as err:
        DpwaConnection("w1", str(cfg), seed=1, group=LocalGroup(), pull="relay-avg", skip_nonfinite_peer=True)
    assert "relay-avg" in str(err.value) and "skip_nonfinite_peer" in str(err.value)
    plain = DpwaConnection("w1", str(cfg), seed=1, group=LocalGroup())
    assert plain._skip_nonfinite is False and plain.nonfinite_skips == 0
    plain.close()


def test_the_adapter_hands_the_switch_to_its_connection(tmp_path):
    cfg = tmp_path / "a.yaml"
    write_cfg(cfg)
    for on in (False, True):
        net = torch.nn.Linear(5, 3)
        kwargs = {"skip_nonfinite_peer": True} if on else {}
        ad = DpwaPyTorchAdapter(net, "w1", str(cfg), seed=1, group=LocalGroup(), **kwargs)
        assert ad.connection._skip_nonfinite is on and ad.nonfinite_skips == 0
        ad.close()
    with pytest.raises(ValueError) as err:
        DpwaPyTorchAdapter(torch.nn.Linear(5, 3), "w1", str(cfg), seed=1, group=LocalGroup(), pull="relay-avg",
                           skip_nonfinite_peer=True)
    assert "skip_nonfinite_peer" in str(err.value)
    from dpwa.adapters.pytorch import DpwaPyTorchAdapter as Alias       # the reference's import paths
    from dpwa.dpwa import DpwaConnection as AliasConnection
    assert Alias is DpwaPyTorchAdapter and AliasConnection is DpwaConnection
