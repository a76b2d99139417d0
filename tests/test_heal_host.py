"""Healing non-finite elements inside the averaging kernel (``heal_nonfinite``), without a device:
tests/heal_ref.py's rule on a table of its own; each of the four wrong selects told from the right one by
an input that tests/test_gpu_heal.py runs; the argument checks that need no device; the Python refusals."""
import ctypes

import numpy as np
import pytest

from dpwa_amd import DpwaConnection, DpwaPyTorchAdapter, _lib, bridge, dpwa
from dpwa_amd.group import LocalGroup
from tests import heal_ref as ref
from tests.test_distance_host import expect_arg_error, layout, write_cfg


@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_the_four_rows_of_the_table(dtype):
    """One element per row (and a subnormal, the largest finite value and a healed -0.0), factor 0.25."""
    one = {"f32": 0x3f800000, "bf16": 0x3f80, "f16": 0x3c00}[dtype]
    nan, inf, neg0 = ref.BAD[dtype]["snan"], ref.BAD[dtype]["-inf"], ref.SIGN[dtype]
    p = np.array([one, one, nan, inf, ref.LARGEST[dtype], nan, 1], dtype=ref.NUMPY[dtype])
    q = np.array([one, nan, one, nan, inf, neg0, ref.LARGEST[dtype]], dtype=ref.NUMPY[dtype])
    r, healed, refused = ref.heal(dtype, p, q, 0.25)
    assert list(r[:6]) == [one, one, one, inf, ref.LARGEST[dtype], neg0] and (healed, refused) == (2, 3)
    assert r[6] == ref.forms_ref.lerp(dtype, p[6:], q[6:], 0.25)[0] and ref.forms_ref.is_finite(dtype, r[6])


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_wrong_select_is_told_by_a_gpu_input(mutant):
    told = []
    for dtype in ref.DTYPES:
        for n in ref.sizes(dtype):
            for variant in ref.VARIANTS:
                p, q = ref.inputs(dtype, n, variant)
                want, got = ref.heal(dtype, p, q, 0.7), ref.heal(dtype, p, q, 0.7, mutant)
                if want[0].tobytes() != got[0].tobytes() or want[1:] != got[1:]:
                    told.append((dtype, n, variant))
    print(mutant, len(told), told[:4])
    assert told and not any(v == "clean" for _, _, v in told)
    if mutant == "per-dword":               # an fp32 dword is one element
        assert {d for d, _, _ in told} == {"bf16", "f16"}
    else:
        assert {d for d, _, _ in told} == set(ref.DTYPES)


def test_bad_arguments_are_reported_without_a_device():
    """Non-NULL pointers here are host addresses no entry may touch: every call must fail first."""
    buf = (ctypes.c_char * 4096)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    a, off4, off8 = ctypes.c_void_p(addr), ctypes.c_void_p(addr + 4), ctypes.c_void_p(addr + 8)
    cfg = ctypes.byref(_lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0))
    ok = [_lib.F32, a, a, 8, cfg, a, 1.0, a, a, a, None, None, None]

    def but(i, v):
        return ok[:i] + [v] + ok[i + 1:]

    for args in (but(1, None), but(2, None), but(3, -1), but(4, None), but(5, None), but(7, None), but(9, None),
                 but(0, 7), but(0, _lib.MIXED), but(9, off4), but(11, a),
                 but(1, off4), but(2, off8), but(8, off4)):            # there is no unaligned form
        expect_arg_error("dpwa_average_guarded", *args)
    assert b"16-byte aligned" in _lib.load().dpwa_last_error()
    good = ctypes.byref(layout((_lib.F32, 0, 4096), (_lib.F16, 4096, 4096)))
    okm = [good, a, a, cfg, a, 1.0, a, None, a, None, None, None]
    for i, v in ((0, None), (1, None), (2, None), (8, None), (8, off4), (1, off8), (7, off4),
                 (0, ctypes.byref(layout((_lib.F32, 0, 100))))):
        expect_arg_error("dpwa_average_guarded_mixed", *(okm[:i] + [v] + okm[i + 1:]))
    expect_arg_error("dpwa_learner_set_heal", None, 1)
    expect_arg_error("dpwa_learner_heal_record", None, None)
    lib = _lib.load()
    assert lib.dpwa_node_set_heal(None, 1) == _lib.ERR_STATE and b"dpwa_node_set_heal" in lib.dpwa_last_error()
    assert lib.dpwa_abi_version() == 11 and ctypes.sizeof(_lib.HealRecord) == 32


def test_the_python_switch_without_a_device(tmp_path):
    """Off by default and zeros before a learner exists; relay-avg refused by name at construction and at
    set_pull (at bind: the GPU test); the adapter hands it on only when set; the wire transport refuses it."""
    cfg = tmp_path / "h.yaml"
    write_cfg(cfg)
    conn = DpwaConnection("w1", str(cfg), seed=1, group=LocalGroup(), heal_nonfinite=True)
    assert conn.nonfinite_elements == (0, 0, 0, 0.0) and conn.nonfinite_elements.healed == 0
    for pull in ("relay-avg", "relay-avg:32"):
        with pytest.raises(ValueError) as err:
            conn.set_pull(pull)
        assert str(err.value) == dpwa.HEAL_RELAY_AVG and "heal_nonfinite" in dpwa.HEAL_RELAY_AVG
    conn.set_pull("kernel")
    conn.close()
    with pytest.raises(ValueError) as err:
        DpwaConnection("w1", str(cfg), seed=1, group=LocalGroup(), pull="relay-avg", heal_nonfinite=True)
    assert str(err.value) == dpwa.HEAL_RELAY_AVG
    import torch
    for on in (False, True):
        ad = DpwaPyTorchAdapter(torch.nn.Linear(5, 3), "w1", str(cfg), seed=1, group=LocalGroup(),
                                **({"heal_nonfinite": True} if on else {}))
        assert ad.connection._heal is on and ad.nonfinite_elements == (0, 0, 0, 0.0)
        ad.close()
    with pytest.raises(ValueError) as err:
        DpwaPyTorchAdapter(torch.nn.Linear(5, 3), "w1", str(cfg), transport="wire", heal_nonfinite=True)
    assert str(err.value) == bridge.HEAL_WIRE and "heal_nonfinite" in bridge.HEAL_WIRE
