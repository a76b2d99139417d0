"""float16 parameters, host side (no GPU): the ABI constant and entry points, the Python dtype
tables, DLPack views and the flat layout for a ``.half()`` model, and the expected-value
restatement the GPU tests (tests/test_gpu_f16.py) rely on, pinned to torch-CPU eager over every
fp16 bit pattern."""
import re

import numpy as np
import pytest
import torch

from dpwa_amd import _lib, devview, learner
from dpwa_amd.flat import FlatParameters
from tests import f16_ref as ref


def test_dtype_code_in_header_and_binding():
    text = open(_lib.HEADER_PATH).read()
    consts = dict(re.findall(r"#define (DPWA_\w+) \(?(-?\d+)\)?", text))
    assert int(consts["DPWA_F16"]) == _lib.F16 == 3
    assert len({_lib.F32, _lib.BF16, _lib.F64, _lib.F16}) == 4


def test_abi_version_is_11():
    assert _lib.ABI_VERSION == 11
    assert _lib.load().dpwa_abi_version() == 11


@pytest.mark.parametrize("fn", ["dpwa_lerp_f16", "dpwa_lerp_f16_host"])
def test_lerp_f16_argument_errors_are_reported(fn):
    lib = _lib.load()
    args = (None, None, -1, None, None) if fn == "dpwa_lerp_f16" else (None, None, -1, 0.5, None)
    assert getattr(lib, fn)(*args) == _lib.ERR_ARG
    assert fn.encode() + b":" in lib.dpwa_last_error()


def test_float16_is_a_learner_dtype():
    assert torch.float16 in learner.DTYPES
    assert learner.DTYPES[torch.float16] == _lib.F16


def test_unsupported_dtype_message_names_float16():
    with pytest.raises(KeyError, match="float16"):
        learner.Learner(torch.device("cuda", 0), 16, torch.float64)


def test_device_tensor_float16_view():
    a = ref.PATTERNS[:1000].copy()
    t = devview.device_tensor(a.ctypes.data, 1000, torch.float16, 0, device_type=devview.KDL_CPU)
    assert t.dtype == torch.float16 and t.shape == (1000,) and t.data_ptr() == a.ctypes.data
    assert np.array_equal(ref.as_u16(t), a)
    t[3] = 1.0                                   # shares the memory
    assert a[3] == 0x3c00


def test_flat_parameters_of_a_half_model():
    net = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.Linear(17, 5)).half()
    want = [p.detach().clone() for p in net.parameters()]
    flat = FlatParameters(net.named_parameters())
    assert flat.dtype == torch.float16 and flat.buffer.dtype == torch.float16
    assert all(o % 128 == 0 for o in flat.offsets)            # 256-byte boundaries, 2-byte elements
    assert flat.numel % 128 == 0
    used = np.zeros(flat.numel, bool)
    for p, o, w in zip(flat.params, flat.offsets, want):
        assert p.dtype == torch.float16 and torch.equal(p.detach(), w)
        assert p.data_ptr() == flat.buffer.data_ptr() + 2 * o
        used[o:o + p.numel()] = True
    assert not ref.as_u16(flat.buffer)[~used].any()           # the gaps are zero


@pytest.mark.parametrize("f", ref.FACTORS)
def test_numpy_restatement_equals_torch_eager_on_every_bit_pattern(f):
    """Peers: all 65,536 fp16 bit patterns; parameters: a fixed permutation of them.  The last
    two factors overflow to inf and produce inf - inf."""
    want = ref.torch_lerp(ref.PERM, ref.PATTERNS, f)
    got = ref.numpy_lerp(ref.PERM, ref.PATTERNS, f)
    assert ref.same(got, want), ref.mismatches(got, want)
    if f in (1.5, -0.25):
        inf = (want & 0x7fff) == 0x7c00
        fin = ~ref.is_nan(ref.PERM) & ~ref.is_nan(ref.PATTERNS) & ((ref.PERM & 0x7c00) != 0x7c00) \
            & ((ref.PATTERNS & 0x7c00) != 0x7c00)
        notnan = ~ref.is_nan(ref.PERM) & ~ref.is_nan(ref.PATTERNS)
        assert (inf & fin).any()                                # overflow of finite inputs
        assert (ref.is_nan(want) & notnan).any()                # inf - inf


def test_restatement_on_the_hard_sample():
    """The GPU tests' sample (signed zeros, smallest subnormals, largest finite values in every
    position class): the restatement and torch eager agree there too, and signed zeros occur."""
    p, q = ref.sample(4099, 3)
    for f in ref.FACTORS:
        want = ref.torch_lerp(p, q, f)
        assert ref.same(ref.numpy_lerp(p, q, f), want), f
    assert (ref.torch_lerp(p, q, 0.5) == ref.NEG_ZERO).any()
    assert ((p == ref.NEG_ZERO) & (q == ref.NEG_ZERO)).any()


def test_same_rule():
    a = np.array([0x3c00, 0x7e00, 0x8000], np.uint16)
    assert ref.same(a, np.array([0x3c00, 0x7c01, 0x8000], np.uint16))       # NaN payloads may differ
    assert not ref.same(a, np.array([0x3c00, 0x7e00, 0x0000], np.uint16))   # -0 is not +0
    assert not ref.same(a, np.array([0x3c00, 0x7c00, 0x8000], np.uint16))   # inf is not NaN
