"""The consensus of a group without a device: the new C-ABI entries exist with the header's arities and
the ABI is still 11; every argument error that needs no device is DPWA_ERR_ARG naming the function; the
host model of tests/consensus_ref.py agrees with exact rational arithmetic on tiny inputs; and every
wrong implementation the model could be mistaken for (consensus_ref.MUTANTS) is told from it by an
input set the GPU test runs."""
import ctypes
import math
import re
from fractions import Fraction

import numpy as np
import pytest

from dpwa_amd import DpwaConnection, DpwaPyTorchAdapter, _lib
from tests import consensus_ref as ref
from tests import dist_ref as dr
from tests.test_distance_host import expect_arg_error, layout, write_cfg

NEW = ["dpwa_consensus_workspace", "dpwa_consensus", "dpwa_consensus_mixed", "dpwa_learner_consensus"]


def test_new_symbols_exist_with_the_headers_arities():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    decls = dict(re.findall(r"\bint\s+(dpwa_\w+)\s*\(([^)]*)\)\s*;", text))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in decls and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name]) == decls[name].count(",") + 1, name
    assert lib.dpwa_abi_version() == 11 and _lib.ABI_VERSION == 11
    assert re.search(r"#define DPWA_ABI_VERSION 11\b", open(_lib.HEADER_PATH).read())


def test_the_record_is_128_bytes_and_the_workspace_is_the_distances():
    assert ctypes.sizeof(_lib.ConsensusRecord) == 128
    assert [f[0] for f in _lib.ConsensusRecord._fields_][:7] == ["norm2", "spread2", "member_spread2", "n", "members",
                                                                 "reserved", "version"]
    assert _lib.ConsensusRecord.member_spread2.offset == 16 and _lib.ConsensusRecord.n.offset == 80
    assert _lib.ConsensusRecord.version.offset == 96
    text = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define DPWA_CONSENSUS_MAX (\d+)", text).group(1)) == _lib.CONSENSUS_MAX == 8
    b, d = ctypes.c_int64(), ctypes.c_int64()
    _lib.call("dpwa_consensus_workspace", ctypes.byref(b))
    _lib.call("dpwa_distance_workspace", ctypes.byref(d))
    assert b.value == d.value == ref.ROWS * _lib.DISTANCE_ACC_STRIDE == 128 << 10
    assert (_lib.CONSENSUS_MAX + 1) * 8 <= _lib.DISTANCE_ACC_STRIDE     # norm2 and eight spreads share a row


def test_bad_arguments_are_reported_without_a_device():
    """Non-NULL pointers here are host addresses no entry may touch: every call must fail first."""
    buf = (ctypes.c_char * (1 << 16))()
    addr = (ctypes.addressof(buf) + 15) & ~15
    a, out, ws, rec = (ctypes.c_void_p(addr + k * 8192) for k in range(4))

    def srcs(*ptrs):
        return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)
    two = srcs(a, ctypes.c_void_p(addr + 4096))
    expect_arg_error("dpwa_consensus_workspace", None)
    ok = [_lib.F32, two, 2, 8, out, ws, rec, None, None, None]

    def with_(base, i, v):
        args = list(base)
        args[i] = v
        return args
    bad = [(0, 7), (0, _lib.F64), (0, _lib.MIXED), (1, None), (2, 0), (2, 9), (2, -1), (3, -1),
           (4, ctypes.c_void_p(addr + 8192 + 4)),                      # out misaligned
           (5, None), (6, None),                                       # a workspace without a record and the reverse
           (5, ctypes.c_void_p(addr + 2 * 8192 + 8)),                  # workspace misaligned
           (6, ctypes.c_void_p(addr + 3 * 8192 + 4)),                  # record misaligned
           (1, srcs(a, None)), (1, srcs(a, ctypes.c_void_p(addr + 4100))),   # a NULL and a misaligned payload
           (4, a), (4, ctypes.c_void_p(addr + 16)),                    # out is a payload / overlaps one
           (8, a), (9, a)]                                             # one event without the other
    for i, v in bad:
        expect_arg_error("dpwa_consensus", *with_(ok, i, v))
    nothing = with_(with_(with_(ok, 4, None), 5, None), 6, None)
    expect_arg_error("dpwa_consensus", *nothing)                       # neither out nor a record
    # the segmented form: the same checks behind the layout's
    good = layout((_lib.F32, 0, 4096), (_lib.F16, 4096, 4096))
    big = (ctypes.c_char * (1 << 17))()
    base = (ctypes.addressof(big) + 15) & ~15
    m0, m1, mout = (ctypes.c_void_p(base + k * 8192) for k in range(3))
    okm = [ctypes.byref(good), srcs(m0, m1), 2, mout, ws, rec, None, None, None]
    expect_arg_error("dpwa_consensus_mixed", *with_(okm, 0, None))
    for lay in (layout(), layout((_lib.F32, 0, 100)), layout((_lib.F32, 4096, 4096)),
                layout((_lib.F32, 0, 4096), (_lib.F32, 4096, 4096)), layout((_lib.F64, 0, 4096))):
        expect_arg_error("dpwa_consensus_mixed", *with_(okm, 0, ctypes.byref(lay)))
    for i, v in ((1, None), (2, 0), (2, 9), (3, ctypes.c_void_p(base + 2 * 8192 + 4)), (4, None), (5, None),
                 (1, srcs(m0, None)), (1, srcs(m0, ctypes.c_void_p(base + 8192 + 8))), (3, m1),
                 (3, ctypes.c_void_p(base + 4096)), (7, m0)):
        expect_arg_error("dpwa_consensus_mixed", *with_(okm, i, v))
    # the learner entry: NULL learner, NULL ids
    ids = (ctypes.c_int32 * 2)(-1, 0)
    expect_arg_error("dpwa_learner_consensus", None, ids, 2, 1, out, rec, None)


def test_python_refusals_without_a_device(tmp_path):
    """A connection that has not published is a RuntimeError naming update_send; relay-avg and the wire
    transport are ValueErrors naming themselves, before any device is touched."""
    from dpwa_amd.bridge import WireConnection
    from dpwa_amd.consensus import RELAY_AVG, WIRE
    from dpwa_amd.group import LocalGroup
    cfg = tmp_path / "c.yaml"
    write_cfg(cfg)
    conn = DpwaConnection("w1", str(cfg), seed=1, group=LocalGroup())
    with pytest.raises(RuntimeError, match="update_send"):
        conn.consensus()
    conn.close()
    conn = DpwaConnection("w1", str(cfg), seed=1, group=LocalGroup(), pull="relay-avg:8")
    with pytest.raises(ValueError) as err:
        conn.consensus()
    assert str(err.value) == RELAY_AVG and "relay-avg" in RELAY_AVG
    conn.close()
    conn = WireConnection("w1", str(cfg), seed=1, serve=False)
    with pytest.raises(ValueError) as err:
        conn.consensus()
    assert str(err.value) == WIRE and "wire" in WIRE
    conn.close()
    assert hasattr(DpwaPyTorchAdapter, "consensus")


def exact(dtype, members):
    """The specification in rational arithmetic: the exact sum of the members (no rounding: the tiny
    inputs below are chosen so that every partial sum is a float64), times the float64 reciprocal,
    rounded once to float64, then to float32; the sums exact over those float64 means."""
    G = len(members)
    x = [[Fraction(float(v)) for v in dr.widen(dtype, b)] for b in members]
    r = Fraction(1.0 / G)
    means, norm, spread = [], Fraction(0), [Fraction(0)] * G
    for j in range(len(x[0])):
        s = sum(x[i][j] for i in range(G))
        assert Fraction(float(s)) == s, "choose inputs whose sums are float64 values"
        m = float(s * r)                     # correctly rounded: the one rounding of the multiplication
        means.append(m)
        norm += Fraction(m) ** 2
        for i in range(G):
            spread[i] += (x[i][j] - Fraction(m)) ** 2
    return np.array(means), norm, spread


@pytest.mark.parametrize("dtype", ref.DTYPES)
@pytest.mark.parametrize("G", ref.GROUPS)
def test_the_model_agrees_with_exact_rational_arithmetic(dtype, G):
    rng = np.random.default_rng(5 + G)
    n = 37
    members = [dr.to_bits(dtype, rng.integers(-64, 64, size=n) / 32.0) for _ in range(G)]
    members[0][:2] = [0, dr.SUBNORMAL[dtype]]       # (no -0: a rational has no sign of zero)
    for other in members[1:]:
        other[1] = 0                         # (a subnormal plus a normal value is no float64)
    bits, m, sums = ref.model(dtype, members)
    means, norm, spread = exact(dtype, members)
    assert np.array_equal(m, means)
    assert np.array_equal(bits, ref.round16(dtype, means.astype(np.float32)))
    # every term of the model carries at most three roundings and fsum one more
    for got, want in [(sums["norm2"], norm), (sums["spread2"], sum(spread))] + list(zip(sums["member"], spread)):
        assert abs(Fraction(got) - want) <= want * Fraction(4, 2 ** 53), (dtype, G, got, float(want))


def small_grid():
    """The part of the GPU test's grid a CPU test can afford: the small sizes, every set."""
    return [(d, G, n, only) for d, G, n, only in ref.grid() if n <= 513]


@pytest.mark.parametrize("mutant", [m for m in ref.MUTANTS if m != "rows-not-zeroed"])
def test_every_mutant_is_told_from_the_model_by_a_set_the_gpu_test_runs(mutant):
    found = []
    for dtype, G, n, only in small_grid():
        for name, members in ref.cases(dtype, G, n, only):
            if ref.differs(dtype, ref.model(dtype, members), ref.model(dtype, members, mutant), n, G):
                found.append((dtype, G, n, name))
    print(mutant, len(found), found[:6])
    assert found, "no input set of the GPU test tells %r from the model" % mutant
    if mutant == "direct-16-bit-rounding":
        assert "ties" in {f[3] for f in found}
        assert all(f[0] != "f32" for f in found)


def test_rows_not_zeroed_is_told_by_the_back_to_back_calls():
    """The GPU test calls twice on one workspace: a second call that still holds the first call's sums
    is outside the bound for every set whose sums are finite and not zero."""
    dtype, G, n = "f32", 3, 257
    members = dict(ref.cases(dtype, G, n))["normal"]
    first = ref.model(dtype, members)
    second = ref.model(dtype, members, "rows-not-zeroed", carry=first[2])
    assert ref.differs(dtype, first, second, n, G)


def test_bit_equality_of_the_means_is_sound_for_every_input_set():
    """Plain bit equality is what the GPU test asserts outside NaN positions: so no input set may hold
    a mean whose bits an honest implementation could legitimately choose differently -- that is only a
    NaN (its payload and sign are not specified).  Every other mean is finite or an infinity."""
    for dtype, G, n, only in small_grid():
        for name, members in ref.cases(dtype, G, n, only):
            bits, m, _ = ref.model(dtype, members)
            stored = dr.widen(dtype, bits)
            assert np.array_equal(np.isnan(stored), np.isnan(m)), (dtype, G, n, name)
            expect_nan = name in ("one-nan", "inf-and-minus-inf")
            assert bool(np.isnan(m).any()) == expect_nan, (dtype, G, n, name)


def test_the_ties_set_shows_the_two_roundings():
    for dtype in ("bf16", "f16"):
        for G in (3, 5, 8):
            cols = ref.tie_columns(dtype, G)
            print(dtype, G, cols.shape)
            assert cols.shape[1] >= 4, (dtype, G, cols.shape)
    for dtype, G in (("f32", 3), ("bf16", 1), ("bf16", 2), ("f16", 2)):      # (why: tie_columns' docstring)
        assert ref.tie_columns(dtype, G).shape[1] == 0


def test_the_bound_is_neither_vacuous_nor_too_tight():
    """numpy's pairwise float64 sum of the model's terms (another order than fsum's) is inside the bound;
    a float32 accumulation of them is not."""
    dtype, G, n = "f32", 5, ref.BIG
    members = dict(ref.cases(dtype, G, n, ("normal",)))["normal"]
    _, m, want = ref.model(dtype, members)
    x = [dr.widen(dtype, b) for b in members]
    got = {"norm2": float(np.sum(m * m)), "member": [float(np.sum((xi - m) * (xi - m))) for xi in x]}
    got["spread2"] = math.fsum(got["member"])
    assert ref.sums_problem(got, want, n, G) is None
    narrow = dict(got, norm2=float(np.sum((m * m).astype(np.float32), dtype=np.float32)))
    assert ref.sums_problem(narrow, want, n, G) is not None


def test_the_mixed_layout_is_the_issues():
    lay = ref.mixed_layout()
    assert [(d, length, count) for d, _, length, count in lay] == [("f32", 4096, 1024), ("bf16", 8192, 2049),
                                                                   ("f16", 4096, 5)]
    assert lay[0][3] * 4 == lay[0][2]                 # float32 fills its block exactly: no padding
