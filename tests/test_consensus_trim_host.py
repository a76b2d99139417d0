"""The trimmed consensus without a device: the new C-ABI entries exist with the header's arities, argument
errors are DPWA_ERR_ARG naming the function, and ``trim``'s ValueErrors come before a device is touched; and
the host model of tests/consensus_trim_ref.py: every wrong kernel it could be mistaken for (its MUTANTS) is
told from it by an input set the GPU test runs, for every dtype, member count and trim, and the input sets
hold what they say."""
import ctypes
import math
import re

import numpy as np
import pytest

from dpwa_amd import DpwaConnection, _lib
from dpwa_amd.consensus import effective_trim
from dpwa_amd.group import LocalGroup
from tests import consensus_ref as ref
from tests import consensus_trim_ref as tr
from tests import dist_ref as dr
from tests.test_distance_host import expect_arg_error, layout, write_cfg


def test_new_symbols_exist_with_the_headers_arities():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    decls = dict(re.findall(r"\bint\s+(dpwa_\w+)\s*\(([^)]*)\)\s*;", text))
    for name in ("dpwa_consensus_trimmed", "dpwa_consensus_trimmed_mixed", "dpwa_learner_consensus_trimmed"):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name]) == decls[name].count(",") + 1, name
    assert lib.dpwa_abi_version() == 11


def test_bad_arguments_are_reported_without_a_device():
    """Non-NULL pointers here are host addresses no entry may touch: every call must fail first."""
    buf = (ctypes.c_char * (1 << 16))()
    addr = (ctypes.addressof(buf) + 15) & ~15
    out, ws, rec = (ctypes.c_void_p(addr + (5 + k) * 4096) for k in range(3))
    srcs = (ctypes.c_void_p * 5)(*[addr + k * 4096 for k in range(5)])
    ok = [_lib.F32, srcs, 5, 2, 8, out, ws, rec, None, None, None]
    okm = [ctypes.byref(layout((_lib.F16, 0, 4096))), srcs, 5, 2, out, ws, rec, None, None, None]
    # count 2 and 9, trim 0 / negative / 2 * trim = count and beyond, then what dpwa_consensus refuses too
    bad = [(2, 2), (2, 9), (3, 0), (3, -1), (3, 3), (2, 4), (0, 7), (0, _lib.MIXED), (1, None), (4, -1),
           (5, ctypes.c_void_p(addr + 5 * 4096 + 4)), (5, ctypes.c_void_p(addr + 16)), (6, None), (7, None), (9, out)]
    badm = [(0, None), (2, 2), (3, 0), (3, 3), (4, ctypes.c_void_p(addr + 5 * 4096 + 8)), (5, None)]
    for name, base, cases in (("dpwa_consensus_trimmed", ok, bad), ("dpwa_consensus_trimmed_mixed", okm, badm)):
        for i, v in cases:
            expect_arg_error(name, *(base[:i] + [v] + base[i + 1:]))
    ids = (ctypes.c_int32 * 3)(-1, 0, 1)
    expect_arg_error("dpwa_learner_consensus_trimmed", None, ids, 3, 1, 1, out, rec, None)


def test_pythons_trim_errors_are_raised_before_anything_is_launched(tmp_path):
    assert [effective_trim(t, 5) for t in (0, 1, 2, "median")] == [0, 1, 2, 2]
    assert [effective_trim("median", G) for G in range(1, 9)] == [0, 0, 1, 1, 2, 2, 3, 3]
    for t, G, most in ((2, 4, 1), (1, 2, 0), (4, 8, 3)):
        with pytest.raises(ValueError, match=r"G = %d members: the largest trim is %d" % (G, most)):
            effective_trim(t, G)
    cfg = tmp_path / "c.yaml"
    write_cfg(cfg)
    conn = DpwaConnection("w1", str(cfg), seed=1, group=LocalGroup())
    for wrong in (-1, "mean", 1.0, True, None):           # before the connection's state is looked at
        with pytest.raises(ValueError, match="'median'"):
            conn.consensus(trim=wrong)
    with pytest.raises(RuntimeError, match="update_send"):
        conn.consensus(trim="median")
    conn.close()


# ---------------------------------------------------------------- the model, its mutants and the input sets
# The fewest wrong kernels any (dtype, G, t) is checked against.  tr.exempt leaves float32 with one or two kept
# values ((3, 1), (4, 1), (5, 2), (6, 2), (7, 3), (8, 3)) five: trim-one-less, value-order, sum-from-plus-zero,
# spread-over-kept, last-member-unsorted -- descending-sum adds one or two values in either order to the same
# float64, the reciprocal of 1 or 2 is exact, no further trim leaves a value and the rest is 16-bit only.
FLOOR = 5


def test_the_pairs_are_the_twelve_the_entries_accept():
    assert tr.PAIRS == ((3, 1), (4, 1), (5, 1), (5, 2), (6, 1), (6, 2), (7, 1), (7, 2), (7, 3), (8, 1), (8, 2), (8, 3))
    live = {(d, G, t): [m for m in tr.MUTANTS if tr.exempt(m, d, G, t) is None] for d in ref.DTYPES for G, t in tr.PAIRS}
    assert min(len(v) for v in live.values()) == FLOOR == len(live["f32", 3, 1])
    assert len(live["bf16", 7, 1]) == len(tr.MUTANTS)


@pytest.mark.parametrize("G,t", tr.PAIRS)
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_every_live_mutant_is_told_from_the_model_by_a_set_the_gpu_test_runs(dtype, G, t):
    live = [m for m in tr.MUTANTS if tr.exempt(m, dtype, G, t) is None]
    assert len(live) >= FLOOR
    caught = {}
    for n in ref.SMALL[dtype]:
        for name, members in tr.cases(dtype, G, t, n):
            want = tr.model(dtype, members, t)
            for mutant in live:
                if mutant not in caught and tr.differs(dtype, want, tr.model(dtype, members, t, mutant), n, G):
                    caught[mutant] = (n, name)
    for mutant in live:
        print(dtype, G, t, mutant, caught.get(mutant))
        assert mutant in caught, "no input set at a small size tells %r from the model for %s" % (mutant, (dtype, G, t))


@pytest.mark.parametrize("G,t", tr.PAIRS)
def test_an_exempt_mutant_is_the_model_on_every_small_set(G, t):
    """tr.exempt's reasons, tried: an exempt mutant gives the model's bits and sums on every set."""
    for dtype in ref.DTYPES:
        for mutant in tr.MUTANTS:
            if tr.exempt(mutant, dtype, G, t) is None or mutant == "trim-one-more":
                continue
            for name, members in tr.cases(dtype, G, t, ref.SMALL[dtype][-1]):
                assert not tr.differs(dtype, tr.model(dtype, members, t), tr.model(dtype, members, t, mutant),
                                      ref.SMALL[dtype][-1], G), (dtype, mutant, name)


@pytest.mark.parametrize("G,t", tr.PAIRS)
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_finite_sets_give_numbers_and_the_hard_set_a_nan_norm(dtype, G, t):
    for n in ref.SMALL[dtype]:
        sets = dict(tr.cases(dtype, G, t, n))
        assert math.isnan(tr.model(dtype, sets["hard"], t)[1]["norm2"]), n
        # (float16's `finite` holds a member scaled past 65504: its sums are numbers or +inf, never NaN)
        assert not any(math.isnan(v) for v in tr.model(dtype, sets["finite"], t)[1]["member"]), n
        numbers = ("normal", "orders", "negative-zeros", "cancellation", "ties", "reciprocal") + tr.POSITIONS
        for name in (("finite",) if dtype != "f16" else ()) + numbers:
            if name in sets:
                sums = tr.model(dtype, sets[name], t)[1]
                assert all(math.isfinite(v) for v in [sums["norm2"], sums["spread2"]] + sums["member"]), (n, name)


def test_the_sum_over_all_members_is_dist_refs():
    members = dict(tr.cases("bf16", 5, 1, 513))
    for name in ("hard", "finite", "normal", "specials"):
        x = [dr.widen("bf16", m) for m in members[name]]
        with np.errstate(all="ignore"):
            terms = [(v - x[0]) * (v - x[0]) for v in x]
        got, want = tr.fsum_all(terms), dr.fsum(np.concatenate(terms))
        assert got == want or (math.isnan(got) and math.isnan(want)), name


def test_the_positional_differences_change_a_kept_value():
    for dtype in ref.DTYPES:
        for G, t in tr.PAIRS:
            n = ref.SMALL[dtype][-1]
            sets = dict(tr.cases(dtype, G, t, n))
            same = tr.model(dtype, [sets[tr.POSITIONS[0]][0]] * G, t)[0]
            for name, at in ((tr.POSITIONS[0], n - 1), (tr.POSITIONS[1], dr.SPAN[dtype] - 1)):
                bits = tr.model(dtype, sets[name], t)[0]
                assert list(np.flatnonzero(bits != same)) == [at], (dtype, G, t, name)


@pytest.mark.parametrize("G", range(3, 9))
def test_orders_holds_every_ordering_in_each_half_of_a_dword(G):
    n = tr.orders_size(G)
    assert tr.order_ranks(G).shape == (G, n)
    for dtype in ("bf16", "f32"):
        members = np.stack(dict(tr.cases(dtype, G, 1, n, ("orders",)))["orders"])
        strict = np.all(np.diff(np.sort(members, axis=0), axis=0) != 0, axis=0)
        one_tie = np.sum(np.diff(np.sort(members, axis=0), axis=0) == 0, axis=0) == 1
        for half in (0, 1):
            at = np.arange(half, n, 2)
            top = 8 * dr.SIZE[dtype] - 1
            half_bits = members[:, at].astype(np.int64)
            ranks = np.argsort(half_bits ^ np.where(half_bits >> top, (2 << top) - 1, 1 << top), axis=0, kind="stable")
            seen = {bytes(c) for c in ranks[:, strict[at]].T.astype(np.int8)}
            assert len(seen) == math.factorial(G), (dtype, half, len(seen))
            assert int(one_tie[at].sum()) == G * (G - 1) // 2 * math.factorial(G - 1), (dtype, half)
    # a smaller n takes the first columns
    first = dict(tr.cases("f16", G, 1, 5, ("orders",)))["orders"]
    assert [len(m) for m in first] == [5] * G and len({int(m[0]) for m in first}) == G


def test_specials_and_the_patterns_are_what_they_say():
    for dtype in ref.DTYPES:
        marks = tr.landmarks(dtype)
        keys = marks.astype(np.int64) ^ np.where(marks >> (8 * dr.SIZE[dtype] - 1), (1 << 8 * dr.SIZE[dtype]) - 1,
                                                 1 << (8 * dr.SIZE[dtype] - 1))
        assert len(marks) == 17 and list(keys) == sorted(set(keys))        # distinct, ascending in the key order
        x = dr.widen(dtype, marks)
        assert np.isnan(x[[0, 15, 16]]).all() and np.isinf(x[[1, 14]]).all() and list(x[[3, 12]]) == [-1.0, 1.0]
        assert tr.special_columns(dtype, 3).shape == (3, 17 ** 3)
        assert len({bytes(c) for c in tr.special_columns(dtype, 3).T}) == 17 ** 3
        assert tr.special_columns(dtype, 6).shape == (6, tr.SPECIAL_DRAW)
    assert tr.PATTERNS not in dict(tr.cases("f32", 5, 1, 1 << 16)) and tr.PATTERNS not in dict(tr.cases("bf16", 5, 1, 513))
    for n in (1 << 16, ref.BIG):
        members = dict(tr.cases("f16", 8, 2, n, (tr.PATTERNS,)))[tr.PATTERNS]
        assert np.array_equal(members[0][:1 << 16], np.arange(1 << 16))
        for m in members:                      # every pattern in every member, in both halves of a dword
            assert len(np.unique(m[:1 << 16])) == 1 << 16
            assert len(np.unique(np.concatenate([m[0:n:2], [0]]))) >= 1 << 15
        pairs = {(int(a), int(b)) for a, b in zip(members[1][0:64:2], members[1][1:64:2])}
        assert len({(b - a) % 65536 for a, b in pairs}) == 1 and all((b - a) % 2 for a, b in pairs)


def test_the_grid_is_the_issues():
    grid = tr.grid()
    assert {(d, G, t) for d, G, t, _, _ in grid} == {(d, G, t) for d in ref.DTYPES for G, t in tr.PAIRS}
    for d in ref.DTYPES:
        for G, t in tr.PAIRS:
            mine = [(n, only) for dd, GG, tt, n, only in grid if (dd, GG, tt) == (d, G, t)]
            assert [n for n, only in mine if only is None] == ref.SMALL[d] + [ref.BIG]
            many = [name for n, only in mine if n == ref.many(d) for name in only]
            assert set(tr.MANY_SETS) <= set(many) and (len(many) > len(tr.MANY_SETS)) == ((G, t) == (5, 2))
