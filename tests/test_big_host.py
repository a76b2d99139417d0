"""tests/big_ref.py without a GPU: the conditions its operands rest on, the model of the right kernel
against expectations formed another way, and every slip of big_ref.MUTANTS shown to fail a check that
tests/test_gpu_big.py applies to the kernels the slip could live in."""
import numpy as np
import pytest

from tests import big_ref as ref
from tests import finite_ref
from tests import forms_ref as fref
from tests.mixed_ref import NUMPY, SIZE

PAYLOADS = {"bf16": lambda: ref.single("bf16"), "f16": lambda: ref.single("f16"), "f32": lambda: ref.single("f32"),
            "mixed": ref.mixed, "tabled": ref.tabled}


@pytest.mark.parametrize("dtype", fref.DTYPES)
def test_the_five_constant_values_differ(dtype):
    """A, B, lerp(A,B), lerp(lerp(A,B),B) and the role-swapped lerp(B,A): an element left alone, copied
    from the peer, averaged, averaged twice or averaged the wrong way round shows."""
    assert ref.FACTOR != 0.5
    for family in ("hard", "exact"):
        a, b = ref.FAMILIES[family][0][dtype]
        once = fref.lerp(dtype, [a], [b], ref.FACTOR)[0]
        twice = fref.lerp(dtype, [once], [b], ref.FACTOR)[0]
        swapped = fref.lerp(dtype, [b], [a], ref.FACTOR)[0]
        values = [int(a), int(b), int(once), int(twice), int(swapped)]
        assert len(set(values)) == 5, (family, [hex(v) for v in values])
        fill = int(np.full(SIZE[dtype], ref.FILL, dtype=np.uint8).view(NUMPY[dtype])[0])
        assert fill not in values                          # an unreached destination differs too
        assert all(fref.is_finite(dtype, np.array(values, dtype=NUMPY[dtype])))


def test_the_shapes_cross_both_lines():
    for d in fref.DTYPES:
        n, s = ref.N[d], SIZE[d]
        assert n * s > ref.L32 and (n * s) % 16 == s, "one element behind the last whole item"
        assert (n - 1001) * s == ref.L32
    assert ref.N["bf16"] > ref.L31 and ref.N["f32"] < ref.L31
    segs = ref.MIXED_SEGS
    assert [b - a for _, a, b in segs] == [ref.L32 + 4096, 8192, 4096] and all(a > ref.L32 for _, a, _ in segs[1:])
    assert all(a % 4096 == 0 and b % 4096 == 0 for _, a, b in segs)
    for (a, b), (c, _) in zip(ref.TENSORS, ref.TENSORS[1:] + ((ref.N["bf16"] * 2, 0),)):
        assert a % 256 == 0 and a < b <= c and (b - a) % 2 == 0


@pytest.mark.parametrize("name", sorted(PAYLOADS))
def test_windows_and_constant_region_cover_the_payload_once(name):
    pl = PAYLOADS[name]()
    parts = sorted(pl.wins + pl.gaps())
    assert parts[0][0] == 0 and parts[-1][1] == pl.nbytes
    assert all(a[1] == b[0] for a, b in zip(parts, parts[1:])) and all(a < b for a, b in parts)
    must = [0, ref.L31 - 1, ref.L31, ref.L32 - 1, ref.L32, pl.nbytes - 1] + [x + o for x in pl.borders for o in (-1, 0) if 0 <= x + o < pl.nbytes]
    for at in must:
        assert any(a <= at < b for a, b in pl.wins), at
    for a, b in pl.wins:
        assert all(x % SIZE[d] == 0 and y % SIZE[d] == 0 for d, x, y in pl.split(a, b))


@pytest.mark.parametrize("family", sorted(ref.FAMILIES))
@pytest.mark.parametrize("name", sorted(PAYLOADS))
def test_every_window_differs_from_every_other_and_from_the_constants(name, family):
    pl = PAYLOADS[name]()
    for op in ref.operands(pl, family)[0 if family != "finite" else 1:]:
        for i, (lo, hi) in enumerate(pl.wins):
            for d, a, b in pl.split(lo, hi):
                bits = ref.as_bits(d, op.data[i][a - lo:b - lo])
                assert (bits != op.const[d]).mean() > 0.5, (name, family, i)
            for j in range(i):
                m = min(len(op.data[i]), len(op.data[j]))
                assert (op.data[i][:m] != op.data[j][:m]).mean() > 0.25, (name, family, i, j)
    P, Q = ref.operands(pl, family)
    if family != "finite":
        assert all((p != q).any() for p, q in zip(P.data, Q.data))


@pytest.mark.parametrize("name", sorted(PAYLOADS))
def test_the_exact_family_is_exact(name):
    """Every value is a half-integer of magnitude at most 31.5, so every term is a multiple of 2^-2 below
    2^12; the elements number at most 2^32 / 2, so every total is a multiple of 2^-2 below 2^46 < 2^51:
    float64 holds every partial sum of any order exactly."""
    pl = PAYLOADS[name]()
    elements = 0
    for op in ref.operands(pl, "exact"):
        for d in pl.dtypes:
            assert ref.decode(d, [op.const[d]])[0] in (1.0, 1.5)
        for i, (lo, hi) in enumerate(pl.wins):
            for d, a, b in pl.split(lo, hi):
                x = ref.decode(d, ref.as_bits(d, op.data[i][a - lo:b - lo]))
                assert (np.abs(x) <= 31.5).all() and (x * 2 == np.round(x * 2)).all()
    for d, a, b in pl.segs:
        elements += (b - a) // SIZE[d]
    assert (63.0 ** 2) < 2 ** 12 and elements * 2 ** 12 < 2 ** 46


# ---------------------------------------------------------------- the right kernel, another way
def _direct_windows(pl, P, Q):
    out = []
    for i, (lo, hi) in enumerate(pl.wins):
        w = np.empty(hi - lo, dtype=np.uint8)
        for d, a, b in pl.split(lo, hi):
            w[a - lo:b - lo] = fref.lerp(d, ref.as_bits(d, P.data[i][a - lo:b - lo]), ref.as_bits(d, Q.data[i][a - lo:b - lo]),
                                         ref.FACTOR).view(np.uint8)
        out.append((lo, hi, w))
    return out


def _direct_sums(pl, P, Q, lo=0, hi=None):
    """The sums over [lo, hi): the constant region in closed form, the windows element by element."""
    hi = pl.nbytes if hi is None else hi
    d2 = n2 = 0.0
    for d, a, b in pl.split(lo, hi):
        inside = 0
        for i, (x, y) in enumerate(pl.wins):
            x, y = max(x, a), min(y, b)
            if x < y:
                w0 = pl.wins[i][0]
                p = ref.decode(d, ref.as_bits(d, P.data[i][x - w0:y - w0]))
                q = ref.decode(d, ref.as_bits(d, Q.data[i][x - w0:y - w0]))
                d2 += float(((q - p) ** 2).sum())
                n2 += float((p ** 2).sum())
                inside += y - x
        cp, cq = ref.decode(d, [P.const[d]])[0], ref.decode(d, [Q.const[d]])[0]
        count = (b - a - inside) // SIZE[d]
        d2 += count * (cq - cp) ** 2
        n2 += count * cp ** 2
    return d2, n2


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: "-".join(c[0]))
def test_the_right_kernel_passes_its_checks(case):
    name, make, family, op, fam = case
    pl = make()
    P, Q = ref.operands(pl, fam)
    got = ref.model(pl, family, op, fam)
    assert got != ref.OUTSIDE
    if op in ("lerp", "tracked"):
        want = _direct_windows(pl, P, Q)
        for dest in ("param", "snap"):
            assert got[dest].stray == 0
            for (_, _, g), (_, _, w) in zip(got[dest].windows, want):
                assert np.array_equal(g, w)
    if op == "tracked":
        assert got["record"].sums == _direct_sums(pl, P, Q)
    if op == "sums":
        assert got.sums == _direct_sums(pl, P, Q)
    if op == "table":
        assert got.sums == [_direct_sums(pl, P, Q, a, b) for a, b in ref.TENSORS]
        assert all(s[0] > 0 and s[1] > 0 for s in got.sums)
    if op == "copy":
        assert got.stray == 0 and all(np.array_equal(g, d) for (_, _, g), d in zip(got.windows, P.data))
    if op == "finite":
        plants = ref.finite_plants(pl, Q)
        assert got.veto == (False,) + (True,) * (len(plants) - 1)
        assert len(plants) >= 1 + 4 * 6


# ---------------------------------------------------------------- every slip fails a check
def _caught():
    """{mutant: [(case, failed checks)]} over every case the slip can live in."""
    out = {m: [] for m in ref.MUTANTS}
    for name, make, family, op, fam in ref.CASES:
        pl = make()
        P, Q = ref.operands(pl, fam)
        want = ref.model(pl, family, op, fam, None, P, Q)
        for m in ref.MUTANTS:
            got = ref.model(pl, family, op, fam, m, P, Q)
            if got is not None:
                out[m].append((name, ref.failures(pl, got, want, exact_bytes=op == "copy")))
    return out


def test_every_mutant_fails_a_check_wherever_it_can_live():
    caught = _caught()
    for m, where in caught.items():
        if m in ref.GUARD_MUTANTS or m in ref.RELAY_MUTANTS:     # the guards' and the relay's own tests below
            continue
        assert where, "%s lives in no case of the GPU module" % m
        for name, failed in where:
            assert failed, "%s in %s passes every check" % (m, name)
    # at the smallest sizes that cross 2^32 bytes everything beyond the line lies in a window: the slips
    # of the vector body show in the windows' bits; the count of the constant region sees the slips
    # that reach further (a segment rounded as another type, 4 KiB of a segmented payload never run)
    for m in ("offset-mod-2^32", "grid-truncated"):
        failed = dict(caught[m])[("lerp", "bf16")]
        assert {"param:windows", "snap:windows"} <= set(failed), (m, failed)
    for m in ("grid-truncated", "segment-begins-32-bit"):
        assert {"param:stray", "snap:stray"} <= set(dict(caught[m])[("average-mixed",)]), m
    assert dict(caught["index-mod-2^31"])[("average-unaligned", "bf16")]
    assert dict(caught["tail-from-32-bit-n"])[("lerp", "f32")] and dict(caught["tail-from-32-bit-n"])[("lerp", "bf16")]
    assert dict(caught["segment-begins-32-bit"]).keys() == {("average-mixed",), ("distance-mixed",), ("finite-mixed",)}
    assert dict(caught["table-begins-32-bit"]) == {("param-distance",): ["sums"]}
    assert dict(caught["param-row-payload-span"]) == {("param-distance",): ["outside"]}
    assert ref.table_rows(ref.TENSORS) == []
    assert all(failed == ["veto"] for _, failed in caught["nonfinite-below-2^32-only"])
    assert dict(caught["offset-sign-extended"])[("distance", "f32")] == ["outside"]


def test_the_sums_tell_one_missing_span_from_none():
    """The exact bar sees a single element counted twice or not at all, where a relative bound at
    n = 2^31 would not see a whole span."""
    pl = ref.single("bf16")
    P, Q = ref.operands(pl, "exact")
    right = ref.sums(pl, P, Q, ref.right_cover(pl))
    at = 12345 * 1024
    for k in (0, 2):
        cov = ref.cover(pl, [at, at + 2], lambda y: ((k if y == at else 1), "bf16"))
        assert ref.sums(pl, P, Q, cov) != right


def test_the_equivalent_slip_is_named_not_counted():
    assert "param-row-before-begin" in ref.EQUIVALENT and not set(ref.EQUIVALENT) & set(ref.MUTANTS)


def test_finite_positions():
    pl = ref.single("bf16")
    pos = ref.finite_positions(pl)
    assert pos == {"last-below-2^31": ref.L31 - 2, "first-at-2^31": ref.L31, "last-below-2^32": ref.L32 - 2,
                   "first-at-2^32": ref.L32, "first-of-last-whole-item": ref.L32 + 2000 - 16, "last-element": ref.L32 + 2000}
    mx = ref.finite_positions(ref.mixed())
    assert mx["first-of-f32-segment"] == ref.L32 + 4096 and mx["first-of-f16-segment"] == ref.L32 + 12288
    Q = ref.operands(pl, "finite")[1]
    assert not finite_ref.vetoes("bf16", np.array([Q.const["bf16"]]))


# ---------------------------------------------------------------- the guards
def test_guard_model_agrees_with_moves_ref_at_small_sizes():
    """big_ref.guard_model and window_model against tests/moves_ref.py on whole host arrays."""
    from tests import moves_ref
    rng = np.random.default_rng(5)
    for n16, tail in ((1, 0), (17, 4), (4097, 0), (8191, 4), (16 * 4095 + 1, 4)):
        nbytes = n16 * 16 + tail
        snap = rng.integers(0, 256, nbytes, dtype=np.uint8)
        for gen in (2, 3, 6, 4099):
            sampled = moves_ref.sampled(n16, gen)
            words = set(rng.integers(0, n16, 6).tolist()) | set(sampled[rng.integers(0, len(sampled), 2)].tolist())
            words |= {n16} if tail and gen % 2 else set()
            flat = moves_ref.written(snap, sorted(words), gen)
            at = moves_ref.write_offsets(sorted(words), nbytes, gen)
            want, hit = moves_ref.guard_expected(snap, flat, gen)
            taken, got_hit = ref.guard_model(nbytes, gen, at)
            assert (np.flatnonzero(want != snap).tolist(), hit) == (taken, got_hit), (n16, tail, gen)
            assert ref.window_model(nbytes, gen, at) == moves_ref.window_expected(snap, flat, gen)


def test_the_guard_cases_tell_the_32_bit_slips():
    from tests import moves_ref
    nbytes = ref.single("bf16").nbytes
    n16 = nbytes // 16
    assert n16 > (1 << 28) and 16 * (n16 - 1) > (1 << 28) * 16 == ref.L32
    gen = 2
    words = ref.guard_case(nbytes, gen)
    at = moves_ref.write_offsets(words, nbytes, gen)
    taken, hit = ref.guard_model(nbytes, gen, at)
    # both chunks and the tail are taken whole, the words just outside them are not
    assert hit and 0 < len(taken) < len(at) and max(taken) >= n16 * 16 and any(ref.L32 <= o < n16 * 16 for o in taken)
    left = sorted(set(at.tolist()) - set(taken))
    assert len(left) == 3, left            # (the word behind the second chunk is the last word, a chunk of its own)
    few = moves_ref.write_offsets(ref.guard_case(nbytes, gen, two_chunks_only=True), nbytes, gen)
    dirty = {k for k, (w, _) in enumerate(ref.guard_sampled(n16, gen)) if w in {o // 16 for o in few.tolist()}}
    assert len(dirty) == 2 and len(few) == len(at) - 1
    for name in ref.GUARD_MUTANTS:
        assert ref.guard_model(nbytes, gen, few, name) != ref.guard_model(nbytes, gen, few), name
    for name in ref.GUARD_MUTANTS:
        assert ref.guard_model(nbytes, gen, at, name) != (taken, hit), name
    verdicts = [ref.window_model(nbytes, g, moves_ref.write_offsets(w, nbytes, g)) for g, w in ref.window_cases(nbytes)]
    assert verdicts == [False, True, True]
    slipped = [ref.window_model(nbytes, g, moves_ref.write_offsets(w, nbytes, g), "guard-base-32-bit")
               for g, w in ref.window_cases(nbytes)]
    assert slipped != verdicts


# ---------------------------------------------------------------- the relay
def test_the_relay_case_crosses_the_lines_at_a_stripe_border():
    pl = ref.relayed()
    stripe = ref.relay_stripe(pl.nbytes)
    assert stripe % 4096 == 0 and ref.L31 < stripe < pl.nbytes <= 2 * stripe and pl.borders == (stripe,)
    assert any(a <= stripe - 1 and stripe < b for a, b in pl.wins)
    from tests import relay_ref
    assert stripe == relay_ref.stripe_bytes(pl.nbytes, ref.RELAY_WORLD) and ref.RELAY_FILL == relay_ref.SENTINEL
    assert set(ref.RELAY_FORMS) <= set(relay_ref.FORMS) and ref.RELAY_PICKS == relay_ref.PICKS[2][0]


@pytest.mark.parametrize("form", ref.RELAY_FORMS)
def test_the_relay_model_and_its_slips(form):
    pl = ref.relayed()
    mine, peer = ref.learner(pl, 0), ref.learner(pl, 1)
    want = ref.relay_model(pl, mine, peer, form)
    direct = _direct_windows(pl, mine, peer)
    assert want["param"].stray == 0 and all(np.array_equal(g, w) for (_, _, g), (_, _, w) in zip(want["param"].windows, direct))
    if form == "gather":
        assert want["staged"].stray == 0 and all(np.array_equal(g, d) for (_, _, g), d in zip(want["staged"].windows, peer.data))
    lived = 0
    for name in ref.MUTANTS:
        got = ref.relay_model(pl, mine, peer, form, name)
        if got is not None:
            lived += 1
            assert ref.failures(pl, got, want, exact_bytes=False), (form, name)
    for name in ref.RELAY_MUTANTS:
        if form == "fused" or name != "stripe-span-mod-2^32":
            assert ref.relay_model(pl, mine, peer, form, name) is not None, (form, name)
    assert lived >= 2
