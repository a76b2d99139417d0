"""The walks of tests/walk_ref.py are worth running (no GPU): the model driven in the reference's loop
order gives what the scripted rounds expect, the committed walks and directed sequences together reach
every operation, refusal, pair of calls, slot, ring place and fetch phase, no walk is mostly refusals
or no-ops, and every model with one bookkeeping error differs from the model somewhere a caller can see.
The walks with the non-finite check on skip rounds and average checked ones, their skipped rounds cover
every averaging form, poison position and kind, and the walks from before those calls are held call for
call by a hash.
"""
import functools
import hashlib
import os

import numpy as np
import pytest

from oracle import lerp as olerp
from tests import factor_ref
from tests import forms_ref as fref
from tests import walk_ref as W
from tests.helpers import load_json, load_npz
from tests.test_gpu_f16 import FUSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def committed():
    """name -> (spec, ops) of every committed walk and directed sequence."""
    out = {W.walk_id(w): W.walk_of(w) for w in W.WALKS + W.CHECK_WALKS}
    out.update(W.directed())
    return out


@functools.lru_cache(maxsize=None)
def traces():
    """name -> [(op, rc, rule, model after the call)]."""
    out = {}
    for name, (spec, ops) in committed().items():
        m, rows = W.Model(spec), []
        for op in ops:
            rc = m.apply(op)
            rows.append((op, rc, m.rule, m.changed, m.copy()))
        out[name] = rows
    return out


# ---------------------------------------------------------------- the walks from before the newer calls
OLD_DIRECTED = ("factor-after-ahead-header", "factor-after-ahead-header-resident", "clock-ring", "slot-parity",
                "written-through", "res-slot", "slot-readers", "staging", "fetch-phase", "distance", "distance-mixed",
                "distance-forms", "previous-version", "no-elements", "many-order", "every-pair")
# sha256 over repr((name, ops)) of W.WALKS and OLD_DIRECTED in this order, computed on the commit before
# set_finite_check and set_param_distance joined the model
OLD_OPS_SHA256 = "5af28388270e35a79bf8b7c34d5d41a09537cc05ebd90980ae0c2948387c98fb"


def test_the_earlier_walks_and_sequences_are_call_for_call_what_they_were():
    """FIRST_DIFFERENCE pins indices into them, and _draw must not consume its rng differently for them."""
    h = hashlib.sha256()
    for w in W.WALKS:
        h.update(repr((W.walk_id(w), W.walk_of(w)[1])).encode())
    assert tuple(W.directed())[:len(OLD_DIRECTED)] == OLD_DIRECTED
    for name in OLD_DIRECTED:
        h.update(repr((name, list(W.directed()[name][1]))).encode())
    assert h.hexdigest() == OLD_OPS_SHA256
    # (repr would shorten a step's array: the hash is sound because none of them holds one)
    newer = ("set_finite_check", "set_param_distance", "step")
    assert not any(op[0] in newer for n in OLD_DIRECTED for op in W.directed()[n][1])
    assert not any(op[0] in newer for w in W.WALKS for op in W.walk_of(w)[1])


# ---------------------------------------------------------------- the rules cite lines that exist
def test_every_rule_cites_a_line_of_the_code():
    text = {}
    for name, (rc, path, line) in W.RULES.items():
        if path not in text:
            with open(os.path.join(ROOT, path)) as f:
                text[path] = f.read()
        assert line in text[path], (name, path, line)
        assert rc in (None, W.ERR_ARG, W.ERR_STATE), name


# ---------------------------------------------------------------- loop order
FORMS = ("average", "average_through", "factor-lerp", "resident", "many")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", fref.DTYPES)
def test_one_round_in_loop_order_gives_the_scripted_rounds_values(dtype, form):
    """publish, fetch, average in each form on the cases of tests/test_gpu_f16.FUSED: the parameters are
    forms_ref.case's, the coefficients and the clock factor_ref.evaluate's."""
    n = fref.multi_span(dtype)
    seed = fref.seed_of(dtype, n)
    for case in FUSED:
        method, value, thr, my_clock, peer_clock, loss, peer_loss = case
        f, new_clock, a, b = factor_ref.evaluate(case)
        p, q, want = fref.case(dtype, n, seed, f)
        spec = W.Spec(dtype, method, value, thr, n=n, seed=seed)
        m = W.Model(spec)
        assert m.L[0].flats[0].tobytes() == p.tobytes() and m.L[0].flats[1].tobytes() == q.tobytes()
        ops = [("step", 1, 1, q), ("write_clock", 1, peer_clock - 1.0), ("publish", 1, 1, peer_loss)]   # learner 1 serves q
        if form == "resident":
            ops += [("set_resident", 0)]
        ops += [("write_clock", 0, my_clock), ("fetch", 0, 1, 1, "ce")]
        flat = "res" if form == "resident" else 0
        ops += {"average": [("average", 0, 0, loss)], "average_through": [("average_through", 0, 0, loss)],
                "factor-lerp": [("factor", 0, loss), ("lerp", 0, 0)], "resident": [("average", 0, "res", loss)],
                "many": [("fetch", 2, 1, 1, "zc"), ("average_many", ((2, 0, loss, 1), (0, 0, loss, 0)))]}[form]
        for op in ops:
            assert m.apply(op) == W.OK, (case, op, m.rule)
        l = m.L[0]
        got = m.params(0, m.params_key(0, flat))
        assert fref.same(dtype, got, np.array(want)), (case, form)
        assert factor_ref.same_result(l.coef[:4], (f, new_clock, a, b)) and l.coef[4] == 0, (case, l.coef)
        assert l.clock[l.cur] == new_clock, (case, l.clock, l.cur)
        if form in ("average_through", "resident"):
            k = l.version % 2
            assert fref.same(dtype, l.slots[k].payload, np.array(want)), (case, form, "the next slot")
            ahead = method != "loss"
            assert l.wt == [("slot", k) if form == "resident" else ("flat", 0), ahead]
            if ahead:
                assert W.header_same(l.slots[k].header, (new_clock + 1.0, float("nan"), 1, n, fref.CODE[dtype]))
                assert l.clock[(l.cur + 1) & 3] == new_clock + 1.0


def test_zero_division_round_changes_nothing_but_the_ring_place():
    method, value, thr, my_clock, peer_clock, loss, peer_loss = fref.ZERO_DIVISION
    m = W.Model(W.Spec("f32", method, value, thr))
    before = m.L[0].flats[0].copy()
    for op in [("write_clock", 1, -1.0), ("publish", 1, 0, peer_loss), ("fetch", 0, 1, 1, "zc"),
               ("set_distance", 0, 1), ("average_through", 0, 0, loss)]:
        assert m.apply(op) == W.OK
    l = m.L[0]
    assert l.coef == (0.0, 0.0, 0.0, 1.0, 1) and l.cur == 1 and l.clock[1] == 0.0 and not m.changed
    assert l.flats[0].tobytes() == before.tobytes() == l.slots[0].payload.tobytes()
    assert l.dist == (0.0, 0.0, 0.0, 0)


def test_several_rounds_in_loop_order_give_the_golden_trajectory():
    """tests/golden/gossip.*: update_send for all, the step, update_wait for all, eight rounds."""
    meta, z = load_json("gossip.json"), load_npz("gossip.npz")
    for case in meta["cases"]:
        k, names, G = case["key"], case["names"], case["G"]
        init, deltas = z[k + "_init"], z[k + "_deltas"]
        spec = W.Spec("f32", case["interpolation"], case["value"], case["divergence_threshold"], n=init.shape[1],
                      learners=G)
        m = W.Model(spec)
        for g in range(G):
            assert m.apply(("step", g, 0, init[g].view(np.uint32))) == W.OK
        for r in range(deltas.shape[0]):
            for g in range(G):
                assert m.apply(("publish", g, 0, case["send_loss"][r][g])) == W.OK
            for g in range(G):
                stepped = m.L[g].flats[0].view(np.float32) + deltas[r, g]
                m.apply(("step", g, 0, stepped.view(np.uint32)))
            for g in range(G):
                factor = 0.0
                for name in case["picks"][r][g]:
                    j = names.index(name)
                    for op in (("fetch", g, j, m.L[j].version, "ce"), ("average", g, 0, case["wait_loss"][r][g])):
                        assert m.apply(op) == W.OK, (k, r, g, op, m.rule)
                    factor = m.L[g].coef[0]
                assert factor == z[k + "_factors"][r, g], (k, r, g)
                assert m.L[g].clock[m.L[g].cur] == z[k + "_clocks"][r, g], (k, r, g)
                assert olerp.bits_equal(m.L[g].flats[0].view(np.float32), z[k + "_params"][r, g]), (k, r, g)


# ---------------------------------------------------------------- what the committed walks are
def test_a_refused_call_changes_nothing():
    for name, rows in traces().items():
        spec, _ = committed()[name]
        before = W.Model(spec)
        for t, (op, rc, rule, _, after) in enumerate(rows):
            assert (rc == W.OK) == (rule is None), (name, t, op)
            if rc != W.OK:
                assert rc == W.RULES[rule][0], (name, t, op, rule)
                assert after.observe()[0] == before.observe()[0], (name, t, op)
                for a, b in zip(after.L, before.L):
                    assert (a.cur, a.wt, a.reading, a.fetch is None) == (b.cur, b.wt, b.reading, b.fetch is None), (name, t, op)
                    assert (a.check, a.skips, a.sticky, a.pd_on, a.pd_every, a.pd_rounds) == \
                           (b.check, b.skips, b.sticky, b.pd_on, b.pd_every, b.pd_rounds), (name, t, op)
                assert not after.skipped and not after.measured and not after.checked, (name, t, op)
            before = after


def test_every_fetch_names_a_version_whose_slot_the_owner_is_not_writing():
    """The peer's current version, or the one before it while no written-through snapshot is pending on
    the owner (whose payload lies in that very slot); anything else is refused."""
    older = 0
    for name, rows in traces().items():
        spec, _ = committed()[name]
        before = W.Model(spec)
        for t, (op, rc, rule, _, after) in enumerate(rows):
            if op[0] == "fetch" and rc == W.OK:
                owner = before.L[op[2]]
                assert op[3] == owner.version or (op[3] == owner.version - 1 and owner.wt is None), (name, t, op)
                older += op[3] != owner.version
            before = after
    assert older >= 2
    # the reader of the older version holds off the publish, the write-through average and the relocation
    held = [(row[0][0], row[2]) for row in traces()["previous-version"] if row[2] == "slot-still-read"]
    assert {name for name, _ in held} >= {"publish", "average_through", "relocate"}, held


def finite(x):
    return x == x and abs(x) != float("inf")


def test_every_measuring_form_writes_a_finite_record_that_is_not_zero():
    """On the hard bit patterns every sum is NaN or infinite, where dist_ref.problem asks only for that; the
    finite-operand walks and the distance sequences hold each form that measures to dist_ref.bound."""
    forms, per_walk = set(), {}
    for name, rows in traces().items():
        for op, rc, _, _, m in rows:
            for i, form in m.measured:
                d2, n2, _, n = m.L[i].dist
                if finite(d2) and finite(n2) and d2 > 0.0 and n2 > 0.0:
                    forms.add(form)
                    per_walk[name] = per_walk.get(name, 0) + 1
    assert forms >= set(W.MEASURING), set(W.MEASURING) - forms
    for w in W.WALKS:
        if w[4]:
            assert per_walk.get(W.walk_id(w), 0) >= 10, (W.walk_id(w), per_walk)
    assert {w[0] for w in W.WALKS if w[4]} == set(W.PROFILES)
    for name in ("distance", "distance-mixed", "distance-forms"):
        assert per_walk.get(name, 0) >= 4, (name, per_walk)
    # a no-op round leaves the record as it was
    rows = traces()["distance"]
    at = next(t for t, row in enumerate(rows) if row[4].L[0].coef[4] == 1)
    assert rows[at][4].L[0].dist == rows[at - 1][4].L[0].dist and not rows[at][4].measured


def main_calls(rows):
    """Per learner, the main calls issued to it in order."""
    per = {}
    for op, *_ in rows:
        if op[0] in W.MAIN:
            per.setdefault(op[1], []).append(op[0])
    return per


def test_coverage_of_the_committed_walks():
    ran, fired, pairs, parities, places, phases = set(), set(), set(), set(), set(), set()
    for name, rows in traces().items():
        for calls in main_calls(rows).values():
            pairs |= set(zip(calls, calls[1:]))
        for op, rc, rule, _, after in rows:
            if rc == W.OK:
                ran.add(op[0])
                if op[0] in ("publish", "publish_reuse"):
                    parities.add((after.L[op[1]].version - 1) % 2)
            else:
                fired.add(rule)
            for l in after.L:
                places.add(l.cur)
                if l.fetch is not None:
                    phases.add((l.fetch.kind, l.fetch.factored))
    assert ran >= set(W.OPS), set(W.OPS) - ran
    assert fired >= set(W.REFUSALS), set(W.REFUSALS) - fired
    missing = {(a, b) for a in W.MAIN for b in W.MAIN} - pairs
    assert not missing, sorted(missing)
    assert parities == {0, 1} and places == {0, 1, 2, 3}
    assert phases == {(k, f) for k in W.FETCH_KINDS for f in (False, True)}, phases


def test_the_directed_sequences_reach_what_they_are_named_for():
    t = traces()
    rules = lambda name: {row[2] for row in t[name]}                                        # noqa: E731
    assert "slot-still-read" in rules("slot-readers") and "slot-still-read" in rules("slot-parity")
    assert {"set-resident-twice", "resident-publish-pointer", "resident-average-pointer", "relocate-with-fetch",
            "lerp-resident", "slot-still-read"} <= rules("res-slot")
    assert {"factor-twice", "average-after-factor", "lerp-without-factor"} <= rules("fetch-phase")
    assert {l.res_slot for *_, m in t["res-slot"] for l in m.L if l.resident} == {0, 1}
    assert any(m.L[0].wt == [("flat", 0), True] for *_, m in t["factor-after-ahead-header"])
    assert {m.L[0].cur for *_, m in t["clock-ring"]} == {0, 1, 2, 3}
    assert any(m.L[0].dist is not None and m.L[0].dist[3] == 261 for *_, m in t["distance"])
    assert all(len(l.flats[0]) == 0 for *_, m in t["no-elements"] for l in m.L)
    # a factor after an ahead-written header: the served header carries the factor's clock, the live clock is the served one
    rows = t["factor-after-ahead-header"]
    at = next(i for i, row in enumerate(rows) if row[0][0] == "publish_reuse")
    m, factored = rows[at][4], rows[at - 2][4]
    assert m.L[0].slots[1].header[0] == factored.L[0].coef[1] + 1.0 == m.L[0].clock[m.L[0].cur]
    assert m.L[0].slots[1].header[1] == 0.75 and m.L[0].slots[1].header[2] == 2


@pytest.mark.parametrize("walk", W.WALKS + W.CHECK_WALKS, ids=W.walk_id)
def test_a_walk_is_neither_mostly_refusals_nor_mostly_no_ops(walk):
    """(The walk on the hard bit patterns with the check on is exempt from the second cap: nearly every snapshot
    there holds a NaN or an infinity, so nearly every checked round is skipped -- which is what it is for.)"""
    rows = traces()[W.walk_id(walk)]
    assert len(rows) == (W.WALK_LENGTH if walk in W.WALKS else W.CHECK_WALK_LENGTH)
    refused = sum(1 for _, rc, *_ in rows if rc != W.OK)
    assert 4 * refused <= len(rows), (refused, len(rows))
    averaging = [row for row in rows if row[0][0] in W.AVERAGING]
    good = sum(1 for _, rc, _, changed, _ in averaging if rc == W.OK and changed)
    assert averaging and (walk == W.ALL_HARD or 3 * good >= len(averaging)), (good, len(averaging))


def skipped_rounds(rows):
    """[(learner, form, poison tags)] of the rounds a trace skipped, and its checked rounds that averaged."""
    skipped = [x for *_, m in rows for x in m.skipped]
    return skipped, sum(m.checked for *_, m in rows)


@pytest.mark.parametrize("walk", W.CHECK_WALKS, ids=W.walk_id)
def test_a_checking_walk_skips_rounds_and_averages_checked_ones(walk):
    """At least 8 skipped rounds and at least 8 checked rounds that averaged.  On the hard bit patterns every
    learner's parameters hold a NaN or an infinity from the start and stay so, so no checked round can average:
    there every checked round that is no ZeroDivision is skipped, and every learner skips several."""
    rows = traces()[W.walk_id(walk)]
    skipped, averaged = skipped_rounds(rows)
    rounds = {(t, x[0]) for t, (*_, m) in enumerate(rows) for x in m.skipped}
    assert len(rounds) >= 8, len(rounds)
    if walk != W.ALL_HARD:
        assert averaged >= 8, averaged
        assert all(tags for _, _, tags in skipped), "a skipped round whose snapshot holds no poison the walk wrote"
    else:
        assert averaged == 0
        per_learner = [sum(1 for _, i in rounds if i == k) for k in range(3)]
        assert min(per_learner) >= 3, per_learner
        assert rows[-1][4].L[0].skips + rows[-1][4].L[1].skips + rows[-1][4].L[2].skips == len(rounds)


def test_every_checking_walk_draws_the_calls_its_spec_asks_for():
    for w in W.CHECK_WALKS:
        drawn = {op[0] for op in committed()[W.walk_id(w)][1]}
        assert "set_finite_check" in drawn and (("set_param_distance" in drawn) == ("param" in w[5])), W.walk_id(w)
        assert ("step" in drawn) == w[4], W.walk_id(w)


def test_the_skipped_rounds_cover_every_form_and_every_poison():
    forms, where, kinds = set(), set(), set()
    for name, rows in traces().items():
        spec = committed()[name][0]
        if not spec.finite:      # (on the hard bit patterns a named element can hold one of the patterns by chance)
            continue
        for _, form, tags in skipped_rounds(rows)[0]:
            forms.add(form)
            where |= {(spec.dtype, w) for w, _ in tags}
            kinds |= {k for _, k in tags}
    assert forms >= set(W.MEASURING), set(W.MEASURING) - forms
    everywhere = {(d, w) for d in W.DTYPES for w in W.POISON_AT[d]}
    assert where == everywhere, everywhere - where
    assert kinds == set(W.POISON_KINDS), kinds


def test_the_parameter_ranges_are_what_the_walks_are_said_to_use():
    """One list per dtype: a tensor that ends inside the first 1-KiB span, an empty one, a gap, a tensor across
    the span boundary that ends with the ragged tail; every segment of a segmented payload holds them all;
    the poison called "gap" lies in no tensor."""
    for dtype in W.DTYPES:
        spec = W.profile_spec(dtype, "plain")
        ranges = spec.param_ranges()
        ends = [off + length for off, length, _ in ranges]
        assert all(off % 256 == 0 for off, _, _ in ranges) and all(b[0] >= a for a, b in zip(ends, ranges[1:]))
        segs = [(0, spec.nbytes)]
        if dtype == "mixed":
            segs = [(o, o + n * W.mixed_ref.SIZE[d]) for d, o, _, n in W.mixed_ref.segments(W.MIXED_SPEC)[0]]
        for lo, hi in segs:
            mine = [(off - lo, off + length - lo) for off, length, _ in ranges if lo <= off < hi]
            assert any(0 < e < 1024 for _, e in mine) and any(b == e for b, e in mine)
            assert any(b < 1024 < e and e == hi - lo for b, e in mine), (dtype, mine)
            assert any(b2 > e1 for (_, e1), (b2, _) in zip(mine, mine[1:]))
        for where in W.POISON_AT[dtype]:
            d, byte, _ = W._element(spec, where)
            assert ("gap" in where) == (not any(off <= byte < off + length for off, length, _ in ranges)), (dtype, where)
            assert byte + W.finite_ref.SIZE[d] <= spec.nbytes


def test_the_new_sequences_reach_what_they_are_named_for():
    t = traces()

    def status(rows, i):
        """The status of learner i's coefficients after each of its factors, lerps and averages."""
        return [m.L[i].coef[4] for op, rc, _, _, m in rows if rc == W.OK and op[0] in W.AVERAGING + ("factor",) and
                (op[1] == i if op[0] != "average_many" else any(e[0] == i for e in op[1]))]

    # skipped, finite, skipped, finite; a refused prepared average between two checked rounds
    assert status(t["veto-stamp"], 0) == [2, 0, 2, 0, 2, 0]
    at = next(k for k, row in enumerate(t["veto-stamp"]) if row[2] == "slot-still-read")
    assert t["veto-stamp"][at][0][0] == "average_through" and t["veto-stamp"][at][4].L[0].check
    switched = [row[0][2] for row in t["veto-stamp"] if row[0][0] == "set_finite_check"]
    assert switched == [1, 0, 1]
    # the hole: both refusals, copied and in place; with the check off the second fetch keeps the factor
    rows = t["second-fetch-checked"]
    refused = [(row[0][0], row[0][-1], row[2]) for row in rows if row[1] != W.OK]
    assert refused == [("fetch", "ce", "fetch-over-checked-factor"), ("fetch", "zc", "fetch-over-checked-factor"),
                       ("set_finite_check", 1, "set-check-over-factor"), ("set_finite_check", 1, "set-check-over-factor")]
    assert all(not sp.vetoes(m.L[0].flats[0]) for sp, (op, _, _, _, m) in ((committed()["second-fetch-checked"][0], r) for r in rows)
               if m.L[0].check), "a checking learner's parameters went non-finite"
    # every form skipped once and followed by a finite round, both records on
    for name, many in (("skip-every-form", "many-batched"), ("skip-every-form-segmented", "many-unbatched")):
        skipped, _ = skipped_rounds(t[name])
        assert [f for _, f, _ in skipped] == ["average", "average_through", "resident", "lerp", many], skipped
        assert status(t[name], 0) == [2, 0] * 2 + [2, 2, 0, 0] + [2, 0] and status(t[name], 1) == [2, 0]
        last = t[name][-1][4]
        assert last.L[0].pd_rounds == (8, 8) and last.L[0].skips == 4 and last.L[0].dist[3] > 0
        assert last.L[0].pd[1] == len(committed()[name][0].param_ranges()) >= 4
    # the dispatch of four
    rows = t["many-one-poisoned"]
    at = next(k for k, row in enumerate(rows) if row[0][0] == "average_many")
    m, sp = rows[at][4], committed()["many-one-poisoned"][0]
    assert [l.coef[4] for l in m.L[:4]] == [0, 2, 0, 0] and [l.skips for l in m.L[:4]] == [0, 1, 0, 0]
    assert sp.vetoes(m.L[3].flats[0]) and not any(sp.vetoes(l.flats[0]) for l in m.L[:3])
    assert {f for _, f, _ in m.skipped} == {"many-batched"}
    assert not finite(m.L[3].dist[0]) and m.L[3].pd[1] == 4 and all(finite(a) and finite(b) for a, b in m.L[3].pd[2])
    # both a ZeroDivision and poisoned: a ZeroDivision, not counted; the sticky word says so, a skip never does
    rows = t["zero-division-and-poison"]
    assert status(rows, 0) == [1, 1, 1, 2] and [r[4].L[0].skips for r in rows][-2:] == [0, 1] and rows[-1][4].L[0].sticky == 1
    assert all(m.L[i].sticky == 0 for n, rws in t.items() if n != "zero-division-and-poison" and n in W._checked_sequences()
               for *_, m in rws for i in range(len(m.L)))
    # every = 3: rounds 3 and 9 write the record, round 6 is due and skipped; counters start anew and freeze
    rows = t["param-every"]
    seen = [(m.L[0].pd_rounds, m.L[0].pd[1], m.L[0].pd[2]) for op, rc, _, _, m in rows
            if op[0] in W.AVERAGING and rc == W.OK]
    assert [r for r, _, _ in seen] == [(k, k // 3) for k in range(1, 11)] + [(10, 3), (1, 0), (2, 1), (2, 1)]
    assert [c for _, c, _ in seen] == [0, 0] + [4] * 9 + [0, 4, 4]
    assert seen[2][2] == seen[5][2] == seen[7][2] != seen[8][2], "the skipped due round wrote the record"
    # unaligned parameters: refused from every entry, nothing counted
    rows = t["param-unaligned-refused"]
    assert [row[0][0] for row in rows if row[2] == "param-unaligned"] == ["average", "average_through", "lerp", "average_many", "average"]
    assert rows[-1][4].L[0].pd_rounds == (0, 0) and rows[-1][4].L[1].pd_rounds == (1, 1)
    # its own parameters are poisoned: it averages; the peer that fetches it skips
    rows = t["own-params-poisoned"]
    assert status(rows, 0) == [0] and status(rows, 2) == [2, 0] and committed()["own-params-poisoned"][0].vetoes(rows[-1][4].L[0].flats[0])


def test_without_the_fix_the_parameters_first_differ_at_the_lerp_of_the_second_fetch():
    """The code before the fix accepts the second fetch (where the return codes part); what a caller holds
    in its parameters first differs at the lerp that follows, which writes the infinity."""
    spec, ops = committed()["second-fetch-checked"]
    a, b = W.Model(spec), W.Model(spec, "lerp-after-second-fetch-unchecked")
    for t, op in enumerate(ops):
        rcs = a.apply(op), b.apply(op)
        if a.L[0].flats[0].tobytes() != b.L[0].flats[0].tobytes():
            break
        assert rcs[0] == rcs[1] or op[0] in ("fetch", "set_finite_check"), (t, op)
    assert (t, ops[t][0], ops[t - 1][0]) == (8, "lerp", "fetch")
    assert spec.vetoes(b.L[0].flats[0]) and not spec.vetoes(a.L[0].flats[0]) and b.L[0].check


# ---------------------------------------------------------------- mutants
# mutant -> (the first committed walk or sequence, in committed()'s order, on which it differs from the
# model; the index of the first call after which it does; that call's name)
FIRST_DIFFERENCE = {
    'factor-keeps-ahead-header': ('mix-bf16-aligned-seed1', 148, 'publish_reuse'),
    'lerp-keeps-written-through': ('through-f32-aligned-seed1', 134, 'publish_reuse'),
    'cancel-keeps-reader': ('plain-f32-aligned-seed1', 26, 'publish_reuse'),
    'parity-from-next-version': ('plain-f32-aligned-seed1', 2, 'publish'),
    'ahead-clock-one-place': ('plain-f32-aligned-seed1', 137, 'average_through'),
    'resident-publish-no-relocate': ('resident-f32-aligned-seed1', 29, 'publish_reuse'),
    'second-fetch-resets-factor': ('plain-f32-aligned-seed1', 83, 'lerp'),
    'many-one-by-one': ('through-f32-aligned-seed1', 87, 'average_many'),
    'write-clock-keeps-header': ('through-bf16-aligned-seed1', 53, 'publish_reuse'),
    'distance-after-the-lerp': ('plain-f32-off1-seed1', 33, 'average'),
    'distance-against-staging': ('plain-bf16-off1-seed2-finite', 26, 'average'),
    'skip-moves-clock': ('plain-f32-aligned-seed4-finite-check', 41, 'average_many'),
    'skip-writes-whole-record': ('plain-f32-aligned-seed4-finite-check', 41, 'average_many'),
    'skip-writes-param-record': ('through-f32-aligned-seed9-finite-check-param', 33, 'average_through'),
    'skip-leaves-snapshot-stale': ('plain-f32-aligned-seed4-finite-check', 126, 'average_through'),
    'stale-veto': ('plain-f32-aligned-seed4-finite-check', 60, 'average'),
    'check-reads-own-params': ('plain-f32-aligned-seed4-finite-check', 22, 'factor'),
    'zero-division-loses-precedence': ('zero-division-and-poison', 5, 'average'),
    'skip-sets-sticky-status': ('plain-f32-aligned-seed4-finite-check', 41, 'average_many'),
    'many-shares-one-veto': ('plain-f32-aligned-seed4-finite-check', 41, 'average_many'),
    'many-checks-first-member-only': ('through-bf16-aligned-seed9-finite-check', 87, 'average_many'),
    'param-every-off-by-one': ('through-f32-aligned-seed9-finite-check-param', 15, 'average_through'),
    'param-reset-keeps-counters': ('through-f32-aligned-seed9-finite-check-param', 62, 'set_param_distance'),
    'param-record-after-the-lerp': ('through-f32-aligned-seed9-finite-check-param', 23, 'average_through'),
    'lerp-after-second-fetch-unchecked': ('mix-mixed-aligned-seed32-finite-check', 58, 'set_finite_check'),
}
FIRST_DIRECTED = {
    'factor-keeps-ahead-header': ('factor-after-ahead-header', 8, 'publish_reuse'),
    'lerp-keeps-written-through': ('written-through', 7, 'publish_reuse'),
    'cancel-keeps-reader': ('slot-parity', 6, 'publish'),
    'parity-from-next-version': ('factor-after-ahead-header', 0, 'publish'),
    'ahead-clock-one-place': ('factor-after-ahead-header', 4, 'average_through'),
    'resident-publish-no-relocate': ('res-slot', 5, 'publish'),
    'second-fetch-resets-factor': ('fetch-phase', 10, 'lerp'),
    'many-one-by-one': ('many-order', 5, 'average_many'),
    'write-clock-keeps-header': ('clock-ring', 8, 'publish_reuse'),
    'distance-after-the-lerp': ('distance', 6, 'average'),
    'distance-against-staging': ('distance-mixed', 11, 'lerp'),
    'skip-moves-clock': ('veto-stamp', 7, 'average'),
    'skip-writes-whole-record': ('veto-stamp', 7, 'average'),
    'skip-writes-param-record': ('skip-every-form', 13, 'average'),
    'skip-leaves-snapshot-stale': ('veto-stamp', 21, 'average_through'),
    'stale-veto': ('veto-stamp', 9, 'average'),
    'check-reads-own-params': ('own-params-poisoned', 5, 'average'),
    'zero-division-loses-precedence': ('zero-division-and-poison', 5, 'average'),
    'skip-sets-sticky-status': ('veto-stamp', 7, 'average'),
    'many-shares-one-veto': ('many-one-poisoned', 15, 'average_many'),
    'many-checks-first-member-only': ('many-one-poisoned', 15, 'average_many'),
    'param-every-off-by-one': ('param-every', 10, 'average'),
    'param-reset-keeps-counters': ('param-every', 32, 'set_param_distance'),
    'param-record-after-the-lerp': ('skip-every-form', 15, 'average'),
    'lerp-after-second-fetch-unchecked': ('second-fetch-checked', 7, 'fetch'),
}
# (a round that is both a ZeroDivision and poisoned needs both clocks at 0 and a poisoned peer at once: no
# seeded walk meets one, the sequence written for it does)
ONLY_DIRECTED = {"zero-division-loses-precedence"}


def test_every_mutant_differs_from_the_model_on_a_committed_walk():
    """Each model with one bookkeeping error gives, on at least one committed walk or sequence, another
    return code or observable value than the model; the first such walk and call are pinned above, so a
    change of the walks that moves them shows."""
    found = {}
    for mutant in W.MUTANTS:
        for name, (spec, ops) in committed().items():
            at = W.first_difference(spec, ops, mutant)
            if at is not None:
                found[mutant] = (name, at, ops[at][0])
                break
    assert found == FIRST_DIFFERENCE, found
    assert set(found) == set(W.MUTANTS)
    # among the directed sequences each is caught first by one written for that state variable
    first_directed = {}
    for mutant in W.MUTANTS:
        for name, (spec, ops) in W.directed().items():
            at = W.first_difference(spec, ops, mutant)
            if at is not None:
                first_directed[mutant] = (name, at, ops[at][0])
                break
    assert first_directed == FIRST_DIRECTED, first_directed
    # and the random walks catch every one of them without the directed sequences
    walks = sorted(W.walk_id(w) for w in W.WALKS)
    old = set(W.MUTANTS) - set(W.NEW_MUTANTS)
    caught = {mu for mu in old for n in walks if W.first_difference(*committed()[n], mu) is not None}
    assert caught == old, sorted(old - caught)
    # (the newer mutants need a learner that checks or measures per parameter: the walks that draw those calls)
    walks = {W.walk_id(w) for w in W.CHECK_WALKS}
    assert {mu for mu in W.NEW_MUTANTS if found[mu][0] in walks} == set(W.NEW_MUTANTS) - ONLY_DIRECTED
