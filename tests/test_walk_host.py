"""The walks of tests/walk_ref.py are worth running (no GPU): the model driven in the reference's loop
order gives what the scripted rounds expect, the committed walks and directed sequences together reach
every operation, refusal, pair of calls, slot, ring place and fetch phase, no walk is mostly refusals
or no-ops, and every model with one bookkeeping error differs from the model somewhere a caller can see.
"""
import functools
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
    out = {W.walk_id(w): W.walk_of(w) for w in W.WALKS}
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
    assert ran >= set(W.OPS) - {"step"}, set(W.OPS) - ran
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


@pytest.mark.parametrize("walk", W.WALKS, ids=W.walk_id)
def test_a_walk_is_neither_mostly_refusals_nor_mostly_no_ops(walk):
    rows = traces()[W.walk_id(walk)]
    assert len(rows) == W.WALK_LENGTH
    refused = sum(1 for _, rc, *_ in rows if rc != W.OK)
    assert 4 * refused <= len(rows), (refused, len(rows))
    averaging = [row for row in rows if row[0][0] in W.AVERAGING]
    good = sum(1 for _, rc, _, changed, _ in averaging if rc == W.OK and changed)
    assert averaging and 3 * good >= len(averaging), (good, len(averaging))


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
}


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
    caught = {mu for mu in W.MUTANTS for n in walks if W.first_difference(*committed()[n], mu) is not None}
    assert caught == set(W.MUTANTS), sorted(set(W.MUTANTS) - caught)
