"""tests/adapter_ref.py is worth replaying (no GPU): torch behaves as its op table says, the committed
walks reach every op and every decision often enough, every wrong adapter restated on the model differs
from it on them, and the model's layout is the flat buffer's."""
import collections
import functools

import numpy as np
import pytest
import torch

from dpwa_amd.flat import FlatParameters, layout_digest
from tests import adapter_ref as A

CASES = [(model, op.name) for model in A.MODELS for op in A.OPS.values() if op.applies(model)]


@functools.lru_cache(maxsize=None)
def committed():
    """name -> (walk, events) of every committed walk and directed sequence, walks first."""
    out = {w.name: (w, A.script(w)) for w in A.WALKS}
    out.update(A.directed())
    return out


@functools.lru_cache(maxsize=None)
def rows(name):
    return A.run_host(*committed()[name])


# ---------------------------------------------------------------- torch does what the table says
@pytest.mark.parametrize("model,name", CASES)
def test_op_class_on_the_cpu(model, name):
    """The class the adapter can see the op by, on CPU FlatParameters.  A torch upgrade that moves a
    version counter where none moved (or the other way) fails here."""
    net = A.build(model, 3)
    flat = FlatParameters(net.named_parameters())
    op = A.OPS[name]
    assert A.observe(op, net, flat, 5) == op.cls


def test_the_table_holds_the_ops_the_adapter_meets():
    assert len(A.OPS) >= 24
    assert {op.cls for op in A.OPS.values()} == set(A.CLASSES)
    for name in ("sgd_fused", "adam_fused", "adamw_fused", "sgd_foreach", "sgd_single", "adam_foreach", "sgd_one_small",
                 "load_sd", "load_sd_assign", "attr_replace"):
        assert name in A.OPS
    assert all(op.cls == "silent" and op.steps for op in A.OPS.values() if op.fused)


# ---------------------------------------------------------------- the committed walks are worth replaying
def test_the_walks_cover_the_forms_and_models():
    assert len(A.WALKS) == 20 and all(w.rounds == 40 for w in A.WALKS)
    assert {(w.model, w.form) for w in A.WALKS} == {(m, f) for m in A.MODELS for f in A.FORMS}
    assert sum(w.method == "clock" for w in A.WALKS) == 5


def test_every_op_occurs_at_least_three_times():
    count = collections.Counter(ev[3] for w in A.WALKS for ev in A.script(w) if ev[0] == "op")
    assert not [name for name in A.OPS if count[name] < 3], count


@pytest.mark.parametrize("form", A.WRITE_THROUGH)
def test_every_class_is_followed_by_an_update_send(form):
    """In every write-through form an op of every class -- and an optimizer step of every kind -- is the
    last thing that happens to a learner before an update_send that could have reused."""
    seen = set()
    for w in A.WALKS:
        if w.form != form:
            continue
        events = A.script(w)
        last = {}
        for ev in events:
            if ev[0] == "op":
                last[ev[2]] = ev
            elif ev[0] == "send" and ev[2] in last:
                op = A.OPS[last.pop(ev[2])[3]]
                seen.add(op.cls)
                if op.fused:
                    seen.add("fused")
            elif ev[0] in ("wait", "wait_many"):
                last.clear()
    assert seen == set(A.CLASSES) | {"fused"}


def test_about_half_of_the_write_through_publishes_reuse():
    pubs = [r for w in A.WALKS if w.form in A.WRITE_THROUGH for r in rows(w.name) if r[2] is not None]
    share = sum(bool(r[2]) for r in pubs) / len(pubs)
    assert 0.3 <= share <= 0.7, share


def test_guarded_publishes_after_silent_writes_hit_and_miss():
    """Reusing publishes of the guarded forms that follow a write no counter saw: at least ten whose
    samples all miss it (the snapshot served is the stale one) and ten that hit."""
    hit = miss = 0
    for w in A.WALKS:
        if w.form not in ("default", "many"):
            continue
        for r in rows(w.name):
            if r[2] and r[6]:
                hit, miss = hit + bool(r[5]), miss + (not r[5])
    assert hit >= 10 and miss >= 10, (hit, miss)


def test_some_rounds_do_not_average():
    for w in A.WALKS:
        assert any(ev[0] == "down" for ev in A.script(w)), w.name


# ---------------------------------------------------------------- mutants
# the first committed walk (in order) on which the mutant shows, and where: (round, learner, what)
FIRST = {
    "first-parameter-versions": ("odd-default-constant-s7", (1, 0, "publish reuse")),
    "no-buffer-counter": ("odd-default-constant-s7", (3, 1, "publish reuse")),
    "rehome-keeps-reuse": ("odd-default-constant-s7", (4, 0, "publish reuse")),
    "reuse-after-no-average": ("odd-default-constant-s7", (8, 1, "publish reuse")),
    "guard-hit-copies-all": ("chunky-default-constant-s107", (4, 0, "publish payload byte 24288")),
    "fused-step-is-none": ("chunky-default-constant-s107", (37, 1, "publish reuse")),
    "replaced-object-kept": ("odd-default-constant-s7", (1, 1, "publish payload byte 0")),
    "gaps-from-parameters": ("odd-default-constant-s7", (0, 0, "publish payload byte 140")),
}


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_every_mutant_differs_from_the_model(mutant):
    assert set(FIRST) == set(A.MUTANTS) and len(A.MUTANTS) >= 8
    for name, (walk, events) in committed().items():
        where = A.first_difference(walk, events, mutant)
        if where is not None:
            assert (name, where) == FIRST[mutant]
            return
    pytest.fail("no committed walk tells %s from the model" % mutant)


@pytest.mark.parametrize("name", [n for n in A.directed() if n.startswith("fused-") and "no-average" not in n])
def test_the_fused_sequences_tell_the_unfixed_adapter_by_the_payload(name):
    """Finding 1 as bytes: an adapter that takes a fused step for no write serves a payload that lacks
    it -- with the guard off at the first publish after the step, with it on at the first whose sample of
    chunk 540 lies in the 40,000-element tensor."""
    walk, events = A.directed()[name]
    model, mutant = A.run_host(walk, events), A.run_host(walk, events, "fused-step-is-none")
    stale = [(a[0], a[1]) for a, b in zip(model, mutant) if a[2] is not None and a[4].tobytes() != b[4].tobytes()]
    assert stale, name


# ---------------------------------------------------------------- layout
@pytest.mark.parametrize("model", list(A.MODELS))
def test_the_models_layout_is_the_flat_buffers(model):
    net = A.build(model, 1)
    lay = A.Layout(net)
    flat = FlatParameters(net.named_parameters())
    want = [(name, {torch.float32: "f32", torch.bfloat16: "bf16"}[d], off, length)
            for name, d, off, length in flat.parameter_ranges()]
    assert lay.ranges == want
    assert lay.nbytes == flat.buffer.numel() * flat.buffer.element_size() and lay.n == flat.numel
    assert lay.digest() == flat.layout_digest
    if flat.layout is not None:
        assert lay.digest() == layout_digest(flat.layout)
        assert [(A.DTYPE[d], o, n) for d, o, n in flat.layout] == lay.segments
    assert np.array_equal(A.module_bytes(net, lay), flat.buffer.view(torch.uint8).numpy())   # gaps zero


def test_the_models_sizes():
    odd = A.Layout(A.build("odd", 1))
    assert len(odd.ranges) == 6 and odd.nbytes // 16 < 4096
    assert sorted(n for _, _, _, n in odd.ranges)[:2] == [0, 4]              # an empty and a 0-dim parameter
    assert [r[3] // 4 for r in A.Layout(A.build("chunky", 1)).ranges] == [6000, 64, 40000]
    assert A.Layout(A.build("bf16", 1)).kind == "bf16" and A.Layout(A.build("mixed", 1)).kind == "mixed"
    for model in A.MODELS:
        assert 1024 <= A.Layout(A.build(model, 1)).nbytes <= 512 * 1024


def test_chunkys_trained_tensor_shares_a_chunk_with_an_untrained_one():
    """(See chunky_geometry: the 256-byte alignment puts the small tensor's first word on a chunk's
    boundary, so the chunk it shares is the one at its end, with the 40,000-element tensor.)"""
    chunk, (lo, hi), words, big = A.chunky_geometry()
    assert lo in words and hi - 1 == big and hi - lo == 3


# ---------------------------------------------------------------- FlatParameters.adopt
def test_adopt_takes_the_modules_new_parameters():
    net = A.build("chunky", 2)
    flat = FlatParameters(net.named_parameters())
    old = net.small
    net.small = torch.nn.Parameter(torch.full((64,), 7.0))
    assert flat.adopt(net.named_parameters()) == 1
    assert flat.params[1] is net.small and net.small.data_ptr() == flat.view("small").data_ptr()
    assert float(flat.view("small")[3]) == 7.0
    with torch.no_grad():
        old.add_(1.0)                        # the object left behind no longer writes the buffer
    assert float(flat.view("small")[3]) == 7.0 and flat.resync() == 0


def test_adopt_names_the_parameter_that_does_not_fit():
    net = A.build("chunky", 2)
    flat = FlatParameters(net.named_parameters())
    net.small = torch.nn.Parameter(torch.zeros(65))
    with pytest.raises(ValueError, match="'small'"):
        flat.adopt(net.named_parameters())
    net = A.build("odd", 2)
    flat = FlatParameters(net.named_parameters())
    A.load_sd_assign(net, flat, np.random.default_rng(0))        # unties t1 / t2: a seventh name
    with pytest.raises(ValueError, match="t2.weight"):
        flat.adopt(net.named_parameters())
