"""Without a GPU: the conditions under which tests/test_gpu_group_dtypes.py may compare float16 and
mixed-dtype models through the multi-process groups with plain bit equality, for exactly the cases it runs
(tests/group_ref.py CASES), and that those cases tell every wrong implementation of group_ref.MUTANTS from
the reference."""
import numpy as np
import pytest

from tests import group_ref as ref
from tests import mixed_ref

LOCKSTEP = ref.lockstep_cases()
IDS = ["%s-%s-%d" % (c.job, c.kind, c.world) for c in LOCKSTEP]


def test_the_sizes_are_the_ones_the_stripe_conditions_were_worked_out_for():
    assert ref.nbytes("f16") == 20_486 and ref.nbytes("f16") % 16 == 6
    segs, total = ref.segments("mixed")
    assert [(d, off, length) for d, off, length, _ in segs] == [("f32", 0, 12288), ("bf16", 12288, 8192),
                                                                ("f16", 20480, 8192)] and total == 28_672
    assert [e - b for b, e in ref.stripes("f16", 3)] == [8192, 8192, 4112]


def test_only_listed_cases_are_handed_out():
    assert ref.case("walk", "f16", 2) is ref.CASES[("walk", "f16", 2)]
    for bad in (("walk", "f16", 4), ("walk", "mixed", 2), ("board", "mixed", 3), ("resident", "f16", 2)):
        with pytest.raises(AssertionError):
            ref.case(*bad)
    # what the GPU file runs: the walk, resident, fd-shared and board jobs of the issue
    assert sorted(ref.CASES) == sorted([("walk", "f16", 2), ("walk", "f16", 3), ("walk", "mixed", 3),
                                        ("walk", "mixed", 4), ("resident", "f16", 3), ("resident", "mixed", 3),
                                        ("vmm", "mixed", 3), ("board", "f16", 3), ("board", "mixed", 2)])
    assert [p for p, _ in ref.PHASES["f16"]] == ["copy", "kernel:64", "relay:8", "relay-avg:8"]
    assert [p for p, _ in ref.PHASES["mixed"]] == ["copy", "kernel:64", "relay:8"]
    for c in ref.CASES.values():
        assert c.world <= 4
        if c.job == "walk":
            assert c.phases == ref.PHASES[c.kind] and all(k == 4 for _, k in c.phases)
        if c.job in ref.LOCKSTEP:
            assert c.fp == 0.8
    assert ref.case("resident", "f16", 3).phases == (("relay-avg:8", 8),)
    assert ref.case("resident", "mixed", 3).phases == (("relay:8", 8),)
    assert ref.case("vmm", "mixed", 3).phases == (("copy", 4), ("relay:8", 4))
    assert ref.case("board", "f16", 3).phases == (("kernel:64", 16),)
    assert ref.case("board", "mixed", 2).phases == (("copy", 16),)


# ---------------------------------------------------------------- conditions, not tolerances
@pytest.mark.parametrize("c", LOCKSTEP, ids=IDS)
def test_the_reference_alone_allows_plain_bit_equality(c):
    """No expected round of any rank holds a NaN or an inf; every (rank, phase) has an averaged round;
    the job has a round without a fetch."""
    exp = ref.reference(c)
    init, deltas, _, _ = ref.case_inputs(c)
    assert ref.finite(c.kind, init) and ref.finite(c.kind, deltas)
    assert ref.finite(c.kind, exp["params"])
    if c.job == "resident":      # the parameters a resident round publishes: the average plus the step
        step = ref.add(c.kind)
        for r in range(ref.rounds(c)):
            for g in range(c.world):
                assert ref.finite(c.kind, step(exp["params"][r, g], deltas[r, g]))
    averaged = exp["averaged"]
    for g in range(c.world):
        for i in range(len(c.phases)):
            rs = [r for r in range(ref.rounds(c)) if ref.phase_of(c, r) == i]
            assert averaged[rs, g].any(), "rank %d never averages in phase %d (%s)" % (g, i, c.phases[i][0])
            assert len(rs) == c.phases[i][1]
    assert not exp["fetching"].all(), "every rank fetches in every round"
    assert np.array_equal(exp["fetching"], averaged)      # lock-step: a granted fetch always delivers


@pytest.mark.parametrize("c", LOCKSTEP, ids=IDS)
def test_the_restated_rounds_are_simulates(c):
    """group_ref.trajectory (the loop the mutants are planted in) with no mutant is oracle.gossip.simulate's
    trajectory: parameters, clocks and peers."""
    exp, got = ref.reference(c), ref.trajectory(c)
    assert ref.differing(c, got) == []
    assert np.array_equal(_bytes(got["params"]), _bytes(exp["params"]))
    assert np.array_equal(got["clocks"], exp["clocks"])
    assert got["peers"] == exp["peers"]


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("c", LOCKSTEP, ids=IDS)
def test_hard_values_sit_at_segment_ends_and_stripe_borders(c):
    init, deltas, _, _ = ref.case_inputs(c)
    segs, _ = ref.segments(c.kind)
    ranges = ref.hard_ranges(c.kind, c.world)
    for i, seg in enumerate(segs):
        d, off, _, n = seg
        size = mixed_ref.SIZE[d]
        mine = [(lo, k) for j, lo, k in ranges if j == i]
        assert mine[0][0] == 0 and mine[-1][0] + mine[-1][1] == n
        hard = set(mixed_ref.HARD[d][:ref.HARD_FINITE].tolist())
        for payload in list(init) + [deltas[r, g] for r in range(deltas.shape[0]) for g in range(c.world)]:
            e = mixed_ref.elements(_bytes(payload), seg)
            for lo, k in mine:
                assert set(e[lo:lo + k].tolist()) <= hard
        for b in ref.borders(c.kind, c.world):         # an element on either side of every border inside it
            if off < b < off + n * size:
                lo = (b - off) // size
                assert any(a <= lo - 1 < a + k for a, k in mine) and any(a <= lo < a + k for a, k in mine)
    # the padding of every mixed payload is zero
    if c.kind == "mixed":
        for d, off, length, n in segs:
            assert not _bytes(init)[:, off + n * mixed_ref.SIZE[d]:off + length].any()
            assert not _bytes(deltas)[:, :, off + n * mixed_ref.SIZE[d]:off + length].any()


@pytest.mark.parametrize("kind,world", [("f16", 3), ("mixed", 2)])
def test_the_board_bases_cannot_overflow(kind, world):
    """Every published base is finite and below half the smallest format's largest finite value, and the
    board's factors lie in [0, 1] (clock interpolation, no threshold): no average is a NaN or an inf."""
    c = ref.case("board", kind, world)
    assert c.interp == "clock" and c.thr == 0.0 and c.fp == 1.0 and ref.rounds(c) == 16
    n = ref.N_F16 if kind == "f16" else ref.nbytes(kind)
    fn = ref.base(kind)
    for g in range(world):
        for r in range(-1, ref.rounds(c)):
            b = fn(g, r, n)
            assert ref.finite(kind, b)
            for seg in ref.segments(kind)[0]:
                e = mixed_ref.elements(_bytes(b), seg)
                v = {"f32": lambda u: u.view(np.float32), "bf16": lambda u: (u.astype(np.uint32) << 16).view(np.float32),
                     "f16": lambda u: u.view(np.float16).astype(np.float32)}[seg[0]](e)
                assert np.abs(v).max() < 32752.0
    # a base is not its neighbour's: a reader of the wrong version cannot pass
    assert ref.same(kind, fn(0, 0, n), fn(0, 1, n)) is not None
    assert ref.same(kind, fn(0, 0, n), fn(1, 0, n)) is not None


# ---------------------------------------------------------------- the stripe conditions
def _inside(kind, b):
    return any(off < b < off + length for _, off, length, _ in ref.segments(kind)[0])


def _on(kind, b):
    return any(b == off for _, off, _, _ in ref.segments(kind)[0][1:])


def test_stripe_borders_of_the_mixed_layout():
    for world in (2, 3, 4):
        assert any(_inside("mixed", b) for b in ref.borders("mixed", world)), world
    assert any(_on("mixed", b) for world in (3, 4) for b in ref.borders("mixed", world))
    lens = [e - b for b, e in ref.stripes("mixed", 4)]
    assert 0 < lens[-1] < min(lens[:-1]), lens
    # what they are, so that a change of the arithmetic shows
    assert ref.borders("mixed", 2) == [16384]
    assert ref.borders("mixed", 3) == [12288, 24576]
    assert ref.borders("mixed", 4) == [8192, 16384, 24576]
    # every border inside a segment has elements (not padding alone) behind it
    for world in (2, 3, 4):
        for b in ref.borders("mixed", world):
            if _inside("mixed", b):
                assert any(off < b < off + n * mixed_ref.SIZE[d] for d, off, _, n in ref.segments("mixed")[0]), (world, b)


def test_the_last_f16_stripe_ends_inside_a_word():
    b, e = ref.stripes("f16", 3)[-1]
    assert b < ref.nbytes("f16") < e and e - ref.nbytes("f16") == 10 and ref.nbytes("f16") % 16 == 6
    assert [x - y for y, x in ref.stripes("f16", 2)] == [12288, 8208]


# ---------------------------------------------------------------- the mutants
@pytest.mark.parametrize("mutant", ref.MUTANTS, ids=[m.name for m in ref.MUTANTS])
def test_every_mutant_differs_in_a_round_the_gpu_test_compares(mutant):
    """The GPU test compares every (rank, round) of every lock-step case; a mutant must differ from the
    reference in at least one of them, in every case that runs the code it breaks -- and each kind has
    such a case."""
    kinds = set()
    for c in LOCKSTEP:
        if not mutant.applies(c):
            continue
        bad = ref.differing(c, ref.trajectory(c, mutant))
        print("%s: %s-%s-%d: %d of %d (rank, round) pairs differ" % (mutant.name, c.job, c.kind, c.world, len(bad),
                                                                     c.world * ref.rounds(c)))
        assert bad, (mutant.name, c)
        kinds.add(c.kind)
    want = {"bf16-segment-as-f16": {"mixed"}, "tail-not-moved": {"f16"}}.get(mutant.name, set(ref.KINDS))
    assert kinds == want, (mutant.name, kinds)


def test_the_mutants_are_the_listed_ones():
    assert [m.name for m in ref.MUTANTS] == ["bf16-segment-as-f16", "f16-as-bf16", "f16-one-rounding", "stale-stripe",
                                             "zero-stripe", "short-last-stripe", "snapshot-after-step", "tail-not-moved"]


# ---------------------------------------------------------------- the float16 training step
def test_the_f16_step_is_numpys_float16_add():
    for c in LOCKSTEP:
        if c.kind != "f16":
            continue
        init, deltas, _, _ = ref.case_inputs(c)
        exp = ref.reference(c)["params"]
        step = ref.add("f16")
        for r in range(ref.rounds(c)):
            for g in range(c.world):
                for p in (init[g], exp[r, g]):
                    want = (p.view(np.float16) + deltas[r, g].view(np.float16)).view(np.uint16)
                    assert np.array_equal(step(p, deltas[r, g]), want), (c, r, g)


# ---------------------------------------------------------------- refusals that need no device
def test_the_refused_layouts_have_equal_bytes_and_other_digests():
    from dpwa_amd.flat import layout_digest
    (a, total_a), (b, total_b) = (ref.layout_of(s) for s in ref.REFUSED_LAYOUTS)
    assert total_a == total_b == 16384
    assert ref.fnv_digest(a) != ref.fnv_digest(b)
    for lay in (a, b, ref.layout("mixed")):
        assert ref.fnv_digest(lay) == layout_digest(tuple((mixed_ref.TORCH[d], off, n) for d, off, n in lay))


def test_relay_avg_is_refused_for_the_mixed_layout(tmp_path):
    from dpwa_amd import DpwaConnection
    from dpwa_amd.dpwa import MIXED_RELAY_AVG
    from dpwa_amd.group import LocalGroup
    from dpwa_amd.launch import write_config
    cfg = write_config(str(tmp_path / "m.yaml"), ["a", "b"], interpolation="constant")
    lay = tuple((mixed_ref.TORCH[d], off, n) for d, off, n in ref.layout("mixed"))
    for pull in ("relay-avg", "relay-avg:8"):
        with pytest.raises(ValueError) as err:
            DpwaConnection("a", cfg, seed=1, group=LocalGroup(), pull=pull, layout=lay)
        assert str(err.value) == MIXED_RELAY_AVG
    conn = DpwaConnection("a", cfg, seed=1, group=LocalGroup(), pull="relay:8", layout=lay)
    try:
        with pytest.raises(ValueError) as err:
            conn.set_pull("relay-avg:8")
        assert str(err.value) == MIXED_RELAY_AVG
        assert conn._pull == "relay:8"                      # the refused call changed nothing
        # the walk's first switch comes before the bind: the relay buffers are still asked for then
        conn.set_pull("copy")
        assert conn._pull == "copy" and conn._relay_created
    finally:
        conn.close()
    from dpwa_amd.group import AsyncDistGroup, DistGroup
    assert DistGroup.relay_capable and not AsyncDistGroup.relay_capable and not hasattr(LocalGroup, "relay_capable")
