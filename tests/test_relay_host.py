"""The host model of the relay (tests/relay_ref.py) without a GPU: the stripe geometry of every size
the GPU test runs, that the copy16 edge points are reached, that no two ranks or rounds share a
factor, that the model agrees with itself (the gathered and the fused form see the same peer bytes)
and that the cases tests/test_gpu_relay.py runs tell every wrong kernel of RELAY_MUTANTS from it."""
import struct

import numpy as np
import pytest

from oracle import policy as opolicy
from tests import forms_ref as fref
from tests import moves_ref
from tests import relay_ref as ref
from tests.forms_ref import SIZE
from tests.test_forms_host import NAN_CAP


def layout(world, nbytes):
    stripe, p16 = ref.stripe_bytes(nbytes, world), ref.round16(nbytes)
    return stripe, [ref.stripe_len(s, stripe, p16) for s in range(world)]


# ---------------------------------------------------------------- geometry
def test_stripe_bytes_is_an_even_share_in_whole_pages():
    for world in range(2, 9):
        for nbytes in (4, 16, 20, 4096, 4100, 8188, 8192, 8196, 12324, 400_012, 262_148):
            stripe = ref.stripe_bytes(nbytes, world)
            assert stripe % ref.PAGE == 0 and stripe % ref.SPAN == 0
            assert stripe * world >= ref.round16(nbytes)                       # the stripes hold the payload
            assert (stripe - ref.PAGE) * world < ref.round16(nbytes)           # a page less would not
            lens = layout(world, nbytes)[1]
            assert sum(lens) == ref.round16(nbytes) and all(x % 16 == 0 for x in lens)
            assert all(b == 0 or a == stripe for a, b in zip(lens, lens[1:]))  # full, one partial, empty


def test_edge_sizes_have_the_layout_they_are_chosen_for():
    got = {(w, b): layout(w, b) for w, b in ref.EDGE_SIZES}
    assert got == {(2, 4100): (4096, [4096, 16]), (2, 8192): (4096, [4096, 4096]), (2, 8188): (4096, [4096, 4096]),
                   (3, 5124): (4096, [4096, 1040, 0]), (4, 12324): (4096, [4096, 4096, 4096, 48]),
                   (4, 12308): (4096, [4096, 4096, 4096, 32]), (4, 20): (4096, [32, 0, 0, 0]),
                   (3, 8196): (4096, [4096, 4096, 16])}
    # 4100 over two ranks: every whole item in stripe 0, the ragged tail alone in stripe 1
    assert 4100 // 16 * 16 == 4096 and all(4096 <= b < 4100 + 4096 for b in range(4096, 4100))
    for dtype in fref.DTYPES:
        assert (4100 - 4096) // SIZE[dtype] == {"f32": 1, "bf16": 2, "f16": 2}[dtype]
    # 8192: no tail, every span whole; 8188: a partial last span, the tail at the end of the last stripe
    assert 8192 % ref.SPAN == 0 and 8192 % 16 == 0
    assert 8188 // 16 * 16 % ref.SPAN != 0 and 8188 % 16 == 12 and ref.round16(8188) == 2 * 4096
    # 5124 over three: one full span and the tail's word in stripe 1, an empty stripe still relayed
    assert 5124 // 16 * 16 - 4096 == ref.SPAN and ref.round16(5124) - 5124 // 16 * 16 == 16
    # 8196 over three: the ragged tail alone in the stripe of a rank that is neither side of a pair
    assert 8196 // 16 * 16 == 2 * 4096
    # over four: 12308 leaves one whole item and the tail's word alone on the last rank (32 bytes),
    # 12324 two whole items and the tail's word (48 bytes)
    assert 12308 // 16 * 16 - 3 * 4096 == 16 and 12308 % 16 == 4
    assert 12324 // 16 * 16 - 3 * 4096 == 32 and 12324 % 16 == 4
    for w, b in ref.EDGE_SIZES:
        assert b % 4 == 0 and (b, ref.EDGE_BLOCKS) in ref.sizes(w)


def test_every_copy16_point_is_reached():
    """For both strides and every world the last non-empty stripe takes the four word counts at which
    copy16 changes its path; a right copy stores each of its words once and nothing behind them."""
    assert {p: (b + 4) // 16 for p, b in ref.relay_sizes(2, 1).items()} == {"4s-1": 2047, "4s": 2048, "4s+1": 2305,
                                                                              "7s+3": 3843}
    assert [ref.stripe_bytes(w * 16 - 4, 2) // 16 for w in (2047, 2305, 3843)] == [1024, 1280, 2048]
    assert [ref.last_stripe(2, w * 16 - 4)[1] for w in (2047, 2305, 3843)] == [1023, 1025, 1795]
    for world in ref.WORLDS:
        for blocks in ref.COPY16_BLOCKS:
            got = ref.relay_sizes(world, blocks)
            assert set(got) == set(ref.COPY16_POINTS), (world, blocks, got)
            for point, nbytes in got.items():
                stripe, lens = layout(world, nbytes)
                s, words = ref.last_stripe(world, nbytes)
                assert words == ref.copy16_words(point, blocks) and lens[s] == words * 16
                assert stripe // 16 - words < world * 256                    # within world x 256 words of full
                assert nbytes % 4 == 0 and nbytes % 16 == ref.TAIL_BYTES and (nbytes, blocks) in ref.sizes(world)
                for n16 in {x // 16 for x in lens}:
                    counts = ref.relay_counts(n16, blocks)
                    assert (counts[:n16] == 1).all() and not counts[n16:].any(), (world, blocks, point, n16)


def test_copy16_variants_go_wrong_at_the_points():
    for blocks in ref.COPY16_BLOCKS:
        for variant in ("no-remainder", "deep+1", "deep-first"):
            wrong = []
            for point in ref.COPY16_POINTS:
                n16 = ref.copy16_words(point, blocks)
                if not np.array_equal(ref.relay_counts(n16, blocks, variant), ref.relay_counts(n16, blocks)):
                    wrong.append(point)
            assert wrong, (blocks, variant)
    # first = blockIdx.y * 256 + lane over the workgroups is every lane of the stride once
    assert np.array_equal(ref.relay_counts(1025, 2), moves_ref.copy16_counts(1025, np.arange(512), 512))


# ---------------------------------------------------------------- topologies and factors
def test_pick_sequences_reach_what_they_are_chosen_for():
    for world, rounds in ref.PICKS.items():
        assert len(rounds) >= 3
        for picks in rounds:
            assert len(picks) == world and all(-1 <= p < world and p != r for r, p in enumerate(picks))
        unpicked_then_picked = any(r not in rounds[t] and r in rounds[t + 1]
                                   for t in range(len(rounds) - 1) for r in range(world))
        assert unpicked_then_picked, world                     # a stale relay stripe would be read
        assert any(-1 in picks for picks in rounds), world
    assert any(len(set(p)) < len(p) and -1 not in p for p in ref.PICKS[3])      # two ranks, one peer
    assert ref.PICKS[4][0] == (1, 2, 3, 0) and ref.PICKS[4][1] == (1, 0, 3, 2) and ref.PICKS[4][2] == (1, 0, 0, 0)
    assert ref.PICKS[3][0] == (1, 2, 0)


def test_no_two_ranks_or_rounds_share_a_factor():
    """Loss interpolation: the factor of (rank, round) with the header of ANY rank of either this
    round or the one before (the other slot) differs from every other, so a header taken from the
    wrong rank or slot shows in the factor, the clock and every averaged element."""
    for world, rounds in ref.PICKS.items():
        right = {}
        for t, picks in enumerate(rounds):
            for r, pick in enumerate(picks):
                if pick < 0:
                    continue
                f = {(q, u): opolicy.interpolation("loss", None, 0.0, 0.0, ref.loss_of(r, t), ref.loss_of(q, u))
                     for q in range(world) for u in (t - 1, t) if u >= 0}
                assert len(set(f.values())) == len(f), (world, t, r)
                assert all(0.0 < x < 1.0 for x in f.values())
                right[(r, t)] = f[(pick, t)]
        assert len(set(right.values())) == len(right), world
    losses = [ref.loss_of(r, t) for r in range(4) for t in range(4)]
    assert len(set(losses)) == len(losses) and all(x + ref.SECOND_LOSS not in losses for x in losses)


def test_payloads_differ_between_ranks_rounds_and_forms():
    for dtype in fref.DTYPES:
        seen = set()
        for form in ref.FORMS:
            for t in range(4):
                for r in range(4):
                    assert fref.hard_phase(ref.seed_of(form, r, t)) == fref.hard_phase(ref.seed_of(form, 0, 0))
                    seen.add(ref.payload_of(dtype, 8188, form, r, t)[1].tobytes())
        assert len(seen) == len(ref.FORMS) * 16
        # the tail of the copy16 payloads has an element that forms_ref.sample does not pin
        n = (2047 * 16 - 4) // SIZE[dtype]
        free = n // fref.PER[dtype] * fref.PER[dtype]
        assert n - free >= 3 and len({int(ref.payload_of(dtype, n * SIZE[dtype], "fused", r, 0)[0][free])
                                      for r in range(4)}) > 1


# ---------------------------------------------------------------- the model with itself
def observations(world, nbytes, dtype, blocks, forms, mutant=None):
    """{(set, form, round, rank): Seen}"""
    job = ref.Job(world, nbytes, dtype, blocks, forms, mutant)
    return {(i, form, t, s.rank): s for i, fs in enumerate(job.learner_sets())
            for form, t, picks, version, seen in job.rounds(fs) for s in seen}


@pytest.mark.parametrize("world", ref.WORLDS)
def test_model_is_self_consistent(world):
    """On every case: the gathered form stages the pick's header and payload and leaves the bytes
    behind round16(payload) alone; the fused form reads the same bytes, every one once; a rank
    without a pick sees nothing and keeps its clock; the factor and clock are the policy's."""
    for nbytes, blocks, dtype in ref.cases(world):
        obs = observations(world, nbytes, dtype, blocks, ref.FORMS)
        assert len(obs) == len(ref.FORMS) * len(ref.PICKS[world]) * world
        versions = {form: set() for form in ref.FORMS}
        for (_, form, t, r), s in obs.items():
            what = (world, nbytes, dtype, blocks, form, t, r)
            versions[form].add((s.version - 1) % 2)
            if form in ref.GATHERS:
                assert (s.staging[ref.PAYLOAD_OFF + ref.round16(nbytes):] == ref.SENTINEL).all(), what
                assert (s.staging[ref.HEADER:ref.PAYLOAD_OFF] == ref.SENTINEL).all(), what
            if s.pick < 0:
                assert s.peer is None and s.factor is None and s.clock_after == s.clock_before, what
                assert s.staging is None or (s.staging == ref.SENTINEL).all(), what
                continue
            theirs = obs[(_, form, t, s.pick)]
            assert np.array_equal(s.peer, theirs.published), what
            assert np.array_equal(s.peer_header[:ref.HEADER_FIELDS], theirs.header), what
            assert s.visits is None or (s.visits == 1).all(), what
            if form == "copy":
                assert s.factor is None and s.clock_after == s.clock_before, what
            else:
                want = opolicy.factor_and_clock("loss", None, 0.0, s.clock_before, theirs.clock_before, s.loss,
                                                theirs.loss)
                assert (s.factor, s.clock_after) == want and 0.0 < s.factor < 1.0, what
        for form in ref.FORMS:                                     # both slots serve every form
            assert versions[form] == {0, 1}, (world, nbytes, form, versions[form])


@pytest.mark.parametrize("dtype", fref.DTYPES)
def test_expected_averages_are_mostly_comparable(dtype):
    """NaNs are exempt from bit comparison: they stay under the cap of tests/test_forms_host.py."""
    worst = 0.0
    for world in ref.WORLDS:
        for nbytes, blocks in ref.sizes(world):
            for form in ("gather", "resident"):
                for t, picks in enumerate(ref.PICKS[world]):
                    for r, pick in enumerate(picks):
                        if pick < 0:
                            continue
                        f = opolicy.interpolation("loss", None, 0.0, 0.0, ref.loss_of(r, t), ref.loss_of(pick, t))
                        peer = ref.payload_of(dtype, nbytes, form, pick, t)[1]
                        share = fref.nan_share(dtype, ref.averaged(dtype, nbytes, form, r, t, f, peer))
                        assert share <= NAN_CAP, (world, nbytes, form, t, r, share)
                        worst = max(worst, share)
    print("largest NaN share, %s: %.4f" % (dtype, worst))


# ---------------------------------------------------------------- mutants
def first_difference(mutant):
    """The first case of the GPU test's set on which the mutant's observations differ from the
    model's: (world, payload bytes, blocks, dtype, form, round, rank), or None."""
    for world in ref.WORLDS:
        for nbytes, blocks, dtype in ref.cases(world):
            if dtype == "bf16":       # the model's bytes do not depend on which 16-bit type
                continue
            right = observations(world, nbytes, dtype, blocks, ("gather", "fused"))
            wrong = observations(world, nbytes, dtype, blocks, ("gather", "fused"), mutant)
            for key, s in right.items():
                if s.observation() != wrong[key].observation():
                    return (world, nbytes, blocks, dtype) + key[1:]
    return None


@pytest.mark.parametrize("mutant", ref.RELAY_MUTANTS)
def test_the_cases_tell_every_mutant_from_the_model(mutant):
    found = first_difference(mutant)
    assert found is not None, mutant
    print("%s: first told apart at %r" % (mutant, found))


def test_mutants_that_need_a_particular_case_find_it():
    """The wrong kernels that only some cases can show are shown by the case chosen for them."""
    def differs(mutant, world, nbytes, blocks, form, dtype="f32"):
        right = observations(world, nbytes, dtype, blocks, (form,))
        wrong = observations(world, nbytes, dtype, blocks, (form,), mutant)
        return [k[1:] for k, s in right.items() if s.observation() != wrong[k].observation()]
    # the tail alone in a stripe a third rank holds: 8196 over three, in round 1 rank 1 averages with
    # rank 0 and reads the tail's word (stripe 2) from rank 2's relay buffer
    assert ref.PICKS[3][1][1] == 0 and ("fused", 1, 1) in differs("tail-from-last-item", 3, 8196, ref.EDGE_BLOCKS,
                                                                  "fused")
    assert differs("payload-floor16", 3, 5124, ref.EDGE_BLOCKS, "gather")
    assert differs("len-unclamped", 2, 4100, ref.EDGE_BLOCKS, "gather")
    # a rank nobody needed in the round before
    assert ("fused", 1, 0) in differs("active-others-only", 2, 8192, ref.EDGE_BLOCKS, "fused")
    assert differs("active-own-only", 3, 5124, ref.EDGE_BLOCKS, "gather")
    assert differs("span-swapped", 2, 8188, ref.EDGE_BLOCKS, "fused")
    for blocks in ref.COPY16_BLOCKS:
        for world in ref.WORLDS:
            sizes = ref.relay_sizes(world, blocks)
            assert differs("copy16-no-remainder", world, sizes["4s+1"], blocks, "gather")
            assert differs("copy16-deep+1", world, sizes["4s-1"], blocks, "gather")     # a load AT the bound
            assert differs("copy16-deep+1", world, sizes["7s+3"], blocks, "gather")
            assert differs("copy16-deep-first", world, sizes["4s-1"], blocks, "gather")


def test_header_fields_are_the_library_struct():
    h = ref.header_bytes(2.5, 0.75, 7, 1025, "bf16")
    assert h.size == ref.HEADER_FIELDS
    assert struct.unpack("<ddQqi", h.tobytes()[:36]) == (2.5, 0.75, 7, 1025, fref.CODE["bf16"])
