"""Host side (no GPU) of tests/test_gpu_moves.py: the byte-moving kernels' model (tests/moves_ref.py)
has teeth at the sizes, generations and write sets the GPU tests use.

(a) Coverage: for every size and generation the GPU tests run, the write sets hold a case the model
    detects and, from 8191 words on (every chunk two words and more), one it must NOT detect -- so no
    GPU case has to be skipped for want of a distinguishing input.
(b) Mutants: every plausible wrong kernel restated in moves_ref (guard_mutant, window_expected's
    variants, copy16_counts' variants) disagrees with the model on at least one of those inputs.
"""
import numpy as np
import pytest

from dpwa_amd import _lib
from tests import moves_ref as ref
from tests.helpers import GUARD_SAMPLES, guard_chunk, guard_words


def payload(nbytes, seed=0):
    """Cheap, non-repeating bytes (the GPU tests use forms_ref.operands; the model only compares)."""
    return np.random.default_rng([nbytes, seed]).integers(0, 256, nbytes, dtype=np.uint8)


def guard_inputs():
    """(n16, tail, gen, case, words) of every guarded publish of the GPU tests but the large one."""
    for n16 in sorted(set(ref.GUARD_N16 + ref.GUARD_BYTES_N16)):
        for tail in ref.GUARD_TAILS:
            for shift in range(3):                               # one per dtype
                for gen, name, words in ref.guard_schedule(n16, tail, shift):
                    yield n16, tail, gen, name, words


def window_inputs():
    for n16 in ref.WINDOW_N16:
        for tail in ref.GUARD_TAILS:
            for shift in ref.WINDOW_SHIFTS:
                for gen, name, words in ref.window_schedule(n16, tail, shift):
                    yield n16, tail, gen, name, words


# ---------------------------------------------------------------- the geometry the model stands on
def test_constants_are_the_librarys():
    assert ref.SLOT_PAYLOAD_OFFSET == _lib.SLOT_PAYLOAD_OFFSET and ref.HEADER_WORDS == 256
    assert GUARD_SAMPLES == 4096


@pytest.mark.parametrize("n16", sorted(set(ref.GUARD_N16)) + [ref.GUARD_BIG_N16])
def test_chunk_bounds_are_helpers_chunks(n16):
    s = ref.samples_of(n16)
    for k in sorted({0, 1, 15, 16, 17, (s - 1) // 2, s - 2, s - 1} & set(range(s))):
        lo, hi = ref.chunk_bounds(n16, k)
        assert guard_chunk(n16, lo) == (k, (lo, hi)) and guard_chunk(n16, hi - 1) == (k, (lo, hi))
        for gen in (0, 2, 3, 6, 11):
            assert ref.chunk_sample(n16, k, gen) in guard_words(n16, gen)
    assert ref.chunk_bounds(n16, s - 1) == (n16 - 1, n16)
    # 8191 words: every chunk but the last holds two; 16 * 4095 + 1: sixteen; the large size: 1025
    if n16 in (8191, 16 * 4095 + 1, ref.GUARD_BIG_N16):
        want = (n16 - 1) // 4095
        assert all(ref.chunk_bounds(n16, k)[1] - ref.chunk_bounds(n16, k)[0] == want for k in range(0, s - 1, 97))


def test_write_sets_hold_the_cases():
    """Word 0, the last word, a middle chunk's sampled and an unsampled word, both of its end words,
    chunks 15 and 16 together, two chunks of one workgroup, a tail byte alone, nothing."""
    n16, gen = 16 * 4095 + 1, 5
    sets = ref.write_sets(n16, gen, tail=4)
    words = guard_words(n16, gen)
    assert sets["nothing"] == () and sets["word0"] == (0,) and sets["last"] == (n16 - 1,)
    assert sets["tail"] == (ref.tail_word(n16),)
    k, (lo, hi) = guard_chunk(n16, sets["mid-sampled"][0])
    assert 16 < k < 4000 and sets["mid-sampled"][0] in words
    assert guard_chunk(n16, sets["mid-unsampled"][0])[0] == k and sets["mid-unsampled"][0] not in words
    assert sets["chunk-ends"] == (lo, hi - 1)
    assert sets["neighbours"] == (lo - 1, sets["mid-sampled"][0], hi)
    assert [guard_chunk(n16, w)[0] for w in sets["chunks-15-16"]] == [15, 16]
    a, b = (guard_chunk(n16, w)[0] for w in sets["two-in-workgroup"])
    assert a != b and a // 16 == b // 16 == k // 16
    assert all(w in words for w in sets["chunks-15-16"] + sets["two-in-workgroup"])
    assert len(sets["all"]) == n16 + 1
    # the names are the same at every generation (the schedules rotate them by index)
    assert list(sets) == list(ref.write_sets(n16, gen + 1, tail=4))
    assert "tail" not in ref.write_sets(n16, gen, tail=0)
    assert set(ref.write_sets(1, gen, tail=4)) == {"nothing", "word0", "tail", "all"}


def test_written_changes_exactly_the_words_asked_for():
    n16, gen = 8191, 3
    base = payload(n16 * 16 + 4)
    for name, words in ref.write_sets(n16, gen, tail=4).items():
        got = ref.written(base, words, gen)
        changed = set(ref._differing_words(base, got, n16).tolist())
        if (got[n16 * 16:] != base[n16 * 16:]).any():
            changed.add(ref.tail_word(n16))
        assert changed == set(words), name


# ---------------------------------------------------------------- the model itself
def test_guard_expected_on_a_hand_made_case():
    """17 words (every word its own chunk) and 3 tail bytes, generation 4: a write to word 5 and to
    a tail byte -- word 5 and that byte are taken, nothing else; nothing written: no hit."""
    n16, tail, gen = 17, 3, 4
    snap = payload(n16 * 16 + tail)
    flat = snap.copy()
    flat[5 * 16 + 9] ^= 1
    flat[n16 * 16 + 1] ^= 1
    got, hit = ref.guard_expected(snap, flat, gen)
    assert hit and np.array_equal(got, flat)
    assert ref.guard_expected(snap.tobytes(), snap.tobytes(), gen)[1] is False
    # two-word chunks: a write beside the sampled word stays out, one at it brings its neighbour along
    n16 = 8191
    snap = payload(n16 * 16)
    k = 2000
    lo, hi = ref.chunk_bounds(n16, k)
    assert (lo, hi) == (4000, 4002) and ref.chunk_sample(n16, k, 3) == 4001
    flat = snap.copy()
    flat[4000 * 16] ^= 1
    got, hit = ref.guard_expected(snap, flat, 3)
    assert not hit and np.array_equal(got, snap)
    flat[4001 * 16] ^= 1
    flat[4002 * 16] ^= 1                                        # the next chunk's unsampled word
    got, hit = ref.guard_expected(snap, flat, 3)
    want = snap.copy()
    want[4000 * 16:4002 * 16] = flat[4000 * 16:4002 * 16]
    assert hit and np.array_equal(got, want)


def test_window_expected_on_hand_made_cases():
    n16, gen = 8191, 3
    pub = payload(n16 * 16 + 4)
    for word, want in ((0, True), (n16 - 1, True), (4001, True), (4000, False), (ref.tail_word(n16), True)):
        assert ref.window_expected(pub, ref.written(pub, (word,), gen), gen) is want, word
    assert ref.window_expected(pub, pub, gen) is False
    assert ref.window_expected(pub[:5], ref.written(pub[:5], (0,), gen), gen) is True      # tail bytes only


# ---------------------------------------------------------------- (a) coverage
def test_every_guard_size_and_generation_has_a_detected_and_an_undetected_case():
    seen = set()
    for n16 in sorted(set(ref.GUARD_N16 + ref.GUARD_BYTES_N16)):
        for tail in ref.GUARD_TAILS:
            snap = payload(n16 * 16 + tail)
            gens = {g for shift in range(3) for g, _, _ in ref.guard_schedule(n16, tail, shift)}
            assert set(range(2, 7)) <= gens
            for gen in sorted(gens):
                hits = {name: ref.guard_expected(snap, ref.written(snap, words, gen), gen)[1]
                        for name, words in ref.write_sets(n16, gen, tail).items()}
                assert any(hits.values()), (n16, tail, gen)
                assert not hits["nothing"]
                if n16 >= 8191:
                    assert not hits["mid-unsampled"], (n16, tail, gen)
                seen.add((n16, tail, gen))
    assert len(seen) >= 5 * len(ref.GUARD_N16) * len(ref.GUARD_TAILS)


def test_every_schedule_writes_every_case_once():
    for n16 in ref.GUARD_N16:
        for tail in ref.GUARD_TAILS:
            for shift in range(3):
                names = [name for _, name, _ in ref.guard_schedule(n16, tail, shift)]
                assert set(names) == set(ref.write_sets(n16, 2, tail)), (n16, tail, shift)
    for n16 in ref.WINDOW_N16:
        for tail in ref.GUARD_TAILS:
            names = {name for shift in ref.WINDOW_SHIFTS for _, name, _ in ref.window_schedule(n16, tail, shift)}
            assert names == set(ref.write_sets(n16, 1, tail)), (n16, tail)


def test_every_window_size_and_generation_has_a_detected_and_an_undetected_case():
    for n16 in ref.WINDOW_N16:
        for tail in ref.GUARD_TAILS:
            pub = payload(n16 * 16 + tail)
            for gen in ref.WINDOW_GENS:
                hits = {name: ref.window_expected(pub, ref.written(pub, words, gen), gen)
                        for name, words in ref.write_sets(n16, gen, tail).items()}
                assert any(hits.values()) and not hits["nothing"], (n16, tail, gen)
                if n16 >= 8191:
                    assert not hits["mid-unsampled"], (n16, tail, gen)
    # and among the windows the GPU test really opens (one case each), both outcomes occur at 8191 words
    got = {ref.window_expected(p, ref.written(p, words, gen), gen)
           for n16, tail, gen, _, words in window_inputs() if n16 == 8191
           for p in [payload(n16 * 16 + tail)]}
    assert got == {True, False}


def test_the_large_case_copies_the_middle_chunk_alone():
    n16, gen = ref.GUARD_BIG_N16, ref.GUARD_FIRST_GEN
    k, words = ref.big_guard_case(gen)
    lo, hi = ref.chunk_bounds(n16, k)
    assert hi - lo == 1025 and len(words) == 3 * 1025 - 2
    snap = np.arange(n16 * 4, dtype=np.uint32).view(np.uint8)
    flat = ref.written(snap, words, gen)
    got, hit = ref.guard_expected(snap, flat, gen)
    assert hit
    assert np.array_equal(got[lo * 16:hi * 16], flat[lo * 16:hi * 16])
    assert np.array_equal(got[:lo * 16], snap[:lo * 16]) and np.array_equal(got[hi * 16:], snap[hi * 16:])
    # the chunk copy runs copy16's four-deep loop in every lane and its remainder in one
    counts = ref.copy16_counts(hi, lo + np.arange(ref.GUARD_BLOCK), ref.GUARD_BLOCK)
    assert counts[lo:hi].tolist() == [1] * 1025 and counts[:lo].sum() == 0 and counts[hi:].sum() == 0
    for name in ("copy16-no-remainder", "copy16-deep-first", "hi+1", "hi-1"):
        assert not np.array_equal(ref.guard_mutant(name, snap, flat, gen)[0], got), name


# ---------------------------------------------------------------- (b) mutants
@pytest.mark.parametrize("name", [m for m in ref.GUARD_MUTANTS if not m.startswith("copy16")])
def test_guard_mutants_differ_on_the_gpu_tests_inputs(name):
    """Every wrong guard leaves other bytes, or another verdict, than the model for at least one
    (size, generation, write set) the GPU tests run.  (The copy16 mutants show at the large case
    only -- no other chunk is longer than 768 words -- which the test above covers.)"""
    caught = []
    for n16, tail, gen, case, words in guard_inputs():
        if case == "all" and n16 > 8191:
            continue                                             # (dense and long: nothing new, and slow)
        snap = payload(n16 * 16 + tail)
        flat = ref.written(snap, words, gen)
        want, hit = ref.guard_expected(snap, flat, gen)
        got, got_hit = ref.guard_mutant(name, snap, flat, gen)
        if got_hit != hit or not np.array_equal(got, want):
            caught.append((n16, tail, gen, case))
    print("%s: caught by %d inputs, e.g. %s" % (name, len(caught), caught[:3]))
    assert caught, name


@pytest.mark.parametrize("name", ref.WINDOW_MUTANTS)
def test_window_mutants_differ_on_the_gpu_tests_inputs(name):
    caught = []
    for n16, tail, gen, case, words in window_inputs():
        pub = payload(n16 * 16 + tail)
        now = ref.written(pub, words, gen)
        if ref.window_expected(pub, now, gen, name) != ref.window_expected(pub, now, gen):
            caught.append((n16, tail, gen, case))
    print("%s: caught by %d inputs, e.g. %s" % (name, len(caught), caught[:3]))
    assert caught, name


@pytest.mark.parametrize("max_blocks", ref.PULL_BLOCKS)
def test_pull_sizes_sit_at_copy16s_edges(max_blocks):
    """The model stores every word of the pulled slot once and none behind it; the sizes hit the
    points of pull_points with the stride the capped grid gives; each copy16 mutant stores otherwise
    at one of them at least."""
    pts = ref.pull_points(max_blocks)
    assert {name for name, _ in pts} == {"stride+1", "4s-1", "4s", "4s+1", "7s+3"}
    assert {g for _, g in pts} == {1, max_blocks}
    sizes = ref.pull_sizes(max_blocks)
    assert sorted({ref.pull_n16(b) for b in sizes}) == sorted(set(pts.values()))
    caught = {"no-remainder": [], "deep+1": [], "deep-first": []}
    for nbytes in sizes:
        n16 = ref.pull_n16(nbytes)
        stride = ref.pull_stride(n16, max_blocks)
        assert stride == min(max_blocks, -(-n16 // 1024)) * 256
        good = ref.pull_counts(nbytes, max_blocks)
        assert (good[:n16] == 1).all() and not good[n16:].any(), nbytes
        for name in caught:
            if not np.array_equal(ref.pull_counts(nbytes, max_blocks, name), good):
                caught[name].append(n16)
    assert all(caught.values()), caught
    # the remainder is needed exactly off the multiples of 4 * stride; `<=` overruns exactly where the
    # last four-deep load of some lane falls on n16
    for (name, g), n16 in pts.items():
        assert (n16 in caught["no-remainder"]) == (n16 in caught["deep-first"]) == (name != "4s"), (name, g)
        assert (n16 in caught["deep+1"]) == (name in ("4s-1", "7s+3")), (name, g)
