"""What the kernels that only move bytes must leave behind, restated on the host in plain numpy:
the model, the sizes and the cases shared by tests/test_moves_host.py (no GPU) and
tests/test_gpu_moves.py.  The kernels are k_publish (vector and byte forms), k_publish_header,
k_copy_payload, k_pull, k_guard_publish, k_guard_publish_bytes and k_window_roll of
dpwa_amd/csrc/kernels.hip.  Each has an exact reference -- a byte copy, plus the guard's chunk
geometry already restated in tests/helpers.py (guard_words, guard_chunk) -- so the bar is byte
equality.

A written word is a 16-byte word of the payload with one byte changed (``write_offsets``); the
pseudo word ``n16`` (``tail_word``) stands for the tail bytes behind the last whole word.

The aligned guard (k_guard_publish) and its byte form (k_guard_publish_bytes) were read side by
side: both compare chunk k at guard_offset(k), both compare the first word at every publish and
report it as chunk 0, both copy the words [guard_base(k), guard_base(k+1)) of a differing chunk (the
last chunk: the last word alone), both compare and copy the tail bytes one by one in workgroup 0 and
both stamp the verdict word once per generation.  They differ in how the work is spread (16 chunks
per 256-lane workgroup with a ballot, against one chunk per lane) and in the copy (copy16 with
stride 256, against a byte loop), not in what they must leave behind, so ``guard_expected`` is one
model for both; the variants below (``GUARD_MUTANTS``) restate how either could go wrong.
"""
import functools

import numpy as np

from tests.helpers import GUARD_SAMPLES, guard_chunk, guard_words

WORD = 16
SLOT_PAYLOAD_OFFSET = 4096                  # include/dpwa_hip.h DPWA_SLOT_PAYLOAD_OFFSET
# A copying fetch moves the slot from its first byte: the header's 4 KiB and the payload rounded up
# to a whole word (learner.cpp dpwa_learner_fetch: kPayloadOff + round_up(payload_bytes, 16)).
HEADER_WORDS = SLOT_PAYLOAD_OFFSET // WORD
BLOCK = 256                                 # kBlock: lanes of a k_pull workgroup
GUARD_BLOCK = 256                           # kGuardBlock: lanes that copy a differing chunk
GUARD_CHUNKS_PER_BLOCK = 16                 # kGuardChunksPerBlock
FLIP = 0x5A                                 # a written byte is the old one xor this


# ---------------------------------------------------------------- copy16
def copy16_counts(n16, first, stride, variant=None):
    """How often copy16(dst, src, n16, first, stride) stores each word, for the lanes whose first
    word is `first` (an array): an array over [0, n16 + 4 * stride), so that a store past the end
    shows.  variant: None (kernels.hip), "no-remainder" (the one-at-a-time loop dropped), "deep+1"
    (the four-deep loop entered when its last load is AT n16: `<=` for `<`) or "deep-first" (entered
    whenever its first load is below n16: one four-deep step in place of the remainder)."""
    assert variant in (None, "no-remainder", "deep+1", "deep-first")
    first = np.asarray(first, dtype=np.int64)
    counts = np.zeros(n16 + 4 * stride, dtype=np.int64)
    i = first.copy()
    live = np.ones(i.shape, dtype=bool)
    while live.any():                                         # the four-deep loop
        last = i + 3 * stride
        live &= (last <= n16) if variant == "deep+1" else (i < n16) if variant == "deep-first" else (last < n16)
        for j in range(4):
            np.add.at(counts, i[live] + j * stride, 1)
        i = np.where(live, i + 4 * stride, i)
    if variant != "no-remainder":
        live = i < n16
        while live.any():
            np.add.at(counts, i[live], 1)
            i = np.where(live, i + stride, i)
            live = i < n16
    return counts


# ---------------------------------------------------------------- pull
PULL_BLOCKS = (1, 2, 512)                   # max_blocks of dpwa_learner_set_pull in the GPU test


def pull_n16(payload_bytes):
    """The words launch_pull is given for a payload."""
    return HEADER_WORDS + (payload_bytes + WORD - 1) // WORD


def pull_grid(n16, max_blocks):
    """launch_pull's grid: one workgroup per 1024 words, at least one, at most max_blocks."""
    return min(max_blocks, max(1, (n16 + 4 * BLOCK - 1) // (4 * BLOCK)))


def pull_stride(n16, max_blocks):
    return pull_grid(n16, max_blocks) * BLOCK


def pull_points(max_blocks):
    """{(point, workgroups): n16} -- the sizes at which copy16 changes its path under k_pull, each
    consistent with the grid launch_pull picks for it (stride = workgroups * 256):
    4 * stride - 1 (the four-deep loop's last load falls one word short for the last lane),
    4 * stride (one four-deep pass, no remainder), 4 * stride + 1 (one remainder word),
    7 * stride + 3 (one pass, then three remainder passes of which the last holds three lanes),
    for one workgroup and for the capped grid.  The last two need n16 > 1024 * workgroups, which only
    the cap allows.  "Below one stride" and "at one stride" cannot be reached through a learner: the
    4 KiB ahead of the payload are 256 words, one workgroup's whole stride, and a larger grid needs
    n16 > 1024 (workgroups - 1) >= its stride; the nearest size, one word more than a stride with one
    workgroup (a one-word payload), stands in for both."""
    pts = {("stride+1", 1): HEADER_WORDS + 1}
    for g in sorted({1, max_blocks}):
        s = g * BLOCK
        for name, n16 in (("4s-1", 4 * s - 1), ("4s", 4 * s), ("4s+1", 4 * s + 1), ("7s+3", 7 * s + 3)):
            if n16 > HEADER_WORDS and pull_stride(n16, max_blocks) == s:
                pts[(name, g)] = n16
    return pts


def pull_sizes(max_blocks):
    """Payload byte counts (multiples of 4, so every dtype holds them) that put the words launch_pull
    sees at pull_points(max_blocks).  Up to two workgroups the payload ends 12 bytes short of its last
    word (the pull rounds it up); the one-word payload is 4 bytes."""
    out = []
    for (name, g), n16 in pull_points(max_blocks).items():
        nbytes = (n16 - HEADER_WORDS) * WORD
        if g <= 2:
            nbytes -= 12
        assert nbytes > 0 and nbytes % 4 == 0 and pull_n16(nbytes) == n16
        out.append(nbytes)
    return sorted(set(out))


def pull_counts(payload_bytes, max_blocks, variant=None):
    """How often k_pull stores each word of the destination (copy16_counts over the whole grid)."""
    n16 = pull_n16(payload_bytes)
    stride = pull_stride(n16, max_blocks)
    return copy16_counts(n16, np.arange(stride), stride, variant)


# ---------------------------------------------------------------- guard geometry
def split(nbytes):
    """(n16, tail bytes) of a payload."""
    return nbytes // WORD, nbytes % WORD


def tail_word(n16):
    """The pseudo word that stands for the tail bytes in a write set."""
    return n16


@functools.lru_cache(maxsize=None)
def sampled(n16, gen):
    """helpers.guard_words as a sorted array (the first and the last word included)."""
    return np.array(sorted(guard_words(n16, gen)), dtype=np.int64)


def samples_of(n16):
    return min(n16, GUARD_SAMPLES)


def chunk_bounds(n16, k):
    """Words [lo, hi) of chunk k (helpers.guard_chunk's ranges, by chunk index)."""
    s = samples_of(n16)
    if s <= 1 or k >= s - 1:
        return max(0, n16 - 1), n16
    return k * (n16 - 1) // (s - 1), (k + 1) * (n16 - 1) // (s - 1)


def chunk_sample(n16, k, gen):
    """The word of chunk k that generation `gen` compares."""
    lo, hi = chunk_bounds(n16, k)
    return lo + gen % (hi - lo)


def write_offsets(words, nbytes, gen):
    """Byte offsets to change for a write set: one byte per word, at a position that moves with the
    word (so all four dwords of a word are hit across a set); for the tail the byte gen mod tail."""
    n16, tail = split(nbytes)
    out = []
    for w in words:
        if w == tail_word(n16):
            assert tail, "this payload has no tail bytes"
            out.append(n16 * WORD + gen % tail)
        else:
            assert 0 <= w < n16
            out.append(w * WORD + (w * 7 + gen) % WORD)
    return np.array(sorted(set(out)), dtype=np.int64)


def written(buf, words, gen):
    """A copy of the uint8 array `buf` with the write set applied."""
    out = np.array(buf, dtype=np.uint8)
    at = write_offsets(words, out.size, gen)
    out[at] ^= FLIP
    return out


def write_sets(n16, gen, tail=0):
    """{case: words to write} for a payload of n16 words and `tail` tail bytes at generation `gen`.
    The names do not depend on `gen`; the words do (what is sampled moves).  Together:
      nothing            no write
      word0              the first word (compared at every publish, reported as chunk 0)
      last               the last word (the last chunk, alone)
      mid-sampled        the sampled word of a middle chunk
      mid-unsampled      an unsampled word of that chunk (chunks of two words and more)
      chunk-ends         both end words of that chunk, b(k) and b(k+1) - 1
      neighbours         its sampled word and the words just outside it, b(k) - 1 and b(k+1)
      chunks-15-16       the sampled words of chunks 15 and 16: the last chunk of one workgroup of
                         k_guard_publish and the first of the next
      two-in-workgroup   the sampled words of two chunks of the middle chunk's workgroup
      tail               a tail byte alone (payloads with tail bytes)
      all                every word, and a tail byte
    Cases a size has no room for are left out (a one-word payload has no middle chunk)."""
    s = samples_of(n16)
    sets = {"nothing": ()}
    if n16 >= 1:
        sets["word0"] = (0,)
    if n16 >= 2:
        sets["last"] = (n16 - 1,)
    if s >= 3:
        k = (s - 1) // 2
        lo, hi = chunk_bounds(n16, k)
        hit = chunk_sample(n16, k, gen)
        sets["mid-sampled"] = (hit,)
        if hi - lo >= 2:
            sets["mid-unsampled"] = (lo + (gen + 1) % (hi - lo),)
        sets["chunk-ends"] = tuple(sorted({lo, hi - 1}))
        sets["neighbours"] = tuple(sorted({lo - 1, hit, hi}))
        k0 = k // GUARD_CHUNKS_PER_BLOCK * GUARD_CHUNKS_PER_BLOCK
        pair = sorted({min(k0 + 1, s - 2), min(k0 + GUARD_CHUNKS_PER_BLOCK - 2, s - 2)})
        if len(pair) == 2:
            sets["two-in-workgroup"] = tuple(chunk_sample(n16, c, gen) for c in pair)
    if s >= GUARD_CHUNKS_PER_BLOCK + 1:
        sets["chunks-15-16"] = (chunk_sample(n16, GUARD_CHUNKS_PER_BLOCK - 1, gen),
                                chunk_sample(n16, GUARD_CHUNKS_PER_BLOCK, gen))
    if tail:
        sets["tail"] = (tail_word(n16),)
    if n16 >= 1:
        sets["all"] = tuple(range(n16)) + ((tail_word(n16),) if tail else ())
    return sets


# ---------------------------------------------------------------- the guard's model
GUARD_MUTANTS = ("hi+1", "hi-1", "no-first-word", "last-merged", "no-tail", "fixed-samples",
                 "copy16-no-remainder", "copy16-deep+1", "copy16-deep-first")


def _bytes(buf):
    a = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.asarray(buf)
    assert a.dtype == np.uint8 and a.ndim == 1
    return a


def _differing_words(a, b, n16):
    """Indices of the whole words at which two uint8 arrays differ."""
    if n16 == 0:
        return np.zeros(0, dtype=np.int64)
    x, y = np.ascontiguousarray(a[:n16 * WORD]), np.ascontiguousarray(b[:n16 * WORD])
    d = (x.view(np.uint64) != y.view(np.uint64)).reshape(n16, 2)
    return np.flatnonzero(d[:, 0] | d[:, 1])


def _compared(n16, gen, variant):
    """The words a publish of generation `gen` compares (sorted array)."""
    if n16 == 0:
        return np.zeros(0, dtype=np.int64)
    s = samples_of(n16)
    if variant == "fixed-samples":
        gen = 0
    words = set(sampled(n16, gen).tolist())
    if variant == "no-first-word" and s > 1 and chunk_sample(n16, 0, gen) != 0:
        words.discard(0)
    if variant == "last-merged" and s > 1:
        lo = chunk_bounds(n16, s - 2)[0]
        words -= {n16 - 1, chunk_sample(n16, s - 2, gen)}
        words |= {0, lo + gen % (n16 - lo)}
    return np.array(sorted(words), dtype=np.int64)


def _chunk_of(n16, word, variant):
    """Word range copied when `word` was found differing."""
    lo, hi = guard_chunk(n16, word)[1]
    s = samples_of(n16)
    if variant == "last-merged" and s > 1 and word >= chunk_bounds(n16, s - 2)[0]:
        return chunk_bounds(n16, s - 2)[0], n16
    return lo, hi


def _guard(snapshot, flat, gen, variant=None):
    snap, flat = _bytes(snapshot), _bytes(flat)
    assert snap.size == flat.size and (variant is None or variant in GUARD_MUTANTS)
    nbytes = snap.size
    n16, tail = split(nbytes)
    out = snap.copy()
    hit = False
    differing = _differing_words(snap, flat, n16)
    for w in np.intersect1d(differing, _compared(n16, gen, variant)).tolist():
        hit = True
        lo, hi = _chunk_of(n16, w, variant)
        if variant is not None and variant.startswith("copy16-"):
            counts = copy16_counts(hi, lo + np.arange(GUARD_BLOCK), GUARD_BLOCK, variant[len("copy16-"):])
            for i in np.flatnonzero(counts).tolist():            # a store past the payload: its bytes
                out[i * WORD:min((i + 1) * WORD, nbytes)] = flat[i * WORD:min((i + 1) * WORD, nbytes)]
            continue
        if variant == "hi+1":
            hi += 1
        elif variant == "hi-1":
            hi -= 1
        out[lo * WORD:min(hi * WORD, nbytes)] = flat[lo * WORD:min(hi * WORD, nbytes)]
    if tail and variant != "no-tail":
        t = slice(n16 * WORD, nbytes)
        if (snap[t] != flat[t]).any():
            hit = True
            out[t] = flat[t]                # byte by byte where they differ: the same bytes
    return out, hit


def guard_expected(snapshot_bytes, flat_bytes, gen):
    """(payload bytes, hit) a guarded reusing publish of generation `gen` must leave in the slot whose
    payload was `snapshot_bytes` when the parameters are `flat_bytes`: the snapshot, with every chunk
    whose sampled word differs taken from the parameters (chunk 0 also when the first word differs)
    and every differing tail byte; hit iff anything differed where it was compared.  Holds for
    k_guard_publish and k_guard_publish_bytes alike (module docstring)."""
    return _guard(snapshot_bytes, flat_bytes, gen)


def guard_mutant(name, snapshot_bytes, flat_bytes, gen):
    """guard_expected as a plausible wrong kernel would leave it:
    hi+1 / hi-1: the copied chunk's upper bound one word off; no-first-word: the first-word lane's
    report dropped; last-merged: the last word not a chunk of its own but part of the one before;
    no-tail: tail bytes ignored; fixed-samples: the sampled words do not move with the generation;
    copy16-no-remainder / copy16-deep+1 / copy16-deep-first: the chunk copy's copy16 as in
    copy16_counts (with chunks of 1025 words and stride 256 no lane's last load falls on the bound,
    so `<=` for `<` is right there; it is wrong under k_pull, tests/test_moves_host.py)."""
    assert name in GUARD_MUTANTS
    return _guard(snapshot_bytes, flat_bytes, gen, name)


WINDOW_MUTANTS = ("no-first-word", "no-last-word", "no-tail", "fixed-samples")


def window_expected(published_bytes, now_bytes, gen, variant=None):
    """Must the window guard count a written window?  `published_bytes` is the payload as it was
    published at generation `gen`, `now_bytes` what the next publish finds there: yes iff a word
    sampled at `gen`, the first word, the last word or a tail byte differs."""
    a, b = _bytes(published_bytes), _bytes(now_bytes)
    assert a.size == b.size and (variant is None or variant in WINDOW_MUTANTS)
    n16, tail = split(a.size)
    if tail and variant != "no-tail" and (a[n16 * WORD:] != b[n16 * WORD:]).any():
        return True
    if n16 == 0:
        return False
    words = set(sampled(n16, 0 if variant == "fixed-samples" else gen).tolist())
    s = samples_of(n16)
    if variant == "no-first-word" and s > 1 and chunk_sample(n16, 0, gen) != 0:
        words.discard(0)
    if variant == "no-last-word":
        words.discard(n16 - 1)
    return bool(np.intersect1d(_differing_words(a, b, n16), np.array(sorted(words), dtype=np.int64)).size)


# ---------------------------------------------------------------- what the GPU tests run
PUBLISH_BYTES = (1, 15, 16, 17, 1023, 1024, 1025, 3 * 1024 + 15)
PUBLISH_BIG_BYTES = 2 * 1024 * 1024 + 777   # past one pass of k_publish<false>'s capped grid (2 MiB)

GUARD_N16 = (1, 2, 17, 4095, 4096, 4097, 8191, 16 * 4095 + 1)
GUARD_BYTES_N16 = (1, 17, 4097, 8191)       # the byte form
GUARD_TAILS = (0, 4)
GUARD_FIRST_GEN = 2                          # the first guarded publish is the learner's second
GUARD_BIG_N16 = 4095 * 1025 + 1              # every chunk 1025 words: copy16's four-deep loop and remainder
WINDOW_N16 = (1, 17, 4097, 8191)
WINDOW_GENS = (1, 2, 3)
WINDOW_SHIFTS = (0, 3, 6, 9)


def guard_schedule(n16, tail, shift=0):
    """[(gen, case, words)] of one learner's guarded publishes: generations 2, 3, ... -- at least 2 to
    6, and as many as there are cases, so every case is written once; `shift` rotates which case
    meets which generation."""
    names = list(write_sets(n16, GUARD_FIRST_GEN, tail))
    out = []
    for r in range(max(5, len(names))):
        gen = GUARD_FIRST_GEN + r
        name = names[(r + shift) % len(names)]
        out.append((gen, name, write_sets(n16, gen, tail)[name]))
    return out


def window_schedule(n16, tail, shift):
    """[(gen, case, words)] of one resident learner's three windows."""
    names = list(write_sets(n16, WINDOW_GENS[0], tail))
    return [(gen, names[(i + shift) % len(names)], write_sets(n16, gen, tail)[names[(i + shift) % len(names)]])
            for i, gen in enumerate(WINDOW_GENS)]


def big_guard_case(gen=GUARD_FIRST_GEN):
    """(chunk, words) of the large case: a middle chunk written whole, its two neighbours written
    everywhere but at their sampled words -- so the middle chunk alone must be copied, all of it."""
    n16 = GUARD_BIG_N16
    k = (samples_of(n16) - 1) // 2
    words = list(range(*chunk_bounds(n16, k)))
    for c in (k - 1, k + 1):
        lo, hi = chunk_bounds(n16, c)
        words += [w for w in range(lo, hi) if w != chunk_sample(n16, c, gen)]
    return k, tuple(sorted(words))
