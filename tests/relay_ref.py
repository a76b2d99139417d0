"""What the relay's stripe kernels must leave behind, restated on the host in plain numpy: the
model, the sizes, the pick sequences and the case list shared by tests/test_relay_host.py (no GPU),
tests/relay_worker.py and tests/test_gpu_relay.py.  The code modelled is k_relay_phase1,
k_relay_phase2, relay_copy and stripe_len, k_lerp_relay's StripeSrc (span_of, span_base, at) and
launch_average_relay of dpwa_amd/csrc/kernels.hip, and what feeds them in learner.cpp:
dpwa_learner_relay_enable's stripe size and relay_args' slot parity.  Restated from
include/dpwa_hip.h and the comments of kernels.hip, not from the kernels' arithmetic:

  a lock-step round of G ranks; rank i averages with rank picks[i] (-1: none).  Every snapshot
  payload (rounded up to 16 bytes) is cut into G stripes of ``stripe_bytes``.  Phase 1 on rank r
  pulls stripe r of every snapshot some rank needs -- its own pick's included, its own snapshot
  never -- into region j of its relay buffer (R_r[j] = stripe r of rank j).  After a barrier, phase
  2 on rank r with pick j gathers the 256-byte header from j's slot and stripe s of j's payload from
  j's slot itself for s == j, from its own relay buffer for s == r and from rank s's relay buffer
  otherwise.  The fused form gathers nothing: the averaging kernel reads every 1-KiB span, and every
  element of the ragged tail, where phase 2 would have read it.

``World`` holds every rank's two slots (publish number v goes to slot (v - 1) % 2) and relay buffer
(filled with SENTINEL at first, keeping earlier rounds' bytes) across rounds.  ``Job`` walks the
rounds of one (world, payload, dtype, blocks) case through every form the GPU test runs and yields,
per round and rank, what that rank must observe; tests/relay_worker.py walks the same Job on the GPU.
Expected parameters are not computed afresh: the model gives the peer bytes a rank must see (the
pick's forms_ref.operands, as test_relay_host.py asserts) and ``averaged`` hands them with the rank's
own operands to forms_ref.lerp, the host reference of the form tests; the factor and the clock are
oracle.policy.factor_and_clock's on the header the model says the rank reads.

The bytes between the payload's end and the next 16-byte boundary belong to nobody (the relay moves
them, nothing defines them): no comparison looks at them.

``RELAY_MUTANTS`` restate ways the code could be wrong; tests/test_relay_host.py shows that the cases
listed here tell each of them from the model.
"""
import functools
import struct

import numpy as np

from oracle import policy as opolicy
from tests import forms_ref, moves_ref
from tests.forms_ref import CODE, SIZE

WORD = 16
HEADER = 256                                # bytes of a slot's header that a gather moves
PAYLOAD_OFF = moves_ref.SLOT_PAYLOAD_OFFSET  # 4096: header room ahead of a slot's (and staging's) payload
PAGE = 4096                                 # stripes and slot rooms are whole pages
SPAN = 1024                                 # bytes one workgroup of the fused average takes (64 lanes x 16 B)
BLOCK = moves_ref.BLOCK                     # lanes of a relay-copy workgroup
SENTINEL = 0xC3                             # relay buffers at first; the staging buffer before every phase 2
OUTSIDE = 0xEE                              # what the model reads outside every buffer (wrong kernels only)

RELAY_MUTANTS = ("len-unclamped", "payload-floor16", "p1-src-stripe-j", "p1-dst-rank", "active-others-only",
                 "active-own-only", "pick-from-relay", "own-from-remote", "tail-from-last-item", "span-swapped",
                 "header-other-slot", "payload-other-slot", "header-other-rank",
                 "copy16-no-remainder", "copy16-deep+1", "copy16-deep-first")


def round_up(x, m):
    return (x + m - 1) // m * m


def round16(nbytes):
    return round_up(nbytes, WORD)


def stripe_bytes(payload_bytes, world):
    """dpwa_learner_relay_enable: the payload rounded up to 16 bytes, split evenly, in whole pages."""
    return round_up(-(-round16(payload_bytes) // world), PAGE)


def stripe_len(s, stripe, payload16, variant=None):
    """Bytes of stripe s that hold payload (payload16: the payload rounded up to 16 bytes)."""
    beg = s * stripe
    if variant == "len-unclamped":
        return stripe
    return max(0, min(stripe, payload16 - beg))


def slot_room(payload_bytes):
    """Bytes of a slot (and of the staging buffer) behind the payload offset."""
    return round_up(payload_bytes, PAGE)


def relay_counts(n16, blocks, variant=None):
    """How often a relay copy of n16 words by `blocks` workgroups stores each word
    (moves_ref.copy16_counts with first = blockIdx.y * 256 + lane and stride = blocks * 256)."""
    return moves_ref.copy16_counts(n16, np.arange(blocks * BLOCK), blocks * BLOCK, variant)


# ---------------------------------------------------------------- buffers
def _read(buf, off, n):
    """n bytes of `buf` from `off`; OUTSIDE where that leaves the buffer."""
    out = np.full(n, OUTSIDE, dtype=np.uint8)
    lo, hi = max(off, 0), min(off + n, buf.size)
    if hi > lo:
        out[lo - off:hi - off] = buf[lo:hi]
    return out


def _write(buf, off, data):
    lo, hi = max(off, 0), min(off + data.size, buf.size)
    if hi > lo:
        buf[lo:hi] = data[lo - off:hi - off]


def header_bytes(clock, loss, version, n, dtype):
    """The defined fields of a dpwa_header (clock, loss, version, n, dtype), 40 bytes."""
    return np.frombuffer(struct.pack("<ddQqii", clock, loss, version, n, CODE[dtype], 0), dtype=np.uint8)


HEADER_FIELDS = 40


class World:
    """Every rank's slots and relay buffer.  ``mutant``: one of RELAY_MUTANTS, or None."""

    def __init__(self, world, payload_bytes, mutant=None):
        assert mutant is None or mutant in RELAY_MUTANTS
        self.world, self.nbytes, self.mutant = world, payload_bytes, mutant
        self.stripe = stripe_bytes(payload_bytes, world)
        self.payload16 = payload_bytes // WORD * WORD if mutant == "payload-floor16" else round16(payload_bytes)
        self.room = slot_room(payload_bytes)
        self.slots = np.zeros((world, 2, PAYLOAD_OFF + self.room), dtype=np.uint8)
        self.relay = np.full((world, world * self.stripe), SENTINEL, dtype=np.uint8)
        self.copy16 = mutant[len("copy16-"):] if mutant and mutant.startswith("copy16-") else None

    # -- what a learner does ------------------------------------------------
    def publish(self, rank, version, header, payload):
        slot = self.slots[rank, (version - 1) % 2]
        slot[:header.size] = header
        slot[PAYLOAD_OFF:PAYLOAD_OFF + self.nbytes] = payload

    def staging(self):
        """A staging buffer as the test leaves it before phase 2."""
        return np.full(PAYLOAD_OFF + self.room, SENTINEL, dtype=np.uint8)

    def _slot(self, rank, version, what):
        k = (version - 1) % 2
        if self.mutant == what + "-other-slot":
            k ^= 1
        return self.slots[rank, k]

    def _len(self, s):
        return stripe_len(s, self.stripe, self.payload16, "len-unclamped" if self.mutant == "len-unclamped" else None)

    def _copy(self, dst, dst_off, src, src_off, nbytes, blocks):
        """relay_copy: nbytes / 16 words, as `blocks` workgroups of copy16 store them."""
        n16 = nbytes // WORD
        if self.copy16 is None:
            _write(dst, dst_off, _read(src, src_off, n16 * WORD))
            return
        at = (np.flatnonzero(relay_counts(n16, blocks, self.copy16))[:, None] * WORD + np.arange(WORD)).ravel()
        s, d = src_off + at, dst_off + at                    # a store past the words: its bytes, where a buffer is
        inside = (s >= 0) & (s < src.size)
        data = np.where(inside, src[np.where(inside, s, 0)], OUTSIDE).astype(np.uint8)
        keep = (d >= 0) & (d < dst.size)
        dst[d[keep]] = data[keep]

    def active(self, rank, j, picks):
        """Does phase 1 on `rank` pull its stripe of rank j's snapshot?"""
        if j == rank:
            return False
        if self.mutant == "active-others-only":
            return any(picks[i] == j for i in range(self.world) if i != rank)
        if self.mutant == "active-own-only":
            return picks[rank] == j
        return any(picks[i] == j for i in range(self.world))

    def phase1(self, rank, picks, version, blocks):
        for j in range(self.world):
            if not self.active(rank, j, picks):
                continue
            s = j if self.mutant == "p1-src-stripe-j" else rank
            d = rank if self.mutant == "p1-dst-rank" else j
            self._copy(self.relay[rank], d * self.stripe, self._slot(j, version, "payload"),
                       PAYLOAD_OFF + s * self.stripe, self._len(s), blocks)

    def sources(self, rank, pick, version):
        """[(buffer, offset)] per stripe s: where rank `rank` finds stripe s of its pick's payload."""
        out = []
        for s in range(self.world):
            own_slot = s == pick and self.mutant != "pick-from-relay"
            if own_slot:
                out.append((self._slot(pick, version, "payload"), PAYLOAD_OFF + s * self.stripe))
            elif s == rank and self.mutant == "own-from-remote":
                out.append((self.relay[(rank + 1) % self.world], pick * self.stripe))
            else:
                out.append((self.relay[s], pick * self.stripe))
        return out

    def header_of(self, rank, pick, version):
        """The 256 header bytes rank `rank` averages with."""
        if self.mutant == "header-other-rank":
            pick = next(r for r in range(self.world) if r != pick)
        return self._slot(pick, version, "header")[:HEADER].copy()

    def phase2(self, rank, picks, version, blocks, staging):
        """The gathered form, into `staging` (header at 0, payload at PAYLOAD_OFF)."""
        pick = picks[rank]
        if pick < 0:
            return staging
        staging[:HEADER] = self.header_of(rank, pick, version)
        for s, (buf, off) in enumerate(self.sources(rank, pick, version)):
            self._copy(staging, PAYLOAD_OFF + s * self.stripe, buf, off, self._len(s), blocks)
        return staging

    # -- the fused form -----------------------------------------------------
    def fused_sources(self, rank, pick, version, dtype):
        """What the fused average reads: [(payload offset, length, buffer, buffer offset)] for every
        1-KiB span that holds whole 16-byte items (in workgroup order) and then for every element of
        the ragged tail."""
        src = self.sources(rank, pick, version)
        size = SIZE[dtype]
        vbytes = self.nbytes // WORD * WORD
        parts, per_stripe = self.world, self.stripe // SPAN
        out = []
        for b in range(parts * per_stripe):
            if self.mutant == "span-swapped":
                span_off = (b // parts) * self.stripe + (b % parts) * SPAN
            else:
                span_off = (b % parts) * self.stripe + (b // parts) * SPAN
            if span_off >= vbytes:
                continue
            s = span_off // self.stripe
            buf, off = src[s]
            out.append((span_off, min(SPAN, vbytes - span_off), buf, off + span_off - s * self.stripe))
        s_last = max(vbytes - WORD, 0) // self.stripe
        for byte in range(vbytes, self.nbytes, size):
            s = s_last if self.mutant == "tail-from-last-item" else byte // self.stripe
            buf, off = src[s]
            out.append((byte, size, buf, off + byte - s * self.stripe))
        return out

    def fused_peer(self, rank, pick, version, dtype):
        """(peer payload bytes as the fused average sees them, how many workgroups or tail lanes take
        each byte): the second is 1 everywhere for a right kernel."""
        peer = np.full(self.nbytes, OUTSIDE, dtype=np.uint8)
        visits = np.zeros(self.nbytes, dtype=np.int64)
        for at, n, buf, off in self.fused_sources(rank, pick, version, dtype):
            peer[at:at + n] = _read(buf, off, n)
            visits[at:at + n] += 1
        return peer, visits


# ---------------------------------------------------------------- sizes
# (world, payload bytes): the stripe-edge sizes; tests/test_relay_host.py asserts each one's layout.
# (4, 12324) leaves 48 bytes on the last rank (two items and the tail's word), so (4, 12308) stands
# beside it for "one item and the tail's word alone on the last rank"; (3, 8196) is the ragged tail
# alone in a stripe held by a rank that is neither side of a pair.
EDGE_SIZES = ((2, 4100), (2, 8192), (2, 8188), (3, 5124), (3, 8196), (4, 12324), (4, 12308), (4, 20))
EDGE_BLOCKS = 2
COPY16_BLOCKS = (1, 2)
COPY16_POINTS = ("4s-1", "4s", "4s+1", "7s+3")
TAIL_BYTES = 12     # of the copy16 payloads: three float32 or six 16-bit elements, of which
                    # forms_ref.sample pins only the last two


def copy16_words(point, blocks):
    s = blocks * BLOCK
    return {"4s-1": 4 * s - 1, "4s": 4 * s, "4s+1": 4 * s + 1, "7s+3": 7 * s + 3}[point]


def last_stripe(world, payload_bytes):
    """(index, words) of the last stripe that holds payload."""
    stripe, p16 = stripe_bytes(payload_bytes, world), round16(payload_bytes)
    s = (p16 - 1) // stripe
    return s, stripe_len(s, stripe, p16) // WORD


@functools.lru_cache(maxsize=None)
def relay_sizes(world, blocks):
    """{point: payload bytes}: the smallest payloads whose last non-empty stripe has the word counts
    at which copy16 changes its path for the stride blocks * 256.  A stripe is a whole number of
    pages, at most a page more than an even share, so the last stripe lies within world * 256 words
    of a full one: a point is reached with `full` whole stripes ahead of it where
    stripe_bytes(payload) reproduces the stripe assumed."""
    out = {}
    for point in COPY16_POINTS:
        want = copy16_words(point, blocks)
        best = None
        for full in range(1, world):
            for stripe_w in range(round_up(want, PAGE // WORD), want + world * (PAGE // WORD) + 1, PAGE // WORD):
                words = full * stripe_w + want
                nbytes = words * WORD - (WORD - TAIL_BYTES)
                if stripe_bytes(nbytes, world) == stripe_w * WORD and last_stripe(world, nbytes) == (full, want):
                    if best is None or nbytes < best:
                        best = nbytes
        if best is not None:
            out[point] = best
    return out


def sizes(world):
    """[(payload bytes, blocks)] the GPU test runs for a world."""
    out = [(b, EDGE_BLOCKS) for w, b in EDGE_SIZES if w == world]
    for blocks in COPY16_BLOCKS:
        out += [(b, blocks) for b in relay_sizes(world, blocks).values()]
    return list(dict.fromkeys(out))


# ---------------------------------------------------------------- topologies, losses, forms
WORLDS = (2, 3, 4)
PICKS = {2: ((1, 0), (1, -1), (-1, 0), (1, 0)),
         3: ((1, 2, 0), (1, 0, -1), (2, 2, 0)),
         4: ((1, 2, 3, 0), (1, 0, 3, 2), (1, 0, 0, 0), (2, 3, -1, 1))}

# gather: fuse = 0, then dpwa_learner_average; fused / through: fuse = 1, then dpwa_learner_average /
# _average_through; copy: fuse = 1, then dpwa_learner_copy_fetched (relay_materialize gathers) and
# dpwa_learner_cancel; resident: fuse = 1 on a resident learner of its own (the out-of-place kernel)
FORMS = ("gather", "fused", "through", "copy", "resident")
GATHERS = ("gather", "copy")                 # forms that fill the staging buffer
REPUBLISH = ("through", "resident")          # forms whose rounds after the first end with a second publish
SECOND_LOSS = 1000.0                         # added to the round's loss for that second publish


def loss_of(rank, t):
    """The loss rank `rank` publishes (and averages with) in round t."""
    return 0.2 + 0.11 * rank + 0.37 * t + 0.05 * ((7 * rank + 3 * t) % 5)


def seed_of(form, rank, t):
    """forms_ref.sample seed of a rank's parameters: one block of sixteen per form, so that all of a
    form's operands have their hard values at the same places (forms_ref.hard_phase) and no two
    (form, round, rank) share a payload."""
    return 16 * (1 + FORMS.index(form)) + 4 * t + rank


def payload_of(dtype, nbytes, form, rank, t):
    """(bits, bytes) of the parameters rank `rank` publishes in round t of `form`."""
    n = nbytes // SIZE[dtype]
    bits = forms_ref.operands(dtype, n, seed_of(form, rank, t))[0]
    return bits, bits.view(np.uint8)


def averaged(dtype, nbytes, form, rank, t, f, peer):
    """Expected bits of rank's parameters of round t after averaging at factor f with the peer payload
    bytes `peer` (what the model says the rank reads; for a right relay the pick's published payload,
    forms_ref.operands of its seed): the host reference of forms_ref."""
    p = payload_of(dtype, nbytes, form, rank, t)[0]
    return forms_ref.lerp(dtype, p, np.ascontiguousarray(peer).view(forms_ref.NUMPY[dtype]), f)


class Seen:
    """What one rank must observe in one round."""
    __slots__ = ("form", "t", "rank", "pick", "version", "loss", "published", "header", "staging", "peer", "visits",
                 "peer_header", "factor", "clock_before", "clock_after", "republish", "republish_clock")

    def observation(self):
        """Everything a wrong relay could change, as one tuple of bytes (for the mutant test)."""
        parts = [self.staging, self.peer, self.visits, self.peer_header]
        return tuple(None if p is None else np.asarray(p).tobytes() for p in parts)


class Job:
    """One (world, payload, dtype, blocks) case through `forms`: iterate ``rounds()``."""

    def __init__(self, world, nbytes, dtype, blocks, forms=FORMS, mutant=None):
        assert nbytes % 4 == 0 and world in PICKS
        self.world, self.nbytes, self.dtype, self.blocks = world, nbytes, dtype, blocks
        self.forms, self.mutant = tuple(forms), mutant
        self.n = nbytes // SIZE[dtype]

    def learner_sets(self):
        """The forms that share one set of learners: a resident learner is resident for life."""
        plain = tuple(f for f in self.forms if f != "resident")
        return [fs for fs in (plain, tuple(f for f in self.forms if f == "resident")) if fs]

    def rounds(self, forms):
        """Yields (form, t, picks, version, [Seen per rank]) for one set of learners, in order."""
        w = World(self.world, self.nbytes, self.mutant)
        clock = [0.0] * self.world
        version = 0
        for form in forms:
            for t, picks in enumerate(PICKS[self.world]):
                version += 1
                seen = []
                for r in range(self.world):
                    clock[r] += 1.0                                       # dpwa.py:112
                    s = Seen()
                    s.form, s.t, s.rank, s.pick, s.version, s.loss = form, t, r, picks[r], version, loss_of(r, t)
                    s.published = payload_of(self.dtype, self.nbytes, form, r, t)[1]
                    s.header = header_bytes(clock[r], s.loss, version, self.n, self.dtype)
                    s.clock_before = clock[r]
                    w.publish(r, version, s.header, s.published)
                    seen.append(s)
                for r in range(self.world):
                    w.phase1(r, picks, version, self.blocks)
                for s in seen:
                    r, pick = s.rank, s.pick
                    s.staging = s.peer = s.visits = s.peer_header = s.factor = None
                    s.clock_after = s.clock_before
                    if form in GATHERS:
                        s.staging = w.phase2(r, picks, version, self.blocks, w.staging())
                    if pick >= 0:
                        if form in GATHERS:
                            s.peer = s.staging[PAYLOAD_OFF:PAYLOAD_OFF + self.nbytes].copy()
                            s.peer_header = s.staging[:HEADER].copy()
                        else:
                            s.peer, s.visits = w.fused_peer(r, pick, version, self.dtype)
                            s.peer_header = w.header_of(r, pick, version)
                        peer_clock, peer_loss = struct.unpack("<dd", s.peer_header[:16].tobytes())
                        if form != "copy":
                            s.factor, s.clock_after = opolicy.factor_and_clock("loss", None, 0.0, s.clock_before,
                                                                               peer_clock, s.loss, peer_loss)
                    clock[r] = s.clock_after
                second = form in REPUBLISH and t > 0
                if second:
                    version += 1
                for s in seen:
                    s.republish = version if second else 0
                    if second:
                        clock[s.rank] += 1.0
                    s.republish_clock = clock[s.rank]
                yield form, t, picks, seen[0].version, seen
                if second:      # the slot no right relay reads (the next round's publish takes the other one)
                    for s in seen:
                        w.publish(s.rank, version, header_bytes(s.republish_clock, s.loss + SECOND_LOSS, version,
                                                                self.n, self.dtype), s.published)


def cases(world):
    """[(payload bytes, blocks, dtype)] of one world's GPU test."""
    return [(nbytes, blocks, dtype) for nbytes, blocks in sizes(world) for dtype in forms_ref.DTYPES]
