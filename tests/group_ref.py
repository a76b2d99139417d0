"""What float16 and mixed-dtype (segmented) models must compute through the multi-process groups, for
tests/test_group_dtypes_host.py and tests/test_gpu_group_dtypes.py.

Nothing here calls the GPU library or torch on a device; the layout and stripe arithmetic is
restated here and not taken from dpwa_amd.

Two payload kinds:

``"f16"``    N_F16 = 10,243 float16 elements: 20,486 bytes, ending 6 bytes into a 16-byte word; at
             world 3 the relay's stripes are 8192, 8192 and 4112 bytes.
``"mixed"``  the segmented layout MIXED = [f32 2049, bf16 2049, f16 2049] of tests/mixed_ref.segments:
             3 + 2 + 2 blocks of 4096 bytes, 28,672 bytes.  Each segment's elements end one element
             behind a block, so that the relay's stripe borders at 8192, 16384 and 24576 (world 4) each
             have one element behind them.

A payload is the bit patterns of its elements (``"f16"``: ``uint16``) or its bytes (``"mixed"``:
``uint8``, padding zero).  The expected trajectory of a lock-step job is ``oracle.gossip.simulate`` with
``lerp(kind)`` and ``add(kind)``; the board runs are checked by ``oracle.async_check.AsyncRuns`` with
``lerp(kind)`` and ``base(kind)``.

The GPU tests take their cases through ``case(job, kind, world)``, which refuses anything that
tests/test_group_dtypes_host.py has not examined.  ``MUTANTS`` are wrong implementations of the lock-step
trajectories (``trajectory(case, mutant)``; with no mutant it is ``simulate``'s, which the host test
asserts): the host test shows that the rounds the GPU test compares tell each of them from the reference.
"""
import collections
import functools

import numpy as np

from oracle import gossip as ogossip
from oracle import lerp as olerp
from oracle.async_check import async_base
from oracle.policy import OracleLearner
from tests import f16_ref, mixed_ref

WORD = 16
PAGE = 4096
N_F16 = 10_243
MIXED = [("f32", 2049), ("bf16", 2049), ("f16", 2049)]
KINDS = ("f16", "mixed")
HARD_FINITE = 7            # of mixed_ref.HARD: signed zeros, smallest and largest subnormals, smallest normal
VALUE = 0.5                # the configs' constant-interpolation value (unused by clock and loss)


def round_up(x, a):
    return (x + a - 1) // a * a


# ---------------------------------------------------------------- layout and stripes (restated)
def segments(kind):
    """([(dtype, byte offset, byte length, elements)], total bytes).  The float16 kind is a plain
    float16 buffer: one segment of exactly its elements, no block padding."""
    if kind == "f16":
        return [("f16", 0, 2 * N_F16, N_F16)], 2 * N_F16
    return mixed_ref.segments(MIXED)


def nbytes(kind):
    return segments(kind)[1]


def layout(kind):
    """The connection's `layout` argument as (dtype name, byte offset, byte length), None for "f16"."""
    if kind == "f16":
        return None
    return tuple((d, off, length) for d, off, length, _ in segments(kind)[0])


def stripe_bytes(kind, world):
    """round_up(ceil(payload16 / world), 4096): dpwa_learner_relay_enable's stripe."""
    payload16 = round_up(nbytes(kind), WORD)
    return round_up((payload16 + world - 1) // world, PAGE)


def stripes(kind, world):
    """[(begin, end)] of every rank's stripe in the payload rounded up to whole 16-byte words (the
    relay moves words); a stripe behind the payload is (end, end)."""
    payload16 = round_up(nbytes(kind), WORD)
    s = stripe_bytes(kind, world)
    return [(min(k * s, payload16), min((k + 1) * s, payload16)) for k in range(world)]


def borders(kind, world):
    """The byte offsets inside the payload at which one stripe ends and the next begins."""
    return [b for b, e in stripes(kind, world)[1:] if e > b]


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _native(kind, b):
    return b.view(np.uint16) if kind == "f16" else b


# ---------------------------------------------------------------- inputs
def _to_bits(d, x):
    if d == "f32":
        return x.view(np.uint32)
    if d == "bf16":
        return olerp.f32_to_bf16(x)
    return x.astype(np.float16).view(np.uint16)


def hard_ranges(kind, world):
    """[(segment index, first element, elements)] of the 16-byte words that carry hard values: the
    first and last word of every segment's elements and the words on either side of every stripe
    border, as far as they hold elements."""
    out = []
    segs, _ = segments(kind)
    for i, (d, off, _, n) in enumerate(segs):
        size, end = mixed_ref.SIZE[d], off + n * mixed_ref.SIZE[d]
        words = {off, off + (n * size - 1) // WORD * WORD}
        for b in borders(kind, world):
            words |= {b - WORD, b}
        for w in sorted(words):
            lo, hi = max(w, off), min(w + WORD, end)
            if lo < hi:
                out.append((i, (lo - off) // size, (hi - lo) // size))
    return out


def _payload(kind, world, rng, scale):
    segs, total = segments(kind)
    out = np.zeros(total, dtype=np.uint8)
    bits = []
    for d, off, _, n in segs:
        x = rng.standard_normal(n, dtype=np.float32)
        x *= np.float32(scale)
        bits.append(_to_bits(d, x).copy())
    for i, lo, k in hard_ranges(kind, world):
        hard = mixed_ref.HARD[segs[i][0]][:HARD_FINITE]
        bits[i][lo:lo + k] = hard[rng.integers(0, HARD_FINITE, k)]
    for (d, off, _, n), b in zip(segs, bits):
        out[off:off + n * mixed_ref.SIZE[d]] = b.view(np.uint8)
    return _native(kind, out)


def inputs(kind, world, T, seed):
    """(init (world, n), deltas (T, world, n), send losses, wait losses): values N(0, 1), deltas
    0.01 N(0, 1), rounded to each dtype; hard_ranges() of the parameters and of every delta hold the
    finite hard values (so those words stay signed zeros, subnormals and small normals through every
    round); padding zero.  Largest finites and infinities are left out: no round overflows."""
    rng = np.random.default_rng(seed)
    init = np.stack([_payload(kind, world, rng, 1.0) for _ in range(world)])
    deltas = np.stack([np.stack([_payload(kind, world, rng, 0.01) for _ in range(world)]) for _ in range(T)])
    send = [[float(2 * np.exp(-r / 4) + 0.05 * rng.random()) for _ in range(world)] for r in range(T)]
    wait = [[float(2 * np.exp(-(r + .5) / 4) + 0.05 * rng.random()) for _ in range(world)] for r in range(T)]
    return init, deltas, send, wait


# ---------------------------------------------------------------- the references, per dtype
def add_f32(p_u32, d_u32):
    return np.add(p_u32.view(np.float32), d_u32.view(np.float32), dtype=np.float32).view(np.uint32)


def add_f16(p_u16, d_u16):
    """torch-CPU eager ``p.add_(d)`` on float16."""
    t = f16_ref.as_half(p_u16)
    t.add_(f16_ref.as_half(d_u16))
    return f16_ref.as_u16(t)


def lerp_f32(p_u32, q_u32, f):
    return olerp.lerp_f32(p_u32.view(np.float32), q_u32.view(np.float32), f).view(np.uint32)


LERP = {"f32": lerp_f32, "bf16": olerp.lerp_bf16, "f16": f16_ref.torch_lerp}
ADD = {"f32": add_f32, "bf16": ogossip.add_bf16, "f16": add_f16}


def per_segment(kind, table):
    """A function of two payloads (and further arguments) that applies table[dtype] to every
    segment's elements; the padding of the result is zero (0 * a + 0 * b, 0 + 0)."""
    segs, total = segments(kind)

    def fn(p, q, *args):
        pb, qb = _bytes(p), _bytes(q)
        out = np.zeros(total, dtype=np.uint8)
        for seg in segs:
            d, off, _, n = seg
            r = table[d](mixed_ref.elements(pb, seg), mixed_ref.elements(qb, seg), *args)
            out[off:off + n * mixed_ref.SIZE[d]] = np.ascontiguousarray(r).view(np.uint8)
        return _native(kind, out)
    return fn


def lerp(kind):
    return f16_ref.torch_lerp if kind == "f16" else per_segment(kind, LERP)


def add(kind):
    return add_f16 if kind == "f16" else per_segment(kind, ADD)


def base(kind):
    """async_base rounded to float16, or per segment to the segment's dtype (each segment counts its
    own elements from 0), as base(rank, r, n) for AsyncRuns; n is the payload's elements ("f16") or
    bytes ("mixed")."""
    segs, total = segments(kind)

    def fn(rank, r, n):
        assert n == (N_F16 if kind == "f16" else total), n
        out = np.zeros(total, dtype=np.uint8)
        for d, off, _, k in segs:
            out[off:off + k * mixed_ref.SIZE[d]] = _to_bits(d, async_base(rank, r, k)).view(np.uint8)
        return _native(kind, out)
    return fn


def same(kind, got, want):
    """None when one payload equals another: bit for bit outside NaNs, padding byte for byte."""
    if kind == "mixed":
        return mixed_ref.same(MIXED, got, want)
    if f16_ref.same(got, want):
        return None
    return "float16: %s" % (f16_ref.mismatches(got, want),)


def finite(kind, payloads):
    """Whether no element of the payloads (any leading shape) is a NaN or an inf."""
    b = _bytes(payloads)
    b = b.reshape(-1, b.shape[-1])
    for d, off, _, n in segments(kind)[0]:
        e = np.ascontiguousarray(b[:, off:off + n * mixed_ref.SIZE[d]]).view(mixed_ref.NUMPY[d])
        exp = {"f32": 0x7f800000, "bf16": 0x7f80, "f16": 0x7c00}[d]
        if ((e & exp) == exp).any():
            return False
    return True


# ---------------------------------------------------------------- the cases
# phases: ((pull, rounds), ...).  A lock-step job creates its connection with pull="relay:8" (the relay
# buffers exist), switches with DpwaConnection.set_pull on every rank before the first round of a phase,
# and runs even rounds through update_wait_average, odd rounds through update_wait then average.
Case = collections.namedtuple("Case", "job kind world phases interp thr fp seed conn_seed")

PHASES = {"f16": (("copy", 4), ("kernel:64", 4), ("relay:8", 4), ("relay-avg:8", 4)),
          "mixed": (("copy", 4), ("kernel:64", 4), ("relay:8", 4))}
FP = 0.8
LOCKSTEP = ("walk", "resident", "vmm")

_CASES = [
    # 1. the phase walk
    Case("walk", "f16", 2, PHASES["f16"], "clock", 0.0, FP, 21, 500),
    Case("walk", "f16", 3, PHASES["f16"], "loss", 0.5, FP, 22, 510),
    Case("walk", "mixed", 3, PHASES["mixed"], "clock", 0.0, FP, 23, 520),
    Case("walk", "mixed", 4, PHASES["mixed"], "loss", 0.5, FP, 24, 530),
    # 2. resident parameters (the step after update_wait), rounds without a fetch relocate
    Case("resident", "f16", 3, (("relay-avg:8", 8),), "clock", 0.0, FP, 25, 540),
    Case("resident", "mixed", 3, (("relay:8", 8),), "loss", 0.5, FP, 26, 550),
    # 3. fd-shared slots
    Case("vmm", "mixed", 3, (("copy", 4), ("relay:8", 4)), "clock", 0.0, FP, 27, 560),
    # 4. the board (free-running, write-through): one pull, T rounds, every round fetches
    Case("board", "f16", 3, (("kernel:64", 16),), "clock", 0.0, 1.0, 0, 800),
    Case("board", "mixed", 2, (("copy", 16),), "clock", 0.0, 1.0, 0, 800),
]
CASES = {(c.job, c.kind, c.world): c for c in _CASES}


def case(job, kind, world):
    """The listed case; anything else is refused (the host test has examined exactly these)."""
    assert (job, kind, world) in CASES, "not in group_ref.CASES: %r" % ((job, kind, world),)
    return CASES[(job, kind, world)]


def lockstep_cases():
    return [c for c in _CASES if c.job in LOCKSTEP]


def rounds(c):
    return sum(k for _, k in c.phases)


def pull_at(c, r):
    """(pull, whether round r is the first of its phase)."""
    first = 0
    for pull, k in c.phases:
        if r < first + k:
            return pull, r == first
        first += k
    raise IndexError(r)


def phase_of(c, r):
    first = 0
    for i, (_, k) in enumerate(c.phases):
        if r < first + k:
            return i
        first += k
    raise IndexError(r)


def names(c):
    return ["r%d" % i for i in range(c.world)]


def seeds(c):
    return [c.conn_seed + g for g in range(c.world)]


@functools.lru_cache(maxsize=None)
def case_inputs(c):
    out = inputs(c.kind, c.world, rounds(c), c.seed)
    for a in out[:2]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(c):
    """oracle.gossip.simulate's trajectory of a lock-step case, computed once and left unchanged."""
    assert c.job in LOCKSTEP
    init, deltas, send, wait = case_inputs(c)
    exp = ogossip.simulate(names(c), init, deltas, send, wait, c.interp, VALUE, c.thr, c.fp, seeds(c),
                           lerp=lerp(c.kind), add=add(c.kind), train_after_wait=c.job == "resident")
    exp["peers"] = [[p[0] if p else "" for p in row] for row in exp["picks"]]       # [round][rank]
    exp["averaged"] = np.array([[bool(p) for p in row] for row in exp["picks"]])
    for k in ("params", "clocks", "averaged"):
        exp[k].setflags(write=False)
    return exp


# ---------------------------------------------------------------- wrong implementations
def lerp_f16_one_rounding(p_u16, q_u16, f):
    """f16(a * q + b * p) with the products and the sum in float32: one rounding instead of three."""
    a, b = olerp.coefficients(f)
    p = np.ascontiguousarray(p_u16).view(np.float16).astype(np.float32)
    q = np.ascontiguousarray(q_u16).view(np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        return (a * q + b * p).astype(np.float16).view(np.uint16)


def _relay(pull):
    return pull.partition(":")[0] in ("relay", "relay-avg")


class Mutant:
    """lerp_table: the per-dtype averages it uses.  fetch(c, pull, snap, prev, after, staged): the bytes
    it takes for the peer's snapshot, given the bytes the peer published this round (snap), one round
    earlier (prev), the peer's parameters after this round's training step (after) and what this rank's
    staging buffer held before (staged).  applies(c): whether the case runs the code it breaks."""

    def __init__(self, name, lerp_table=None, fetch=None, applies=lambda c: True):
        self.name, self.lerp_table, self.fetch, self.applies = name, lerp_table, fetch, applies


def _stale_stripe(c, pull, snap, prev, after, staged):
    out = snap.copy()
    if _relay(pull):
        lo, hi = stripes(c.kind, c.world)[1]
        out[lo:hi] = prev[lo:hi]
    return out


def _zero_stripe(c, pull, snap, prev, after, staged):
    out = snap.copy()
    if _relay(pull):
        lo, hi = stripes(c.kind, c.world)[1]
        out[lo:hi] = 0
    return out


def _short_last_stripe(c, pull, snap, prev, after, staged):
    out = snap.copy()
    if _relay(pull):
        lo, hi = [s for s in stripes(c.kind, c.world) if s[1] > s[0]][-1]
        cut = lo + (hi - lo - 1) // PAGE * PAGE
        out[cut:] = staged[cut:]
    return out


def _after_step(c, pull, snap, prev, after, staged):
    return after.copy()


def _tail_not_moved(c, pull, snap, prev, after, staged):
    out = snap.copy()
    k = out.size % WORD
    out[out.size - k:] = staged[out.size - k:]
    return out


MUTANTS = [
    Mutant("bf16-segment-as-f16", lerp_table=dict(LERP, bf16=f16_ref.torch_lerp), applies=lambda c: c.kind == "mixed"),
    Mutant("f16-as-bf16", lerp_table=dict(LERP, f16=olerp.lerp_bf16)),
    Mutant("f16-one-rounding", lerp_table=dict(LERP, f16=lerp_f16_one_rounding)),
    Mutant("stale-stripe", fetch=_stale_stripe),
    Mutant("zero-stripe", fetch=_zero_stripe),
    Mutant("short-last-stripe", fetch=_short_last_stripe),
    # (a resident loop trains after every rank's update_wait: there is no step inside the window)
    Mutant("snapshot-after-step", fetch=_after_step, applies=lambda c: c.job != "resident"),
    Mutant("tail-not-moved", fetch=_tail_not_moved, applies=lambda c: nbytes(c.kind) % WORD != 0),
]


def trajectory(c, mutant=None):
    """The lock-step rounds of a case restated over oracle.policy.OracleLearner with a staging buffer
    per rank, so that a mutant can misread a snapshot; {"params" (T, G, n), "clocks" (T, G), "peers"}.
    Without a mutant it is reference(c)'s."""
    kind, G, T = c.kind, c.world, rounds(c)
    nm = names(c)
    idx = {x: i for i, x in enumerate(nm)}
    init, deltas, send, wait = case_inputs(c)
    learners = [OracleLearner(nm[g], [x for x in nm if x != nm[g]], c.fp, c.interp, VALUE, c.thr, seeds(c)[g])
                for g in range(G)]
    avg = per_segment(kind, mutant.lerp_table if mutant is not None and mutant.lerp_table else LERP)
    step = add(kind)
    params = [init[g].copy() for g in range(G)]
    staged = [np.zeros(nbytes(kind), dtype=np.uint8) for _ in range(G)]
    prev = [np.zeros(nbytes(kind), dtype=np.uint8) for _ in range(G)]
    out = np.zeros((T, G) + init.shape[1:], init.dtype)
    clocks, peers = np.zeros((T, G)), [[""] * G for _ in range(T)]
    resident = c.job == "resident"
    for r in range(T):
        pull = pull_at(c, r)[0]
        states = [learners[g].update_send(send[r][g]) for g in range(G)]
        snaps = [_bytes(params[g]).copy() for g in range(G)]
        if not resident:
            params = [step(params[g], deltas[r, g]) for g in range(G)]
        after = [_bytes(params[g]).copy() for g in range(G)]
        for g in range(G):
            L = learners[g]
            state, q = None, None
            if L.fetching:
                state, q, _ = L.fetch(lambda peer: "ok", lambda peer: ("payload", states[idx[peer]], idx[peer]))
            averaged, factor = L.update_wait(wait[r][g], state, q is not None)
            if averaged:
                got = snaps[q]
                if mutant is not None and mutant.fetch is not None:
                    got = mutant.fetch(c, pull, snaps[q], prev[q], after[q], staged[g])
                staged[g] = got
                params[g] = avg(params[g], _native(kind, got), factor)
                peers[r][g] = nm[q]
            clocks[r, g] = L.clock
            out[r, g] = params[g]
        if resident:
            params = [step(params[g], deltas[r, g]) for g in range(G)]
        prev = snaps
    return {"params": out, "clocks": clocks, "peers": peers}


def differing(c, got):
    """The (rank, round) pairs in which a trajectory's parameters are not reference(c)'s."""
    want = reference(c)["params"]
    return [(g, r) for r in range(want.shape[0]) for g in range(want.shape[1])
            if same(c.kind, got["params"][r, g], want[r, g]) is not None]


# ---------------------------------------------------------------- the cross-process refusals
# two layouts of equal bytes (4096 + 8192 + 4096 and 4096 + 4096 + 8192) and other digests
REFUSED_LAYOUTS = ([("f32", 1), ("bf16", 2049), ("f16", 5)], [("f32", 1), ("bf16", 5), ("f16", 2049)])
REFUSED_DTYPES = ("f16", "bf16")      # rank 0's and rank 1's learner, REFUSED_N elements each
REFUSED_N = 2049
CONTROL_FACTOR = 0.5


def layout_of(spec):
    """(layout as (dtype name, offset, length), total bytes) of a mixed_ref spec."""
    segs, total = mixed_ref.segments(spec)
    return tuple((d, off, length) for d, off, length, _ in segs), total


def fnv_digest(lay):
    """dpwa_layout_digest restated: FNV-1a over each segment's little-endian (int32 dtype code, int64
    offset, int64 length); 0 becomes 1."""
    import struct
    h = 2166136261
    for d, off, length in lay:
        for byte in struct.pack("<iqq", mixed_ref.CODE[d], off, length):
            h = ((h ^ byte) * 16777619) & 0xffffffff
    return h or 1


def control_payload(rank):
    """What rank `rank` of the control pair holds and publishes (layout REFUSED_LAYOUTS[0])."""
    return mixed_ref.sample(REFUSED_LAYOUTS[0], 40 + rank)[0]
