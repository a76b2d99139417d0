"""Payloads beyond 2^31 elements and 2^32 bytes, described by position, and what every streaming
kernel must leave in them: the host side of tests/test_gpu_big.py, checked by tests/test_big_host.py.

Nothing of 4 GiB exists on the host.  An ``Operand`` is a constant bit pattern per element type
everywhere but in a few 4-KiB ``windows`` of the payload -- at byte 0, around byte 2^31, around byte
2^32, over the last 4096 bytes (ragged tail included) and 2 KiB either side of every segment or tensor
border -- which hold seeded values of their own.  Three families of operands:

  HARD    constants 1.0 (parameters) and 2.5 (peer), windows of ``forms_ref.operands`` hard values;
          with FACTOR the five values A, B, lerp(A,B), lerp(lerp(A,B),B) and lerp(B,A) differ, so an
          element averaged twice, not at all, or with the roles swapped shows in the constant region
  EXACT   constants 1.0 and 1.5, windows of seeded half-integers |x| <= 31.5: every term (q-p)^2 and
          p^2 is a multiple of 2^-2 below 2^12 and every total stays below 2^46, so each float64
          addition is exact in any order and the expected sums are compared with ==
  FINITE  the peer alone: ``finite_ref.LARGEST`` everywhere, ``finite_ref.finite_noise`` in the windows

The model restates a kernel as a ``cover`` of the payload's bytes: pieces (lo, hi, k, dtype) where k
counts the threads that load, combine and store the elements of [lo, hi) (1 everywhere for a right
kernel; 0: never reached; 2: reached twice, which an in-place average applies twice and a sum counts
twice) and dtype is the element type the piece is treated as.  A kernel whose wrong arithmetic makes it
address bytes before the buffer has no cover: ``OUTSIDE``.  From a cover and the operands come the four
things the GPU module checks -- the bits of every window, the number of constant-region elements that
differ from the host-computed constant (``stray``), the exact sums, and the veto -- each evaluated on
the windows and, for the constant region, per piece in closed form.

``MUTANTS`` restates plausible 32-bit slips as covers.  ``EQUIVALENT`` names the slip asked about that
no output can show, and why.

The reuse guard and the window guard have a model of their own at the end (``guard_model``,
``window_model``): the snapshot and the parameters differ at a handful of written bytes only, so what a
guarded publish must leave is the set of written bytes it takes over -- tests/moves_ref.py's model on
whole host arrays, which tests/test_big_host.py compares it with at small sizes -- and two more slips
(``GUARD_MUTANTS``) live there.  The relay's stripe cover (``relay_cover``, ``relay_model``) and its slips
(``RELAY_MUTANTS``) follow it.
"""
import numpy as np

from tests import finite_ref
from tests import forms_ref as fref
from tests.mixed_ref import NUMPY, SIZE

L31, L32 = 1 << 31, 1 << 32
WIN, HALF = 4096, 2048
FACTOR = 0.3                      # != 0.5: the role-swapped average differs
FILL = fref.GUARD_BYTE            # what a destination holds before the kernel (forms_ref.guarded)
OUTSIDE = "OUTSIDE"               # the kernel reads or writes bytes that are not the buffer's
CHUNK = 1 << 28                   # elements per device-side comparison

# the smallest sizes at which a 32-bit byte offset (and, at 2 bytes, an element index) wraps
N = {"bf16": L31 + 1001, "f16": L31 + 1001, "f32": (1 << 30) + 1001}
MIXED_SEGS = (("bf16", 0, L32 + 4096), ("f32", L32 + 4096, L32 + 12288), ("f16", L32 + 12288, L32 + 16384))
# tensors of the bf16 payload (begin, end), begins on 256-byte boundaries
TENSORS = ((0, L31 + 100), (L31 + 256, L32 - 262), (L32 - 256, L32 + 300), (L32 + 512, N["bf16"] * 2))


# ---------------------------------------------------------------- bit patterns
def encode(dtype, values):
    """Bits of values that `dtype` holds exactly."""
    x = np.asarray(values, dtype=np.float32)
    if dtype == "f32":
        return x.view(np.uint32).copy()
    if dtype == "bf16":
        u = x.view(np.uint32)
        assert not (u & 0xffff).any(), "not a bfloat16 value"
        return (u >> 16).astype(np.uint16)
    h = x.astype(np.float16)
    assert (h.astype(np.float32) == x).all(), "not a float16 value"
    return h.view(np.uint16).copy()


def decode(dtype, bits):
    """float64 values of bit patterns (every widening is exact)."""
    bits = np.ascontiguousarray(bits, dtype=NUMPY[dtype])
    if dtype == "f32":
        return bits.view(np.float32).astype(np.float64)
    if dtype == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return bits.view(np.float16).astype(np.float64)


def as_bits(dtype, raw):
    return np.ascontiguousarray(raw, dtype=np.uint8).view(NUMPY[dtype])


# ---------------------------------------------------------------- payloads and windows
class Payload:
    """`nbytes` of one element type or of segments [(dtype, lo, hi)]; `borders`: the byte offsets
    (segment or tensor borders, stripe borders) that get a window of their own."""

    def __init__(self, segs, borders=()):
        self.segs = tuple(segs)
        assert self.segs[0][1] == 0 and all(a[2] == b[1] for a, b in zip(self.segs, self.segs[1:]))
        self.nbytes = self.segs[-1][2]
        self.borders = tuple(borders)
        self.dtypes = tuple(d for d, _, _ in self.segs)
        self.wins = windows(self.nbytes, self.borders)

    @property
    def dtype(self):
        assert len(self.segs) == 1
        return self.segs[0][0]

    def split(self, lo, hi):
        """[(dtype, a, b)]: [lo, hi) by segment."""
        return [(d, max(lo, a), min(hi, b)) for d, a, b in self.segs if max(lo, a) < min(hi, b)]

    def gaps(self):
        """The constant region: [(lo, hi)] between the windows."""
        edges = [0] + [x for w in self.wins for x in w] + [self.nbytes]
        return [(a, b) for a, b in zip(edges[0::2], edges[1::2]) if a < b]


def windows(nbytes, borders=()):
    raw = [(0, WIN), (L31 - HALF, L31 + HALF), (L32 - HALF, L32 + HALF), (nbytes - WIN, nbytes)]
    raw += [(b - HALF, b + HALF) for b in borders]
    out = []
    for lo, hi in sorted((max(0, a), min(nbytes, b)) for a, b in raw):
        if lo >= hi:
            continue
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def single(dtype, n=None, borders=()):
    return Payload([(dtype, 0, (N[dtype] if n is None else n) * SIZE[dtype])], borders)


def mixed():
    return Payload(MIXED_SEGS, [a for _, a, _ in MIXED_SEGS[1:]])


def tabled():
    """The bf16 payload with a window at every tensor border."""
    return single("bf16", borders=sorted({x for t in TENSORS for x in t}))


# ---------------------------------------------------------------- families
def _hard(dtype, m, seed):
    return fref.operands(dtype, m, seed)


def _exact(dtype, m, seed):
    rng = np.random.default_rng([seed, 77])
    return tuple(encode(dtype, rng.integers(-63, 64, m) / 2.0) for _ in range(2))


def _noise(dtype, m, seed):
    return None, finite_ref.finite_noise(dtype, m, seed)


def _consts(p, q):
    return {d: (encode(d, [p])[0], encode(d, [q])[0]) for d in fref.DTYPES}


FAMILIES = {
    "hard": (_consts(1.0, 2.5), _hard),
    "exact": (_consts(1.0, 1.5), _exact),
    "finite": ({d: (encode(d, [1.0])[0], NUMPY[d](finite_ref.LARGEST[d])) for d in fref.DTYPES}, _noise),
}


class Operand:
    """One buffer of a payload: `const[dtype]` everywhere, `data[k]` (uint8) in window k."""

    def __init__(self, payload, const, data):
        self.payload, self.const, self.data = payload, const, data

    def bytes(self, lo, hi):
        """The bytes of [lo, hi) (small ranges only)."""
        assert 0 <= lo <= hi <= self.payload.nbytes and hi - lo <= (1 << 20)
        out = np.empty(hi - lo, dtype=np.uint8)
        for d, a, b in self.payload.split(lo, hi):
            assert a % SIZE[d] == 0 and b % SIZE[d] == 0, "a range cuts an element"
            out[a - lo:b - lo] = np.full((b - a) // SIZE[d], self.const[d], dtype=NUMPY[d]).view(np.uint8)
        for (a, b), w in zip(self.payload.wins, self.data):
            x, y = max(a, lo), min(b, hi)
            if x < y:
                out[x - lo:y - lo] = w[x - a:y - a]
        return out

    def planted(self, at, dtype, bits):
        """A copy with one element replaced; `at` (bytes) must lie in a window."""
        k = [i for i, (a, b) in enumerate(self.payload.wins) if a <= at < b]
        assert len(k) == 1, "a planted element lies in no window"
        data = list(self.data)
        w = data[k[0]].copy()
        a = self.payload.wins[k[0]][0]
        w[at - a:at - a + SIZE[dtype]] = np.array([bits], dtype=NUMPY[dtype]).view(np.uint8)
        data[k[0]] = w
        return Operand(self.payload, self.const, data)


def operands(payload, family, seed=0):
    """(parameters, peer) of a family over a payload; window k of the pair has its own seed."""
    const, draw = FAMILIES[family]
    pd, qd = [], []
    for k, (lo, hi) in enumerate(payload.wins):
        p, q = np.zeros(hi - lo, dtype=np.uint8), np.zeros(hi - lo, dtype=np.uint8)
        for j, (d, a, b) in enumerate(payload.split(lo, hi)):
            pb, qb = draw(d, (b - a) // SIZE[d], 4001 + 64 * seed + 4 * k + j)
            q[a - lo:b - lo] = np.asarray(qb).view(np.uint8)
            if pb is not None:
                p[a - lo:b - lo] = np.asarray(pb).view(np.uint8)
        pd.append(p)
        qd.append(q)
    return (Operand(payload, {d: c[0] for d, c in const.items()}, pd),
            Operand(payload, {d: c[1] for d, c in const.items()}, qd))


LEARNER_CONST = (1.0, 2.5, -0.75)      # resident learners that average each other's parameters


def learner(payload, i):
    """The parameters of resident learner i (hard family): a constant and windows of its own."""
    P, Q = operands(payload, "hard", seed=1 + i // 2)
    src = (P, Q)[i % 2]
    return Operand(payload, {d: encode(d, [LEARNER_CONST[i]])[0] for d in fref.DTYPES}, src.data)


# ---------------------------------------------------------------- covers
def cover(payload, breaks, fn):
    """[(lo, hi, fn(lo))] over the payload, cut at `breaks`."""
    pts = sorted({b for b in breaks if 0 < b < payload.nbytes} | {0, payload.nbytes})
    return [(lo, hi) + tuple(fn(lo)) for lo, hi in zip(pts, pts[1:])]


def _body(payload, family):
    """The bytes the vector body covers: whole 16-byte items for a span kernel, the rest is its
    ragged tail; an element-wise kernel has no tail of its own."""
    return payload.nbytes // 16 * 16 if family == "span" else payload.nbytes


def seg_dtype(begins, dtypes, off):
    """kernels.hip seg_dtype: the last segment whose begin is at or below `off`."""
    d = dtypes[0]
    for k in range(1, len(begins)):
        if off >= begins[k]:
            d = dtypes[k]
    return d


def right_cover(payload):
    return cover(payload, [a for _, a, _ in payload.segs], lambda y: (1, seg_dtype([a for _, a, _ in payload.segs],
                                                                                  payload.dtypes, y)))


# name -> what the slip is, and where it can live: kernel families ("span": one descriptor per 1-KiB
# or wider span of 16-byte items plus a ragged tail; "elem": the grid-stride element-wise forms) or a
# single operation
MUTANTS = {
    "offset-mod-2^32": "the byte offset of a span or element kept in 32 bits",
    "offset-sign-extended": "the byte offset widened from a signed 32-bit value",
    "index-mod-2^31": "the element index of an element-wise kernel kept in 31 bits",
    "tail-from-32-bit-n": "the ragged tail's byte offset computed in 32 bits",
    "grid-truncated": "spans beyond 2^32 bytes never run",
    "segment-begins-32-bit": "a segmented payload's begins truncated to 32 bits: later segments get the wrong rounding",
    "table-begins-32-bit": "the tensor table's begins truncated to 32 bits",
    "nonfinite-below-2^32-only": "the finite check looks at the first 2^32 bytes only",
}
# param_row's span index taken before the tensor's begin is subtracted: the row is
# first_row + s % rows either way, so the term lands in another row OF THE SAME TENSOR and the finishing
# step, which sums all of a tensor's rows, gives the same pair.  No output tells it from the model.
EQUIVALENT = {"param-row-before-begin": "s % rows stays inside the tensor's own rows, which are summed together"}
# The variant of it that does show: the payload's span index reduced modulo max_rows, not the tensor's own
# span index modulo the tensor's rows.  A tensor of fewer rows than max_rows then adds into rows behind its
# own: the next tensor's, or none of the workspace's (``table_rows``).
MUTANTS["param-row-payload-span"] = "param_row's row from the payload's span index modulo max_rows"
PARAM_MAX_ROWS = 1024


def table_rows(tensors, name=None):
    """[(tensor the row belongs to, or OUTSIDE)] for every (tensor, 1-KiB span it touches) pair whose term
    does not land in the tensor's own rows; empty for the right kernel."""
    spans = [(a // 1024, -(-b // 1024)) for a, b in tensors]
    rows = [min(hi - lo, PARAM_MAX_ROWS) for lo, hi in spans]
    first = [sum(rows[:t]) for t in range(len(rows))]
    astray = []
    if name == "param-row-payload-span":
        for t, (lo, hi) in enumerate(spans):
            for s in set(range(lo, min(hi, lo + PARAM_MAX_ROWS))) | {hi - 1}:
                row = first[t] + s % PARAM_MAX_ROWS
                if not first[t] <= row < first[t] + rows[t]:
                    owner = [u for u in range(len(rows)) if first[u] <= row < first[u] + rows[u]]
                    astray.append((t, s, owner[0] if owner else OUTSIDE))
    return astray


def mutant_cover(payload, family, op, name):
    """The cover of `op` ("lerp", "copy", "sums", "finite", "table") run by a `family` kernel with the
    slip `name`; OUTSIDE; or None where the slip cannot live in that kernel or changes nothing there."""
    nb, body = payload.nbytes, _body(payload, family)
    begins = [a for _, a, _ in payload.segs]
    right = right_cover(payload)

    def dt(y):
        return seg_dtype(begins, payload.dtypes, y)

    if name == "offset-mod-2^32":
        if body <= L32:
            return None
        w = body - L32        # threads at y and y + 2^32 both address y
        out = cover(payload, begins + [w, L32, body], lambda y: ((2 if y < w else 1 if y < L32 else 0 if y < body else 1), dt(y)))
    elif name == "offset-sign-extended":
        return OUTSIDE if body > L31 else None
    elif name == "index-mod-2^31":
        if family != "elem" or len(payload.segs) > 1:
            return None
        wrap = L31 * SIZE[payload.dtype]
        if nb <= wrap:
            return None
        out = cover(payload, [nb - wrap, wrap], lambda y: ((2 if y < nb - wrap else 1 if y < wrap else 0), dt(y)))
    elif name == "tail-from-32-bit-n":
        if family != "span" or body == nb or body < L32:
            return None
        t = body - L32        # where the tail's elements are read and stored instead
        out = cover(payload, begins + [t, t + nb - body, body], lambda y: ((2 if t <= y < t + nb - body else 0 if y >= body else 1), dt(y)))
    elif name == "grid-truncated":
        if family != "span" or body <= L32:
            return None
        out = cover(payload, begins + [L32, body], lambda y: ((0 if L32 <= y < body else 1), dt(y)))
    elif name == "segment-begins-32-bit":
        if len(payload.segs) == 1:
            return None
        cut = [b & (L32 - 1) for b in begins]
        out = cover(payload, begins + cut, lambda y: (1, seg_dtype(cut, payload.dtypes, y)))
    elif name == "nonfinite-below-2^32-only":
        if op != "finite" or nb <= L32:
            return None
        out = cover(payload, begins + [L32], lambda y: ((1 if y < L32 else 0), dt(y)))
    else:
        return None
    return None if out == right else out


def table_members(payload, tensors, name=None):
    """[(lo, hi, t)]: which tensor (-1: none) the pass adds the bytes of [lo, hi) to.  The lookup takes
    the last tensor whose begin is at or below the byte, and the byte counts if it lies before that
    tensor's end."""
    begins = [b & (L32 - 1) if name == "table-begins-32-bit" else b for b, _ in tensors]
    ends = [e for _, e in tensors]

    def member(y):
        t = max((i for i, b in enumerate(begins) if b <= y), default=-1)
        return (t if t >= 0 and y < ends[t] else -1,)
    return cover(payload, begins + ends, member)


# ---------------------------------------------------------------- what a cover leaves behind
class Outcome:
    """What the GPU module compares: `windows` [(lo, hi, uint8 bytes)], `stray` (constant-region
    elements that differ from the host-computed constant), `sums`, `veto` (None where not applicable)."""

    def __init__(self, windows=None, stray=None, sums=None, veto=None):
        self.windows, self.stray, self.sums, self.veto = windows, stray, sums, veto


def _pieces(cov, lo, hi):
    return [(max(lo, a), min(hi, b)) + tuple(rest) for a, b, *rest in cov if max(lo, a) < min(hi, b)]


def lerp_const(P, Q, f=FACTOR):
    """The averaged constant, per element type."""
    return {d: fref.lerp(d, [P.const[d]], [Q.const[d]], f)[0] for d in P.payload.dtypes}


def _lerp_value(P, Q, f, fill):
    """value(lo, hi, k, dtype) of the bytes an average leaves in a destination: `fill` None for the
    parameters averaged in place (k times), else the byte an unreached destination keeps."""
    def value(lo, hi, k, dtype):
        p, q = P.bytes(lo, hi), Q.bytes(lo, hi)
        if k == 0:
            return p if fill is None else np.full(hi - lo, fill, dtype=np.uint8)
        v = as_bits(dtype, p)
        for _ in range(k if fill is None else 1):
            v = fref.lerp(dtype, v, as_bits(dtype, q), f)
        return v.view(np.uint8)
    return value


def _copy_value(S, fill):
    def value(lo, hi, k, dtype):
        return S.bytes(lo, hi) if k else np.full(hi - lo, fill, dtype=np.uint8)
    return value


def leave(payload, cov, value, want_const):
    """The Outcome (windows, stray) of a destination whose bytes are value(lo, hi, k, dtype) per piece
    of `cov`; want_const[dtype]: the constant the right kernel leaves."""
    if cov == OUTSIDE:
        return OUTSIDE
    wins = []
    for lo, hi in payload.wins:
        out = np.empty(hi - lo, dtype=np.uint8)
        for a, b, k, d in _pieces(cov, lo, hi):
            out[a - lo:b - lo] = value(a, b, k, d)
        wins.append((lo, hi, out))
    stray = 0
    for lo, hi in payload.gaps():
        for a, b, k, d in _pieces(cov, lo, hi):
            for true, x, y in payload.split(a, b):
                want = np.array([want_const[true]], dtype=NUMPY[true])
                if y - x <= 8192:
                    stray += int((as_bits(true, value(x, y, k, d)) != want).sum())
                    continue
                head = x + (-x) % 16 + 16                     # one aligned item stands for the piece's items
                stray += int((as_bits(true, value(x, head, k, d)) != want).sum())
                bad = int((as_bits(true, value(head, head + 16, k, d)) != want).sum())
                items = (y - head) // 16
                stray += bad * items
                stray += int((as_bits(true, value(head + 16 * items, y, k, d)) != want).sum())
    return Outcome(windows=wins, stray=stray)


def average(payload, P, Q, cov, f=FACTOR, through=False, resident=False):
    """{"param": Outcome, "snap": Outcome}: an average in place (and written through to a snapshot), or
    the resident form, which leaves the parameters and writes the snapshot alone."""
    want = lerp_const(P, Q, f)
    out = {}
    if resident:
        out["param"] = leave(payload, right_cover(payload), _copy_value(P, FILL), P.const)
    else:
        out["param"] = leave(payload, cov, _lerp_value(P, Q, f, None), want)
    if through or resident:
        if resident or cov == OUTSIDE:
            out["snap"] = leave(payload, cov, _lerp_value(P, Q, f, FILL), want)
        else:       # the write-through copy of what the in-place average stored
            out["snap"] = leave(payload, cov, lambda lo, hi, k, d: (_lerp_value(P, Q, f, None)(lo, hi, k, d) if k else
                                                                    np.full(hi - lo, FILL, dtype=np.uint8)), want)
    return OUTSIDE if any(v == OUTSIDE for v in out.values()) else out


def moved(payload, S, cov, fill=FILL):
    """A byte mover's destination, which held `fill` before."""
    return leave(payload, cov, _copy_value(S, fill), S.const)


def _terms(dtype, p_raw, q_raw):
    p, q = decode(dtype, as_bits(dtype, p_raw)), decode(dtype, as_bits(dtype, q_raw))
    return float(((q - p) ** 2).sum()), float((p * p).sum())


def sums(payload, P, Q, cov, members=None):
    """(dist2, norm2) of the exact family under a cover -- or, with `members` (table_members), one pair
    per tensor.  Exact: every partial sum is a multiple of 2^-2 below 2^53 * 2^-2."""
    if cov == OUTSIDE:
        return OUTSIDE
    whole = members is None
    members = [(0, payload.nbytes, 0)] if whole else members
    tot = [[0.0, 0.0] for _ in range(1 if whole else len(TENSORS))]
    for lo, hi, k, d in cov:
        if k == 0:
            continue
        for a, b, t in _pieces(members, lo, hi):
            if t < 0:
                continue
            edges = [a] + [x for w in payload.wins for x in w if a < x < b] + [b]
            for x, y in zip(edges, edges[1:]):
                if any(w[0] <= x < w[1] for w in payload.wins) or y - x <= 8192:
                    d2, n2 = _terms(d, P.bytes(x, y), Q.bytes(x, y))
                else:           # constants: one element's terms times the elements
                    e2, m2 = _terms(d, P.bytes(x, x + SIZE[d]), Q.bytes(x, x + SIZE[d]))
                    d2, n2 = e2 * ((y - x) // SIZE[d]), m2 * ((y - x) // SIZE[d])
                tot[t][0] += k * d2
                tot[t][1] += k * n2
    return tuple(tot[0]) if whole else [tuple(t) for t in tot]


def veto(payload, Q, cov):
    """Does the finite check of the peer `Q` veto?"""
    if cov == OUTSIDE:
        return OUTSIDE
    for lo, hi, k, d in cov:
        if k == 0:
            continue
        edges = [lo] + [x for w in payload.wins for x in w if lo < x < hi] + [hi]
        for x, y in zip(edges, edges[1:]):
            y = y if any(w[0] <= x < w[1] for w in payload.wins) or y - x <= 8192 else x + 16
            if finite_ref.vetoes(d, as_bits(d, Q.bytes(x, y))):
                return True
    return False


def finite_positions(payload):
    """{name: byte offset} of the elements a non-finite pattern is planted at."""
    out = {}
    for d, a, b in payload.segs:
        s = SIZE[d]
        if a:
            out["first-of-%s-segment" % d] = a
        for name, at in (("last-below-2^31", L31 - s), ("first-at-2^31", L31), ("last-below-2^32", L32 - s),
                         ("first-at-2^32", L32)):
            if a <= at < b:
                out[name] = at
    d, a, b = payload.segs[-1]
    out["first-of-last-whole-item"] = b // 16 * 16 - 16
    out["last-element"] = b - SIZE[d]
    return out


def finite_plants(payload, Q):
    """[(name, peer)]: the finite peer as it is (no veto), then with one finite_ref.BAD pattern at one
    of finite_positions at a time (a veto each)."""
    out = [(("finite",), Q)]
    for where, at in finite_positions(payload).items():
        d = payload.split(at, at + 1)[0][0]
        out += [((where, kind), Q.planted(at, d, bits)) for kind, bits in finite_ref.BAD[d].items()]
    return out


# ---------------------------------------------------------------- the checks
def failures(payload, got, want, exact_bytes=False):
    """The checks `got` fails against the reference `want` (Outcomes, or dicts of them per
    destination): "windows" (NaN positions coincide, every other element bit-equal; byte-equal for the
    byte movers), "stray", "sums", "veto".  OUTSIDE fails all of them."""
    if isinstance(want, dict):
        if got == OUTSIDE:
            return ["outside"]
        return sorted({"%s:%s" % (k, f) for k in want for f in failures(payload, got[k], want[k], exact_bytes)})
    if got == OUTSIDE:
        return ["outside"]
    out = []
    if want.windows is not None:
        for (lo, hi, g), (_, _, w) in zip(got.windows, want.windows):
            for d, a, b in payload.split(lo, hi):
                gb, wb = g[a - lo:b - lo], w[a - lo:b - lo]
                ok = np.array_equal(gb, wb) if exact_bytes else fref.same(d, as_bits(d, gb), as_bits(d, wb))
                if not ok:
                    out.append("windows")
    if want.stray is not None and got.stray != want.stray:
        out.append("stray")
    if want.sums is not None and got.sums != want.sums:
        out.append("sums")
    if want.veto is not None and got.veto != want.veto:
        out.append("veto")
    return sorted(set(out))


# ---------------------------------------------------------------- the cases of the GPU module
# (name, payload maker, kernel family, operation, operand family): what tests/test_gpu_big.py runs and
# tests/test_big_host.py runs every mutant through
CASES = [(("lerp", d), lambda d=d: single(d), "span", "lerp", "hard") for d in fref.DTYPES]
CASES += [(("average", d), lambda d=d: single(d), "span", "lerp", "hard") for d in ("bf16", "f32")]
CASES += [(("average-unaligned", "bf16"), lambda: single("bf16"), "elem", "lerp", "hard")]
CASES += [(("tracked", d), lambda d=d: single(d), "span", "tracked", "exact") for d in ("bf16", "f32")]
CASES += [(("average-mixed",), mixed, "span", "lerp", "hard")]
CASES += [(("resident", "bf16"), lambda: single("bf16"), "span", "lerp", "hard")]
CASES += [(("distance", d), lambda d=d: single(d), "span", "sums", "exact") for d in ("bf16", "f32")]
CASES += [(("distance-unaligned", d), lambda d=d: single(d), "elem", "sums", "exact") for d in ("bf16", "f32")]
CASES += [(("distance-mixed",), mixed, "span", "sums", "exact")]
CASES += [(("param-distance",), tabled, "span", "table", "exact")]
CASES += [(("finite", d), lambda d=d: single(d), "span", "finite", "finite") for d in fref.DTYPES]
CASES += [(("finite-unaligned", d), lambda d=d: single(d), "elem", "finite", "finite") for d in fref.DTYPES]
CASES += [(("finite-mixed",), mixed, "span", "finite", "finite")]
CASES += [(("copy", "bf16"), lambda: single("bf16"), "span", "copy", "hard")]


def model(payload, family, op, fam, name=None, P=None, Q=None):
    """The outcome of a case under the slip `name` (None: the right kernel); None where the slip cannot
    live in the case's kernel."""
    if P is None:
        P, Q = operands(payload, fam)
    if op == "table":
        if name == "param-row-payload-span":
            astray = table_rows(TENSORS, name)
            assert astray and all(o == OUTSIDE for _, _, o in astray)      # at this table: behind the workspace
            return OUTSIDE
        if name not in (None, "table-begins-32-bit"):
            cov = mutant_cover(payload, family, "sums", name)
            if cov is None:
                return None
            return Outcome(sums=sums(payload, P, Q, cov, table_members(payload, TENSORS))) if cov != OUTSIDE else OUTSIDE
        return Outcome(sums=sums(payload, P, Q, right_cover(payload), table_members(payload, TENSORS, name)))
    cov = right_cover(payload) if name is None else mutant_cover(payload, family, "sums" if op == "tracked" else op, name)
    if cov is None:
        return None
    if op == "lerp":
        return average(payload, P, Q, cov, through=True)
    if op == "tracked":
        out = average(payload, P, Q, cov, through=True)
        if out == OUTSIDE:
            return OUTSIDE
        out["record"] = Outcome(sums=sums(payload, P, Q, cov))
        return out
    if op == "copy":
        return moved(payload, P, cov)
    if op == "sums":
        s = sums(payload, P, Q, cov)
        return OUTSIDE if s == OUTSIDE else Outcome(sums=s)
    if cov == OUTSIDE:
        return OUTSIDE
    return Outcome(veto=tuple(veto(payload, peer, cov) for _, peer in finite_plants(payload, Q)))


# ---------------------------------------------------------------- the reuse guard and the window guard
# (kernels.hip guard_base / guard_offset over n16 words; tests/moves_ref.py holds the model on whole
# host arrays, which these sizes do not allow: here the snapshot and the parameters differ at the
# written bytes only, so what a guarded publish must leave is the set of written bytes it takes over)
GUARD_SAMPLES = 4096
GUARD_MUTANTS = {
    "guard-base-32-bit": "guard_base's product k * (n16 - 1) in 32 bits (it overflows from k = 16 at this size)",
    "chunk-bounds-32-bit": "a dirty chunk's byte bounds (words << 4) kept in 32 bits",
}
MUTANTS.update(GUARD_MUTANTS)


def _guard_bases(n16, name=None):
    """b(0..s-1) and the last word: chunk k is words [b(k), b(k+1)), the last chunk the last word alone."""
    s = min(n16, GUARD_SAMPLES)
    if s <= 1:
        return [0, n16]
    prod = (lambda k: (k * (n16 - 1)) & (L32 - 1)) if name == "guard-base-32-bit" else (lambda k: k * (n16 - 1))
    return [prod(k) // (s - 1) if s == GUARD_SAMPLES else k for k in range(s - 1)] + [n16 - 1, n16]


def guard_sampled(n16, gen, name=None):
    """[(sampled word, (lo, hi) words of its chunk)] per chunk at generation `gen`."""
    b = _guard_bases(n16, name)
    out = []
    for k in range(len(b) - 1):
        length = b[k + 1] - b[k]
        out.append((b[k] + (gen % length if length > 0 else 0), (b[k], b[k + 1])))
    return out


def guard_words(n16, gen, chunk_of):
    """The words written around the chunk holding word `chunk_of`: its sampled word, both its end words
    (copied with it) and the words just outside it (in chunks whose samples lie elsewhere)."""
    hit, (lo, hi) = next((w, c) for w, c in guard_sampled(n16, gen) if c[0] <= chunk_of < c[1])
    return sorted({hit, lo, hi - 1, lo - 1, hi} - {-1, n16})


def guard_model(nbytes, gen, written, name=None):
    """(the written byte offsets a guarded reusing publish of generation `gen` takes into the snapshot,
    hit): a chunk is copied when its sampled word (chunk 0: or the first word) holds a written byte, and
    every written tail byte is."""
    n16, tail = nbytes // 16, nbytes % 16
    written = sorted(int(o) for o in written)
    words = {o // 16 for o in written if o < n16 * 16}
    taken = {o for o in written if o >= n16 * 16}
    hit = bool(taken)
    for k, (w, (lo, hi)) in enumerate(guard_sampled(n16, gen, name)):
        if w in words or (k == 0 and 0 in words):
            hit = True
            lo, hi = lo * 16, hi * 16
            if name == "chunk-bounds-32-bit":
                lo, hi = lo & (L32 - 1), hi & (L32 - 1)
            taken |= {o for o in written if lo <= o < hi}
    assert tail or not any(o >= n16 * 16 for o in written)
    return sorted(taken), hit


def window_model(nbytes, gen, written, name=None):
    """Must the window guard count a window in which `written` bytes changed: a word sampled at `gen`,
    the first word, the last word or a tail byte among them."""
    n16 = nbytes // 16
    compared = {w for w, _ in guard_sampled(n16, gen, name)} | {0, n16 - 1}
    return any(o >= n16 * 16 or o // 16 in compared for o in written)


def guard_case(nbytes, gen, two_chunks_only=False):
    """The words written before the guarded publish of `gen`: around the chunks holding words 2^27 and
    2^28 (the second lies beyond byte 2^32), and the tail.  two_chunks_only (the byte form, which
    copies a dirty chunk in one thread): without the last word, a chunk of its own behind the second."""
    n16 = nbytes // 16
    words = guard_words(n16, gen, 1 << 27) + guard_words(n16, gen, 1 << 28) + [n16]
    return [w for w in words if not (two_chunks_only and w == n16 - 1)]


def window_cases(nbytes):
    """[(gen, words)] of a resident learner's three windows: unsampled words of the two chunks (no
    hit), the sampled word of the chunk beyond byte 2^32 (a hit), the tail alone (a hit)."""
    n16 = nbytes // 16
    out = []
    for gen in (1, 2, 3):
        far = next((w, c) for w, c in guard_sampled(n16, gen) if c[0] <= (1 << 28) < c[1])
        near = next((w, c) for w, c in guard_sampled(n16, gen) if c[0] <= (1 << 27) < c[1])
        if gen == 1:
            words = [near[0] + 1, far[0] + 1]
        elif gen == 2:
            words = [far[0]]
        else:
            words = [n16]
        out.append((gen, words))
    return out


# ---------------------------------------------------------------- the relay
# (kernels.hip k_relay_phase1 / k_relay_phase2 / StripeSrc: every payload, rounded up to 16 bytes, is cut
# into `world` stripes of whole pages; a gathered round copies every stripe of the pick's snapshot into the
# staging buffer, from the pick's slot or from a relay buffer; the fused round's averaging kernel reads
# each 1-KiB span where the gather would have)
RELAY_WORLD, RELAY_PICKS, RELAY_FORMS, RELAY_BLOCKS = 2, (1, 0), ("gather", "fused"), 256
RELAY_FILL = 0xC3                 # relay_ref.SENTINEL: the staging buffer before the gather
RELAY_MUTANTS = {
    "stripe-begin-signed-32-bit": "a stripe's begin s * stripe in a signed 32-bit product",
    "stripe-length-32-bit": "the payload's bytes kept in 32 bits where a stripe's length is clamped to them",
    "stripe-span-mod-2^32": "StripeSrc::span_of's byte offset kept in 32 bits (the fused form)",
}
MUTANTS.update(RELAY_MUTANTS)


def relay_stripe(nbytes, world=RELAY_WORLD):
    """dpwa_learner_relay_enable: the payload rounded up to 16 bytes, split evenly, in whole pages."""
    p16 = (nbytes + 15) // 16 * 16
    return (-(-p16 // world) + 4095) // 4096 * 4096


def relayed():
    """The bf16 payload with a window at every stripe border."""
    nbytes = N["bf16"] * 2
    stripe = relay_stripe(nbytes)
    return single("bf16", borders=[s * stripe for s in range(1, RELAY_WORLD) if s * stripe < nbytes])


def relay_cover(payload, form, name=None):
    """The cover of a relay round: which bytes the gather copies (form "gather") or the fused average
    reaches (form "fused"); OUTSIDE; None where the slip cannot live in that form or changes nothing."""
    nb, d = payload.nbytes, payload.dtype
    stripe, body = relay_stripe(nb), nb // 16 * 16
    right = right_cover(payload)
    if name is None:
        return right
    if name == "stripe-begin-signed-32-bit":
        return OUTSIDE if any(s * stripe >= L31 for s in range(RELAY_WORLD) if s * stripe < nb) else None
    if name == "stripe-length-32-bit":
        seen = ((nb + 15) // 16 * 16) & (L32 - 1)          # stripes beginning at or behind it are empty
        out = cover(payload, [seen], lambda y: ((1 if y < seen else 0), d))
    elif name == "stripe-span-mod-2^32":
        if form != "fused" or body <= L32:
            return None
        w = body - L32
        out = cover(payload, [w, L32, body], lambda y: ((2 if y < w else 1 if y < L32 else 0 if y < body else 1), d))
    else:
        return mutant_cover(payload, "span", "lerp" if form == "fused" else "copy", name) if form == "fused" else None
    return None if out == right else out


def relay_model(payload, mine, peer, form, name=None):
    """{"staged": what the gather leaves in the staging buffer (form "gather" only), "param": the
    averaged parameters}, or OUTSIDE, or None."""
    cov = relay_cover(payload, form, name)
    if cov is None or cov == OUTSIDE:
        return cov
    out = {}
    if form == "gather":            # the average that follows reads the staging buffer: bytes never gathered are the fill
        out["staged"] = moved(payload, peer, cov, RELAY_FILL)
        staged = Operand(payload, {d: NUMPY[d](int(np.full(SIZE[d], RELAY_FILL, dtype=np.uint8).view(NUMPY[d])[0]))
                                   for d in payload.dtypes}, [w for _, _, w in out["staged"].windows])
        q = peer if cov == right_cover(payload) else staged
        out["param"] = average(payload, mine, q, right_cover(payload))["param"]
        if q is staged:             # the constant region behind what was gathered averages with the fill
            gone = [(lo, hi) for lo, hi, k, _ in cov if k == 0]
            out["param"].stray += sum((hi - lo) // SIZE[payload.dtype] for lo, hi in gone)
    else:
        out["param"] = average(payload, mine, peer, cov)["param"]
    return out
