"""What the per-parameter distance to the peer must be, for tests/test_pdist_host.py and
tests/test_gpu_pdist.py.

The quantity (include/dpwa_hip.h ``dpwa_param_range``): tests/dist_ref.py's two sums for every
parameter tensor over that tensor's own elements only; bytes of no tensor enter no sum.  The
reference slices each tensor out of the payload bytes and hands it to ``dist_ref`` (``widen``,
``terms``, ``fsum``); the tolerance is ``dist_ref.bound(n_t)``, checked with ``dist_ref.problem``.

``model`` is the pass and its finishing step as the kernels are specified (1-KiB spans, 256-byte
quarters, tensor t's span s into row s mod rows_t, rows summed and zeroed), in float64 numpy; with a
``mutant`` it is one of the wrong kernels the tests must be able to tell from the right one.
Nothing here calls the GPU library or torch on a device.
"""
import numpy as np

from tests import dist_ref

SPAN, QUARTER, ITEM_BYTES, ALIGN, SEGMENT = 1024, 256, 16, 256, 4096
MUTANTS = ("quarter-to-neighbour", "gap-counted", "last-item-dropped", "last-item-overcounted",
           "payload-span-row", "rows-not-zeroed")
CASE_NAMES = ("normal", "equal", "last-element", "huge-opposite-signs", "subnormal-differences", "signed-zeros",
              "one-nan", "one-inf")


class Layout:
    """`tensors`: [(name, dtype, byte offset, byte length)] ascending; `payload`: "f32" / "bf16" /
    "f16" or "mixed" with `segments` [(dtype, byte offset, byte length)]."""

    def __init__(self, name, payload, total_bytes, tensors, segments=None):
        self.name, self.payload, self.total_bytes = name, payload, total_bytes
        self.tensors, self.segments = list(tensors), segments

    def elements(self, t):
        return self.tensors[t][3] // dist_ref.SIZE[self.tensors[t][1]]


def _up(x, to):
    return (x + to - 1) // to * to


def single(name, dtype, sizes):
    """A single-dtype payload as dpwa_amd/flat.py lays it out: every tensor on a 256-byte boundary;
    the payload ends with the last tensor's 256-byte slot."""
    size, off, tensors = dist_ref.SIZE[dtype], 0, []
    for i, n in enumerate(sizes):
        tensors.append(("t%d" % i, dtype, off, n * size))
        off += _up(n * size, ALIGN)
    return Layout(name, dtype, off, tensors)


def ragged(name, dtype, sizes):
    """The same, the payload ending with the last tensor's last element (inside a 16-byte item)."""
    lay = single(name, dtype, sizes)
    lay.total_bytes = lay.tensors[-1][2] + lay.tensors[-1][3]
    return lay


def mixed(name, by_dtype):
    """A segmented payload as dpwa_amd/flat.py lays it out: `by_dtype` {dtype: sizes}; segments in
    the order f32, bf16, f16, each a whole number of 4-KiB blocks."""
    off, tensors, segments = 0, [], []
    for dtype in dist_ref.DTYPES:
        if dtype not in by_dtype:
            continue
        begin = off
        for i, n in enumerate(by_dtype[dtype]):
            b = n * dist_ref.SIZE[dtype]
            tensors.append(("%s_%d" % (dtype, i), dtype, off, b))
            off += _up(b, ALIGN)
        off = _up(max(off, begin + 1), SEGMENT)
        segments.append((dtype, begin, off - begin))
    return Layout(name, "mixed", off, tensors, segments)


A_SIZES = [1, 63, 64, 65, 0, 256, 257]
A16_SIZES = [1, 127, 128, 129, 0, 512, 513]
M_SIZES = {"f32": [1, 65], "bf16": [129, 512], "f16": [1]}


def layout_a():
    return single("A", "f32", A_SIZES)


def layout_a16(dtype):
    return single("A16-" + dtype, dtype, A16_SIZES)


def layout_b(max_rows, dtype="f32"):
    """One tensor of (3 R + 2) spans plus an item and one element, then a 1-element neighbour."""
    return ragged("B", dtype, [dist_ref.many_spans(dtype, max_rows), 1])


def layout_m():
    return mixed("M", M_SIZES)


def small_layouts():
    return [layout_a(), layout_a16("bf16"), layout_a16("f16"), layout_m()]


# ---------------------------------------------------------------- payloads
def gap_mask(lay):
    """True for the payload bytes that belong to no tensor."""
    m = np.ones(lay.total_bytes, dtype=bool)
    for _, _, off, length in lay.tensors:
        m[off:off + length] = False
    return m


def payload(lay, per_tensor, fill=0):
    """The payload bytes (uint8) with tensor t holding the bit patterns per_tensor[t]; gap bytes
    `fill` (0x7f and 0xff both make NaN patterns of every dtype when they fill a whole element)."""
    out = np.full(lay.total_bytes, fill, dtype=np.uint8)
    for (_, dtype, off, length), bits in zip(lay.tensors, per_tensor):
        out[off:off + length] = np.ascontiguousarray(bits, dtype=dist_ref.BITS[dtype]).view(np.uint8)
    return out


def tensor_bits(lay, t, data):
    _, dtype, off, length = lay.tensors[t]
    return np.ascontiguousarray(data[off:off + length]).view(dist_ref.BITS[dtype])


_CASES = {}


def tensor_case(dtype, n, case, seed):
    """(p_bits, q_bits) of dist_ref.cases(dtype, n)'s input set `case` (empty tensors: empty)."""
    if n == 0:
        e = np.zeros(0, dtype=dist_ref.BITS[dtype])
        return e, e
    key = (dtype, n, seed)
    if key not in _CASES:
        _CASES[key] = {name: (p, q) for name, p, q in dist_ref.cases(dtype, n, seed=seed)}
    return _CASES[key][case]


def inputs(lay, case, victim=None, base="normal", fill=0):
    """(param bytes, peer bytes): every tensor holds its own input set `case`; with `victim` only that
    tensor does and every other tensor holds `base`."""
    ps, qs = [], []
    for t, (_, dtype, _, _) in enumerate(lay.tensors):
        name = case if victim is None or t == victim else base
        p, q = tensor_case(dtype, lay.elements(t), name, seed=t)
        ps.append(p)
        qs.append(q)
    return payload(lay, ps, fill), payload(lay, qs, fill)


# ---------------------------------------------------------------- the reference
def reference(lay, p, q):
    """[(dist2, norm2)] per tensor, exactly rounded; (0, 0) for an empty tensor."""
    out = []
    for t, (_, dtype, _, _) in enumerate(lay.tensors):
        out.append(dist_ref.reference(dtype, tensor_bits(lay, t, p), tensor_bits(lay, t, q))
                   if lay.elements(t) else (0.0, 0.0))
    return out


def problems(lay, got, ref):
    """The tensors whose pair misses dist_ref's rule, as text; empty when all meet it."""
    out = []
    for t in range(len(lay.tensors)):
        for k, what in enumerate(("dist2", "norm2")):
            why = dist_ref.problem(float(got[t][k]), ref[t][k], max(lay.elements(t), 1))
            if why:
                out.append("%s tensor %d (%s) %s: %s" % (lay.name, t, lay.tensors[t][0], what, why))
    return out


# ---------------------------------------------------------------- the kernels' model
def rows_of(lay, max_rows):
    """[(first_row, rows)] per tensor and the rows in all."""
    out, first = [], 0
    for _, _, off, length in lay.tensors:
        spans = (_up(off + length, SPAN) // SPAN - off // SPAN) if length else 0
        r = min(spans, max_rows)
        out.append((first, r))
        first += r
    return out, first


def _sums(dtype, p, q, lo, hi):
    """The two float64 sums over payload bytes [lo, hi) read as `dtype` (whole elements)."""
    if hi <= lo:
        return 0.0, 0.0
    bits = dist_ref.BITS[dtype]
    d, n = dist_ref.terms(dtype, np.ascontiguousarray(p[lo:hi]).view(bits), np.ascontiguousarray(q[lo:hi]).view(bits))
    with np.errstate(all="ignore"):
        return float(np.sum(d)), float(np.sum(n))


def model(lay, p, q, max_rows, mutant=None, rows=None):
    """(the record [(dist2, norm2)], the rows as the call leaves them).  `rows`: the accumulator rows
    as an earlier call left them (None: zero)."""
    assert mutant is None or mutant in MUTANTS
    table, total_rows = rows_of(lay, max_rows)
    acc = np.zeros((max(total_rows, 1), 2)) if rows is None else rows.copy()
    live = [t for t in range(len(lay.tensors)) if lay.tensors[t][3]]
    for at, t in enumerate(live):
        _, dtype, begin, length = lay.tensors[t]
        end, size = begin + length, dist_ref.SIZE[dtype]
        next_begin = lay.tensors[live[at + 1]][2] if at + 1 < len(live) else lay.total_bytes
        first_span = begin // SPAN
        for s in range(first_span, _up(end, SPAN) // SPAN):
            whole = begin <= s * SPAN and end >= (s + 1) * SPAN
            for k in range(SPAN // QUARTER):
                lo = max(s * SPAN + k * QUARTER, begin)
                hi = min(s * SPAN + (k + 1) * QUARTER, end)
                if hi <= lo:
                    continue
                last = hi == end
                if mutant == "gap-counted" and last:        # the gap behind the tensor, as far as the quarter goes
                    hi = min(_up(end, QUARTER), next_begin, lay.total_bytes) // size * size
                if mutant == "last-item-dropped" and last and end % ITEM_BYTES:
                    hi = end // ITEM_BYTES * ITEM_BYTES
                if mutant == "last-item-overcounted" and last and end % ITEM_BYTES:
                    hi = min(_up(end, ITEM_BYTES), lay.total_bytes) // size * size
                d2, n2 = _sums(dtype, p, q, lo, hi)
                first, r = table[t]
                row = first + (s - first_span) % r
                if mutant == "payload-span-row":
                    row = (first + s % max_rows) % total_rows
                if mutant == "quarter-to-neighbour" and not whole and k > 0 and at > 0:
                    first, r = table[live[at - 1]]          # the tensor of the quarter before
                    row = first + (s - lay.tensors[live[at - 1]][2] // SPAN) % r
                acc[row, 0] += d2
                acc[row, 1] += n2
    record = []
    for first, r in table:
        with np.errstate(all="ignore"):
            record.append((float(np.sum(acc[first:first + r, 0])), float(np.sum(acc[first:first + r, 1]))))
    if mutant != "rows-not-zeroed":
        acc[:] = 0.0
    return record, acc
