"""A host model of a group of learners, for walks over the call orders the C ABI allows:
tests/test_walk_host.py (no GPU) and tests/test_gpu_walk.py.

The model holds, per learner, exactly what a caller of include/dpwa_hip.h can observe -- the
parameter bits of its flat buffers, both snapshot slots (header fields and payload), the version, the
live clock, the last dpwa_coef, where resident parameters are, the whole-model distance record -- and
the bookkeeping behind it that the caller cannot see but that decides the next call: the four-deep
clock ring and ``cur``, the fetch in flight (source learner, slot, copied or in place, fetched or
factored), the pending written-through snapshot (for which ``flat``, with or without its header).
An operation is a tuple (``OPS`` below); ``Model.apply(op)`` returns the expected return code and
moves the state, and a refused call moves nothing.

The two opt-ins that keep state between calls are in the model too: the non-finite peer check (its
switch, the skip counter, the sticky status word, DPWA_STATUS_PEER_NONFINITE in the coefficients) and the
per-parameter distance (its record, ``every`` and the two host counters).  A walk reaches them only when
its ``Spec`` asks (``draws``); a learner's parameters are poisoned and healed with the ``step`` op, whose
bits ``poisoned`` and ``healed`` make from what the model holds.  Whether a payload vetoes comes from
``tests/finite_ref`` and the per-tensor sums from ``tests/pdist_ref``.

No arithmetic is restated here.  The factor, the status and the clock come from
``oracle.policy.factor_and_clock`` as ``tests/factor_ref.evaluate`` reads it; the averaged bits from
``tests/forms_ref.lerp`` (``oracle.lerp``, ``tests/f16_ref``) and ``tests/mixed_ref.lerp``; the
distance record from ``tests/dist_ref``.  Nothing here touches a GPU.

The walks fetch the peer's current version (and, for the refusals, version 0 and a slot never
published); the sequence "previous-version" fetches the version before it while its owner has no
written-through snapshot pending, which holds a reader on the very slot the owner rewrites next.  A
caller that names an older version while a write-through is pending reads a slot its owner has already
written into, which the ABI leaves to the caller (dpwa_hip.h, dpwa_learner_fetch: the events protect a
slot from the readers its owner knows, not from one that arrives later); no walk does that.

On the hard bit patterns every distance sum is NaN or infinite, which says nothing about the operands the
record was taken from; `Spec(finite=True)` gives finite operands, on which the record is held to
dist_ref.bound: one walk per profile and the distance sequences use them.

A mutant "average_many commits in reverse order" would not be observable: average_commit
(learner.cpp) touches only its own learner's bookkeeping, so any order of commits leaves the same
state.  What IS observable about dpwa_learner_average_many's order is that every learner is prepared
before any is committed -- a learner whose write-through slot an earlier learner of the same call
still reads is refused, where one call after another would pass -- and the mutant
``many-one-by-one`` stands for it.
"""
import copy
import math
import random

import numpy as np

from tests import dist_ref, factor_ref, finite_ref, mixed_ref, pdist_ref
from tests import forms_ref as fref

OK, ERR_ARG, ERR_STATE = 0, -1, -3
METHOD_CODE = {"constant": 0, "clock": 1, "loss": 2}
MIXED_CODE = 4
FETCH_KINDS = ("ce", "k1", "k512", "zc")      # copy engine, DPWA_PULL_KERNEL with 1 / 512 blocks, zero copy
MAIN = ("publish", "publish_reuse", "fetch", "factor", "lerp", "average", "average_through", "cancel", "relocate",
        "write_clock")
OTHER = ("average_many", "copy_fetched", "copy_factor", "read_snapshot", "set_distance", "set_header_publish",
         "set_resident", "step", "set_finite_check", "set_param_distance")
OPS = MAIN + OTHER
AVERAGING = ("lerp", "average", "average_through", "average_many")
MIXED_SPEC = (("f32", 261), ("bf16", 521))     # two segments of one 4-KiB block each: 8 KiB
SIZES = {"f32": 261, "bf16": 521, "f16": 521, "mixed": 8192}   # one 1-KiB span and a ragged tail
DTYPES = ("f32", "bf16", "f16", "mixed")
STATUS_ZD, STATUS_SKIPPED = 1, 2               # DPWA_STATUS_ZERO_DIVISION, DPWA_STATUS_PEER_NONFINITE

# The parameter tensors of dpwa_learner_set_param_distance, one fixed list per dtype (elements; pdist_ref lays
# each on a 256-byte boundary): tensor 0 ends inside the first 1-KiB span, tensor 1 is empty, tensor 2 ends
# 112 bytes before tensor 3 begins (a gap, like the 16 bytes behind tensor 0), tensor 3 crosses the span
# boundary and ends with the payload's ragged tail.  A segmented payload holds the same four in each segment.
PARAM_SIZES = {"f32": (60, 0, 100, 69), "bf16": (120, 0, 200, 137), "f16": (120, 0, 200, 137)}
GAP_ELEMENT = {"f32": 170, "bf16": 340, "f16": 340}     # byte 680: between tensors 2 and 3
# Where a walk poisons a payload: name -> (segment dtype or None, element index)
POISON_AT = {d: {"first": (None, 0), "span-last": (None, finite_ref.SPAN[d] - 1), "tail-last": (None, SIZES[d] - 1),
                 "gap": (None, GAP_ELEMENT[d])} for d in ("f32", "bf16", "f16")}
POISON_AT["mixed"] = {"f32-first": ("f32", 0), "bf16-last": ("bf16", 520), "f32-gap": ("f32", GAP_ELEMENT["f32"])}
POISON_KINDS = ("snan", "qnan", "+inf", "-inf")

# The refusal rules: name -> (return code, file, a fragment of the line that decides it: its condition, or
# the name of its message).  tests/test_walk_host.py checks that every cited fragment is in the file.
# (One line of average_prepare decides both average-without-fetch and average-after-factor.)
H, LC, FH, MH = "include/dpwa_hip.h", "dpwa_amd/csrc/learner.cpp", "dpwa_amd/csrc/fetch.hpp", "dpwa_amd/csrc/measure.hpp"
RULES = {
    "factor-without-fetch": (ERR_STATE, LC, '"dpwa_learner_factor: no fetch in flight"'),
    "factor-twice": (ERR_STATE, LC, '"dpwa_learner_factor: factor already computed'),
    "lerp-without-factor": (ERR_STATE, LC, '"dpwa_learner_lerp: no factor computed'),
    "lerp-resident": (ERR_STATE, LC, '"dpwa_learner_lerp: a resident learner averages with'),
    "average-without-fetch": (ERR_STATE, LC, "if (!l->fetch.fetched() || l->fetch.factored())"),
    "average-after-factor": (ERR_STATE, LC, "if (!l->fetch.fetched() || l->fetch.factored())"),
    "copy-fetched-without-fetch": (ERR_STATE, LC, '"dpwa_learner_copy_fetched: no fetch in flight"'),
    "relocate-with-fetch": (ERR_STATE, LC, '"dpwa_learner_relocate: a fetch is in flight'),
    "resident-publish-pointer": (ERR_ARG, LC, '"resident learner: publish the parameters where they are'),
    "resident-average-pointer": (ERR_ARG, LC, '"resident learner: average the parameters where they are'),
    "resident-not-in-next-slot": (ERR_STATE, LC, '"resident learner: parameters not in the next slot"'),
    "slot-still-read": (ERR_STATE, LC, "if (r->fetch.reads(l, k))"),
    "reads-any-kind": (None, FH, "return fetched() && src_.owner == owner && src_.slot == slot;"),
    "fetch-version-0": (ERR_STATE, LC, "if (peer_version == 0)"),
    "fetch-slot-never-published": (ERR_STATE, LC, "if (!pl->published[k].noted())"),
    "set-resident-twice": (ERR_STATE, LC, '"dpwa_learner_set_resident: already resident"'),
    "set-resident-late": (ERR_STATE, LC, "if (l->version != 0 || l->fetch.fetched())"),
    # a checking learner's split round: the pass ran in the factor, on the snapshot then in flight
    "fetch-over-checked-factor": (ERR_STATE, LC, "if (l->finite_check && l->fetch.factored())"),
    "set-check-over-factor": (ERR_STATE, LC, "if (on && l->fetch.factored())"),
    # average_prepare and dpwa_learner_lerp ask Measure::operands_problem behind their state and layout
    # refusals and before the resident pointer and the slot's readers
    "param-unaligned": (ERR_ARG, MH, "if (!param_ || aligned16(flat)) return DPWA_OK;"),
    # not refusals: what the model keeps because the code does
    "second-fetch-keeps-factor": (None, FH, "if (phase_ == Phase::None) phase_ = Phase::Fetched;"),
    "write-clock-drops-header": (None, LC, "l->wt_header = false;   // the next header was written from the old clock"),
    "factor-drops-header": (None, LC, "l->wt_header = false;   // (as dpwa_learner_write_clock does"),
    "no-op-round-writes-snapshot": (None, "dpwa_amd/csrc/kernels.hip", "if (MODE == COEF_FUSED && DUAL) {   // no-op round"),
    "many-prepares-all-first": (None, LC, "if (rc) return rc;   // nothing launched yet for this learner"),
    "distance-before-the-average": (None, "dpwa_amd/csrc/measure.hpp", "if (int rc = ms[i].m->before(ms[i].p, ms[i].flat, ms[i].peer, fused, s)) return rc;"),
    "skip-is-the-no-op-round": (None, "dpwa_amd/csrc/kernels.hip", "if (vetoed && c.status == DPWA_STATUS_OK) {"),
    "skip-is-no-error": (None, "dpwa_amd/csrc/kernels.hip", "if (fa.status_mirror && c.status == DPWA_STATUS_ZERO_DIVISION) *fa.status_mirror = c.status;"),
    "many-checks-each-member": (None, LC, "if (int rc = finite_pass(checker[i], b.e[i].fa, b.e[i].peer, s)) return rc;"),
    "param-round-counted-at-launch": (None, MH, "if (param_) pd_.due = ++pd_.rounds % pd_.every == 0;"),
    "param-record-only-when-ok": (None, H, "the record is written only when"),
    "param-on-again-starts-anew": (None, MH, "pd_ = Param{count, workspace_off, record_off, every};"),
}
# (resident-not-in-next-slot cannot fire: a resident publish relocates first, which notes the written-through
# snapshot; it is what the mutant resident-publish-no-relocate runs into)
REFUSALS = tuple(k for k, v in RULES.items() if v[0] is not None and k != "resident-not-in-next-slot")

MUTANTS = (
    "factor-keeps-ahead-header",        # the code before this model's fix
    "lerp-keeps-written-through",
    "cancel-keeps-reader",
    "parity-from-next-version",
    "ahead-clock-one-place",
    "resident-publish-no-relocate",
    "second-fetch-resets-factor",
    "many-one-by-one",
    "write-clock-keeps-header",
    "distance-after-the-lerp",          # the record taken from the averaged parameters
    "distance-against-staging",         # an in-place fetch measured against what the last copy left in staging
    "skip-moves-clock",
    "skip-writes-whole-record",
    "skip-writes-param-record",
    "skip-leaves-snapshot-stale",       # a write-through or resident skipped round does not write the slot
    "stale-veto",                       # a veto outlives its round: once vetoed, every later checked round is
    "check-reads-own-params",
    "zero-division-loses-precedence",
    "skip-sets-sticky-status",
    "many-shares-one-veto",
    "many-checks-first-member-only",
    "param-every-off-by-one",
    "param-reset-keeps-counters",
    "param-record-after-the-lerp",
    "lerp-after-second-fetch-unchecked",   # the code before this model's fix
)
NEW_MUTANTS = MUTANTS[MUTANTS.index("skip-moves-clock"):]
# how a round that wrote the distance record averaged (Model.measured)
MEASURING = ("average", "average_through", "lerp", "resident", "many-batched", "many-unbatched", "unaligned")


class Spec:
    """What a group is made of: the dtype, n (elements; bytes for "mixed"), the interpolation, how far
    behind a 16-byte boundary the flat buffers begin (elements), which learners are resident."""

    def __init__(self, dtype, method, value=None, threshold=0.0, n=None, offset=0, resident=(), learners=3, seed=1,
                 finite=False, draws=()):
        self.dtype, self.method, self.value, self.threshold = dtype, method, value, threshold
        self.n = SIZES[dtype] if n is None else n
        self.offset, self.resident, self.learners, self.seed = offset, tuple(resident), learners, seed
        self.finite = finite          # operands without NaNs and infinities: the distance sums are finite
        # what a walk draws besides the calls it always drew: "check" (set_finite_check; on finite operands
        # poisoning and healing steps too), "param" (set_param_distance)
        self.draws = tuple(draws)
        assert dtype != "mixed" or (offset == 0 and self.n in (0, SIZES["mixed"]))

    @property
    def code(self):
        return MIXED_CODE if self.dtype == "mixed" else fref.CODE[self.dtype]

    @property
    def elem(self):
        return 1 if self.dtype == "mixed" else fref.SIZE[self.dtype]

    @property
    def numpy(self):
        return np.uint8 if self.dtype == "mixed" else fref.NUMPY[self.dtype]

    @property
    def nbytes(self):
        return self.n * self.elem

    @property
    def offset_bytes(self):
        return self.offset * self.elem

    def distance_n(self):
        """dpwa_distance.n: the elements summed over (a segmented payload: its element slots)."""
        if self.dtype != "mixed":
            return self.n
        return sum(length // mixed_ref.SIZE[d] for d, _, length, _ in mixed_ref.segments(MIXED_SPEC)[0])

    def terms(self):
        """The terms of each distance sum that can be non-zero: the elements (padding adds exact zeros)."""
        return sum(n for _, n in MIXED_SPEC) if self.dtype == "mixed" and self.n else self.n

    def _finite(self, i):
        """Normal deviates rounded to the dtype (dist_ref.to_bits), a subnormal and a signed zero among them."""
        rng = np.random.default_rng([self.seed + i, 77])

        def draw(d, n):
            bits = dist_ref.to_bits(d, rng.standard_normal(n))
            if n > 2:
                bits[1], bits[n - 2] = dist_ref.SUBNORMAL[d], dist_ref.NEG_ZERO[d]
            return bits
        if self.dtype != "mixed":
            return draw(self.dtype, self.n), draw(self.dtype, self.n)
        segs, total = mixed_ref.segments(MIXED_SPEC)
        out = []
        for _ in range(2):
            buf = np.zeros(total if self.n else 0, np.uint8)
            for d, off, _, n in segs if self.n else ():
                buf[off:off + n * mixed_ref.SIZE[d]] = draw(d, n).view(np.uint8)
            out.append(buf)
        return tuple(out)

    def operands(self, i):
        """The two flat buffers of learner i: the hard bit patterns of forms_ref.operands (mixed_ref.sample
        for a segmented payload), or finite values where the spec asks for them."""
        if self.finite:
            return self._finite(i)
        if self.dtype == "mixed":
            if self.n == 0:
                return np.zeros(0, np.uint8), np.zeros(0, np.uint8)
            p, q = mixed_ref.sample(MIXED_SPEC, self.seed + i)
            return p.copy(), q.copy()
        p, q = fref.operands(self.dtype, self.n, self.seed + i)
        return np.array(p), np.array(q)

    def lerp(self, p, q, f):
        if self.n == 0:
            return p.copy()
        if self.dtype == "mixed":
            return mixed_ref.lerp(MIXED_SPEC, p, q, f)
        return np.array(fref.lerp(self.dtype, p, q, f))

    def same(self, got, want):
        """NaN positions coincide, everything else bit for bit (the rule of forms_ref / mixed_ref)."""
        if self.n == 0:
            return len(got) == 0 and len(want) == 0
        if self.dtype == "mixed":
            return mixed_ref.same(MIXED_SPEC, np.asarray(got), np.asarray(want)) is None
        return fref.same(self.dtype, np.asarray(got), np.asarray(want))

    def nonfinite(self, payload):
        """Per element (per byte of a segmented payload): a NaN or an infinity, by finite_ref's rule."""
        if self.dtype != "mixed":
            return finite_ref.nonfinite(self.dtype, payload)
        out = np.zeros(len(payload), bool)
        for d, off, length, _ in mixed_ref.segments(MIXED_SPEC)[0] if self.n else ():
            bad = finite_ref.nonfinite(d, np.ascontiguousarray(payload[off:off + length]).view(finite_ref.NUMPY[d]))
            out[off:off + length] = np.repeat(bad, finite_ref.SIZE[d])
        return out

    def vetoes(self, payload):
        """finite_ref's answer for a peer payload (a segmented one: every byte of every segment)."""
        if self.n == 0:
            return False
        if self.dtype != "mixed":
            return finite_ref.vetoes(self.dtype, payload)
        return finite_ref.vetoes_mixed(mixed_ref.segments(MIXED_SPEC)[0], payload)

    def param_layout(self):
        """The parameter tensors as pdist_ref lays them out (PARAM_SIZES)."""
        assert self.n == SIZES[self.dtype]
        if self.dtype == "mixed":
            return pdist_ref.mixed("walk", {d: list(PARAM_SIZES[d]) for d, _ in MIXED_SPEC})
        return pdist_ref.ragged("walk", self.dtype, list(PARAM_SIZES[self.dtype]))

    def param_ranges(self):
        """[(byte offset, byte length, dtype code)] for dpwa_learner_set_param_distance."""
        return [(off, length, fref.CODE[d]) for _, d, off, length in self.param_layout().tensors]

    def param_distance(self, p, q):
        """((dist2, norm2), ...) per tensor: pdist_ref.reference."""
        as_bytes = lambda x: np.ascontiguousarray(x).view(np.uint8)                    # noqa: E731
        return tuple(pdist_ref.reference(self.param_layout(), as_bytes(p), as_bytes(q)))

    def distance(self, p, q):
        if self.dtype != "mixed":
            return dist_ref.reference(self.dtype, p, q)
        if self.n == 0:
            return 0.0, 0.0
        segs = mixed_ref.segments(MIXED_SPEC)[0]
        return dist_ref.reference_many([(s[0], mixed_ref.elements(p, s), mixed_ref.elements(q, s)) for s in segs])


ZERO_HEADER = (0.0, 0.0, 0, 0, 0)       # clock, loss, version, n, dtype: a slot as dpwa_learner_create leaves it
ZERO_COEF = (0.0, 0.0, 0.0, 0.0, 0)     # factor, new_clock, a, b, status


class Slot:
    def __init__(self):
        self.header = ZERO_HEADER
        self.payload = None          # unknown until written (hipMalloc does not clear it)
        self.published = False       # published[k].noted()


class Fetch:
    def __init__(self, owner, slot, kind, header, payload):
        self.owner, self.slot, self.kind = owner, slot, kind
        self.copied = kind != "zc"
        self.header, self.payload = header, payload       # of a copy: what landed in staging
        self.factored = False


class Learner:
    def __init__(self, flats):
        self.flats = [f.copy() for f in flats]
        self.slots = [Slot(), Slot()]
        self.version = 0
        self.clock = [0.0, 0.0, 0.0, 0.0]
        self.cur = 0
        self.coef = ZERO_COEF
        self.fetch = None
        self.reading = None          # (owner, slot) of the unfinished fetch: what Fetch::reads answers
        self.wt = None               # written_through noted: [flat key, with header]
        self.header_on_publish = False
        self.resident = False
        self.res_slot = 0
        self.dist_on = False
        self.dist = None             # the record (dist2, norm2, clock, n) once tracking was ever on
        self.staged = None           # what the last copying fetch left in staging (no caller reads it there)
        self.check = False           # dpwa_learner_set_finite_check
        self.skips = 0               # dpwa_learner_finite_skips
        self.sticky = 0              # the sticky status word (no walk polls it, so it is never cleared)
        self.vetoed_once = False     # (only the mutant stale-veto reads it)
        self.pd_on = False           # dpwa_learner_set_param_distance
        self.pd_every = 1
        self.pd = None               # the record (clock, count, pairs) once the option was ever on
        self.pd_rounds = (0, 0)      # dpwa_learner_param_distance_rounds: averaged, measured


class Model:
    def __init__(self, spec, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.spec, self.mutant = spec, mutant
        self.L = [Learner(spec.operands(i)) for i in range(spec.learners)]
        self.rule = None             # the refusal rule the last call fired
        self.out = None              # what the last copy_fetched / copy_factor / read_snapshot gave
        self.changed = False         # the last averaging call ended OK and changed the parameters
        self.measured = []           # (learner, MEASURING form) of the records the last call wrote
        self.skipped = []            # (learner, MEASURING form, poison_tags of the snapshot) of the rounds it skipped
        self.checked = 0             # checked rounds of the last call that averaged

    def copy(self):
        return copy.deepcopy(self)

    # ------------------------------------------------------------------ helpers
    def _refuse(self, rule):
        self.rule = rule
        return RULES[rule][0]

    def _next_slot(self, l):
        return (l.version + (1 if self.mutant == "parity-from-next-version" else 0)) % 2

    def _still_read(self, i, k):
        """wait_slot_readers: a peer holds an unconsumed fetch of learner i's slot k."""
        return any(r.reading == (i, k) for r in self.L)

    def params_key(self, i, flat):
        """What `flat` names: a buffer of the learner's (0, 1) or the resident pointer ("res")."""
        l = self.L[i]
        return ("slot", l.res_slot) if flat == "res" else ("flat", flat)

    def params(self, i, key):
        l = self.L[i]
        return l.slots[key[1]].payload if key[0] == "slot" else l.flats[key[1]]

    def source(self, i):
        """(header, payload) the fetch in flight reads: the staged copy, or the peer's slot as it is."""
        f = self.L[i].fetch
        if f.copied:
            return f.header, f.payload
        s = self.L[f.owner].slots[f.slot]
        return s.header, s.payload

    def _coef(self, l, header, loss):
        """factor_math and factor_commit's clock: factor_ref.evaluate of the case."""
        sp = self.spec
        case = (sp.method, sp.value, sp.threshold, l.clock[l.cur], header[0], loss, header[1])
        want = factor_ref.evaluate(case)
        if want == factor_ref.ZD:
            return (0.0, l.clock[l.cur], 0.0, 1.0, 1)
        f, new_clock, a, b = want
        return (f, new_clock, float(a), float(b), 0)

    def _vetoes(self, l, p, q):
        """Does the pass of a round of learner l veto it?  q: the snapshot read, p: its own parameters."""
        if not l.check:
            return False
        bad = self.spec.vetoes(q)
        if self.mutant == "check-reads-own-params":
            bad = bad or self.spec.vetoes(p)
        if self.mutant == "stale-veto":
            bad = bad or l.vetoed_once
        l.vetoed_once = l.vetoed_once or bad
        return bad

    def _round_coef(self, l, header, loss, vetoed):
        """fused_factor: the coefficients of a round whose pass said `vetoed`; counts a skip, sets the sticky word."""
        c = self._coef(l, header, loss)
        if c[4] == STATUS_ZD:
            if vetoed and self.mutant == "zero-division-loses-precedence":
                c = c[:4] + (STATUS_SKIPPED,)
                l.skips += 1
            else:
                l.sticky = STATUS_ZD
        elif vetoed:
            c = (0.0, c[1] if self.mutant == "skip-moves-clock" else l.clock[l.cur], 0.0, 1.0, STATUS_SKIPPED)
            l.skips += 1
            if self.mutant == "skip-sets-sticky-status":
                l.sticky = STATUS_SKIPPED
        return c

    def _finish(self, l):
        l.fetch = None
        l.reading = None

    def _record(self, l, p, q, form, after=None):
        """The record of a round that averaged: p and q as they were before it (measure.hpp: the pass runs
        before the average, the tracked kernel sums the operands it loaded)."""
        i, status = self.L.index(l), l.coef[4]
        forms = (form,) + (("unaligned",) if self.spec.offset and not l.resident else ())
        if status == STATUS_SKIPPED:
            self.skipped += [(i, f, poison_tags(self.spec, q)) for f in forms]
        elif status == 0 and l.check:
            self.checked += 1
        if l.pd_on:     # Measure::before counts the round that launches, whatever it turns out to be
            rounds = l.pd_rounds[0] + 1
            due = (rounds + (1 if self.mutant == "param-every-off-by-one" else 0)) % l.pd_every == 0
            l.pd_rounds = (rounds, l.pd_rounds[1] + int(due))
            if due and (status == 0 or (status == STATUS_SKIPPED and self.mutant == "skip-writes-param-record")):
                pp = after if self.mutant == "param-record-after-the-lerp" and after is not None else p
                pairs = self.spec.param_distance(pp, q)
                l.pd = (l.coef[1], len(pairs), pairs)
        if l.dist_on and (status == 0 or (status == STATUS_SKIPPED and self.mutant == "skip-writes-whole-record")):
            if self.mutant == "distance-after-the-lerp" and after is not None:
                p = after
            if self.mutant == "distance-against-staging" and not l.fetch.copied and l.staged is not None:
                q = l.staged
            d2, n2 = self.spec.distance(p, q)
            l.dist = (d2, n2, l.coef[1], self.spec.distance_n())
            self.measured += [(i, f) for f in forms]

    # ------------------------------------------------------------------ the calls
    def apply(self, op):
        self.rule, self.out, self.changed, self.measured, self.skipped, self.checked = None, None, False, [], [], 0
        return getattr(self, "_" + op[0])(*op[1:])

    def _step(self, i, flat, bits):
        """The caller's own write of its parameters (the training step): not a library call."""
        key = self.params_key(i, flat)
        if key[0] == "slot":
            self.L[i].slots[key[1]].payload = np.array(bits, dtype=self.spec.numpy)
        else:
            self.L[i].flats[key[1]] = np.array(bits, dtype=self.spec.numpy)
        return OK

    def _set_resident(self, i, flat=0):
        l = self.L[i]
        if l.resident:
            return self._refuse("set-resident-twice")
        if l.version != 0 or l.fetch is not None:
            return self._refuse("set-resident-late")
        l.slots[0].payload = l.flats[flat].copy()
        l.resident, l.res_slot = True, 0
        l.wt = [("slot", 0), False]
        return OK

    def _relocate_impl(self, i):
        l = self.L[i]
        k = self._next_slot(l)
        if not l.resident or l.res_slot == k:
            return OK
        if self._still_read(i, k):
            return self._refuse("slot-still-read")
        l.slots[k].payload = l.slots[l.res_slot].payload.copy()
        l.res_slot = k
        l.wt = [("slot", k), False]
        return OK

    def _relocate(self, i):
        if self.L[i].fetch is not None:
            return self._refuse("relocate-with-fetch")
        return self._relocate_impl(i)

    def _publish(self, i, flat, loss, reuse=False):
        l, sp = self.L[i], self.spec
        k = self._next_slot(l)
        if l.resident:
            if flat != "res":
                return self._refuse("resident-publish-pointer")
            if self.mutant != "resident-publish-no-relocate":
                rc = self._relocate_impl(i)
                if rc:
                    return rc
            reuse = True
        key = self.params_key(i, flat)
        header_only = reuse and l.wt is not None and l.wt[0] == key
        if header_only:
            if l.wt[1]:
                l.cur = (l.cur + 1) & 3          # header and clock were written ahead: nothing moves
            else:
                l.clock[l.cur] += 1.0
                l.slots[k].header = (l.clock[l.cur], float(loss), l.version + 1, sp.n, sp.code)
        else:
            if l.resident:
                return self._refuse("resident-not-in-next-slot")
            if self._still_read(i, k):
                return self._refuse("slot-still-read")
            l.slots[k].payload = self.params(i, key).copy()
            l.clock[l.cur] += 1.0
            l.slots[k].header = (l.clock[l.cur], float(loss), l.version + 1, sp.n, sp.code)
        l.wt = None
        l.slots[k].published = True
        l.version += 1
        return OK

    def _publish_reuse(self, i, flat, loss):
        return self._publish(i, flat, loss, True)

    def _fetch(self, i, j, version, kind):
        l, peer = self.L[i], self.L[j]
        assert i != j and kind in FETCH_KINDS
        if version == 0:
            return self._refuse("fetch-version-0")
        if l.check and l.fetch is not None and l.fetch.factored and self.mutant != "lerp-after-second-fetch-unchecked":
            return self._refuse("fetch-over-checked-factor")
        k = (version - 1) % 2
        if not peer.slots[k].published:
            return self._refuse("fetch-slot-never-published")
        s = peer.slots[k]
        f = Fetch(j, k, kind, s.header, None if kind == "zc" else s.payload.copy())
        if l.fetch is not None and self.mutant != "second-fetch-resets-factor":
            f.factored = l.fetch.factored       # "as it always has" (fetch.hpp)
        l.fetch = f
        l.reading = (j, k)
        if f.copied:
            l.staged = f.payload
        return OK

    def _factor(self, i, loss):
        l = self.L[i]
        if l.fetch is None:
            return self._refuse("factor-without-fetch")
        if l.fetch.factored:
            return self._refuse("factor-twice")
        header, q = self.source(i)
        # (whatever flat the lerp will name: the mutant that reads the learner's own parameters reads flat 0)
        l.coef = self._round_coef(l, header, loss, self._vetoes(l, self.params(i, self.params_key(i, "res" if l.resident else 0)), q))
        l.clock[(l.cur + 1) & 3] = l.coef[1]
        l.cur = (l.cur + 1) & 3
        l.fetch.factored = True
        if l.wt is not None and self.mutant != "factor-keeps-ahead-header":
            l.wt[1] = False
        return OK

    def _lerp(self, i, flat):
        l = self.L[i]
        if l.fetch is None or not l.fetch.factored:
            return self._refuse("lerp-without-factor")
        if l.resident:
            return self._refuse("lerp-resident")
        assert flat != "res"
        if l.pd_on and self.spec.offset:
            return self._refuse("param-unaligned")
        _, q = self.source(i)
        p = l.flats[flat]
        r = self.spec.lerp(p, q, l.coef[0]) if l.coef[4] == 0 else p
        self._record(l, p, q, "lerp", r)
        if l.coef[4] == 0:
            self.changed = r.tobytes() != p.tobytes()
            l.flats[flat] = r
        if self.mutant != "lerp-keeps-written-through":
            l.wt = None
        self._finish(l)
        return OK

    def _average_check(self, i, flat, through):
        """average_prepare's refusals, against the state as it is."""
        l = self.L[i]
        if l.fetch is None:
            return self._refuse("average-without-fetch")
        if l.fetch.factored:
            return self._refuse("average-after-factor")
        if l.pd_on and flat != "res" and self.spec.offset:
            return self._refuse("param-unaligned")
        if l.resident:
            if flat != "res":
                return self._refuse("resident-average-pointer")
            through = True
        else:
            assert flat != "res"
        if through and self._still_read(i, self._next_slot(l)):
            return self._refuse("slot-still-read")
        return OK

    def _average_commit(self, i, flat, loss, through, form=None, vetoed=None):
        l, sp = self.L[i], self.spec
        oop = l.resident
        through = through or oop
        key = self.params_key(i, flat)
        header, q = self.source(i)
        p = self.params(i, key)
        l.coef = self._round_coef(l, header, loss, self._vetoes(l, p, q) if vetoed is None else vetoed)
        r = sp.lerp(p, q, l.coef[0]) if l.coef[4] == 0 else p.copy()
        self._record(l, p, q, form or ("resident" if oop else "average_through" if through else "average"), r)
        self.changed = self.changed or (l.coef[4] == 0 and r.tobytes() != p.tobytes())
        l.clock[(l.cur + 1) & 3] = l.coef[1]
        ahead = False
        if through:
            k = self._next_slot(l)
            ahead = sp.method != "loss" and not l.header_on_publish
            if ahead:
                place = 1 if self.mutant == "ahead-clock-one-place" else 2
                l.clock[(l.cur + place) & 3] = l.coef[1] + 1.0
                l.slots[k].header = (l.coef[1] + 1.0, math.nan, l.version + 1, sp.n, sp.code)
            stale = self.mutant == "skip-leaves-snapshot-stale" and l.coef[4] == STATUS_SKIPPED
            if not (stale and l.slots[k].payload is not None):
                l.slots[k].payload = r.copy()
            if oop:
                l.res_slot = k
        if not oop:
            l.flats[key[1]] = r
        l.cur = (l.cur + 1) & 3
        l.wt = [("slot", l.res_slot) if oop else key, ahead] if through else None
        self._finish(l)

    def _average(self, i, flat, loss, through=False):
        rc = self._average_check(i, flat, through)
        if rc:
            return rc
        self._average_commit(i, flat, loss, through)
        return OK

    def _average_through(self, i, flat, loss):
        return self._average(i, flat, loss, True)

    def _average_many(self, entries):
        """entries: ((learner, flat, loss, write_through), ...), each learner once."""
        assert len({e[0] for e in entries}) == len(entries)
        if self.mutant == "many-one-by-one":
            trial = self.copy()
            trial.mutant = None
            for i, flat, loss, through in entries:
                rc = trial._average(i, flat, loss, bool(through))
                if rc:
                    self.rule = trial.rule
                    return rc
        else:
            for i, flat, loss, through in entries:
                rc = self._average_check(i, flat, bool(through))
                if rc:
                    return rc
        # launch_plans: 16-byte aligned plans of one element type share a dispatch with those of the same
        # (write-through, resident) form; every other plan is launched on its own
        def form_of(e):
            return (bool(e[3]) or self.L[e[0]].resident, self.L[e[0]].resident)
        batchable = [e for e in entries if self.spec.dtype != "mixed" and (self.L[e[0]].resident or not self.spec.offset)]
        # each checking member's pass reads that member's own snapshot, before anything of the dispatch
        vetoed = {}
        for i, flat, _, _ in entries:
            vetoed[i] = self._vetoes(self.L[i], self.params(i, self.params_key(i, flat)), self.source(i)[1])
        checking = [e[0] for e in entries if self.L[e[0]].check]
        if self.mutant == "many-shares-one-veto" and any(vetoed[i] for i in checking):
            vetoed.update({i: True for i in checking})
        if self.mutant == "many-checks-first-member-only":
            vetoed.update({i: False for i in checking[1:]})
        for e in entries:
            i, flat, loss, through = e
            shared = sum(1 for o in batchable if form_of(o) == form_of(e))
            form = "many-unbatched" if e not in batchable else "many-batched" if shared > 1 else "many-alone"
            self._average_commit(i, flat, loss, bool(through), form, vetoed[i])
        return OK

    def _cancel(self, i):
        l = self.L[i]
        l.fetch = None
        if self.mutant != "cancel-keeps-reader":
            l.reading = None
        return OK

    def _write_clock(self, i, clock):
        l = self.L[i]
        l.clock[l.cur] = float(clock)
        if l.wt is not None and self.mutant != "write-clock-keeps-header":
            l.wt[1] = False
        return OK

    def _copy_fetched(self, i):
        if self.L[i].fetch is None:
            return self._refuse("copy-fetched-without-fetch")
        self.out = self.source(i)[1].copy()
        return OK

    def _copy_factor(self, i):
        self.out = self.L[i].coef[0]
        return OK

    def _read_snapshot(self, i):
        l = self.L[i]
        if l.version == 0:
            self.out = (0, None, None)
        else:
            s = l.slots[(l.version - 1) % 2]
            self.out = (l.version, s.header, s.payload.copy())
        return OK

    def _set_distance(self, i, on):
        l = self.L[i]
        l.dist_on = bool(on)
        if on and l.dist is None:
            l.dist = (0.0, 0.0, 0.0, 0)
        return OK

    def _set_finite_check(self, i, on):
        l = self.L[i]
        if on and l.fetch is not None and l.fetch.factored and self.mutant != "lerp-after-second-fetch-unchecked":
            return self._refuse("set-check-over-factor")
        l.check = bool(on)
        return OK

    def _set_param_distance(self, i, every):
        """every == 0: count = 0, which switches the option off and leaves the record and the counters."""
        l = self.L[i]
        if every == 0:
            l.pd_on = False
            return OK
        count = len(self.spec.param_ranges())
        l.pd_on, l.pd_every = True, every
        l.pd = (0.0, 0, ((0.0, 0.0),) * count)
        if self.mutant != "param-reset-keeps-counters":
            l.pd_rounds = (0, 0)
        return OK

    def _set_header_publish(self, i, always):
        self.L[i].header_on_publish = bool(always)
        return OK

    # ------------------------------------------------------------------ what a caller can observe
    def observe(self):
        """Everything the ABI shows, as plain comparable values (arrays as bytes, doubles as bits)."""
        out = []
        for l in self.L:
            slots = tuple((header_key(s.header), None if s.payload is None else s.payload.tobytes(), s.published)
                          for s in l.slots)
            out.append((tuple(f.tobytes() for f in l.flats), slots, l.version, bits(l.clock[l.cur]),
                        tuple(bits(x) for x in l.coef[:4]) + (l.coef[4],),
                        l.res_slot if l.resident else -1,
                        None if l.dist is None else tuple(bits(x) for x in l.dist[:3]) + (l.dist[3],),
                        l.check, l.skips, l.sticky, l.pd_rounds,
                        None if l.pd is None else (bits(l.pd[0]), l.pd[1], tuple((bits(a), bits(b)) for a, b in l.pd[2]))))
        o = self.out
        if isinstance(o, np.ndarray):
            o = o.tobytes()
        elif isinstance(o, float):
            o = bits(o)
        elif isinstance(o, tuple):
            o = (o[0], None if o[1] is None else header_key(o[1]), None if o[2] is None else o[2].tobytes())
        return tuple(out), o


def bits(x):
    return "nan" if x != x else factor_ref.bits64(float(x))


def header_key(h):
    return (bits(h[0]), bits(h[1]), h[2], h[3], h[4])


def header_same(got, want):
    """Header fields as moves_ref / relay_ref compare them: clock and loss as doubles (a NaN loss is
    "a NaN"), version, n and dtype as integers."""
    return header_key(got) == header_key(want)


# ---------------------------------------------------------------------- poisoning a learner's parameters
def _element(spec, where):
    """(dtype, byte offset, numpy type) of the element POISON_AT names."""
    seg, index = POISON_AT[spec.dtype][where]
    if seg is None:
        return spec.dtype, index * spec.elem, spec.numpy
    off = next(off for d, off, _, _ in mixed_ref.segments(MIXED_SPEC)[0] if d == seg)
    return seg, off + index * finite_ref.SIZE[seg], finite_ref.NUMPY[seg]


def poisoned(m, i, flat, where, kind):
    """Learner i's current parameter bits (of `flat`, or "res") with the element POISON_AT[dtype][where]
    replaced by finite_ref.BAD's `kind`: what a ("step", i, flat, bits) writes to poison it."""
    spec = m.spec
    d, byte, np_t = _element(spec, where)
    out = m.params(i, m.params_key(i, flat)).copy()
    raw = out.view(np.uint8)
    raw[byte:byte + finite_ref.SIZE[d]] = np.array([finite_ref.BAD[d][kind]], dtype=np_t).view(np.uint8)
    return out


def healed(m, i, flat):
    """The same bits with every NaN and infinity replaced by what the learner began with there."""
    cur = m.params(i, m.params_key(i, flat))
    return np.where(m.spec.nonfinite(cur), m.spec.operands(i)[0], cur).astype(m.spec.numpy)


def poison_tags(spec, q):
    """((position, kind), ...): the named elements of payload q that hold one of finite_ref.BAD's patterns."""
    if spec.n != SIZES[spec.dtype]:
        return ()
    out, raw = [], np.ascontiguousarray(q).view(np.uint8)
    for where in POISON_AT[spec.dtype]:
        d, byte, np_t = _element(spec, where)
        got = int(raw[byte:byte + finite_ref.SIZE[d]].view(np_t)[0])
        out += [(where, kind) for kind, pattern in finite_ref.BAD[d].items() if got == pattern]
    return tuple(out)


# ---------------------------------------------------------------------- running a list of calls
def run(spec, ops, mutant=None):
    """[(rc, rule, observation)] of the model over `ops`."""
    m = Model(spec, mutant)
    out = []
    for op in ops:
        rc = m.apply(op)
        out.append((rc, m.rule, m.observe()))
    return out


def first_difference(spec, ops, mutant):
    """The index of the first call after which `mutant` differs from the model in the return code or
    an observable value; None when it never does."""
    a, b = Model(spec), Model(spec, mutant)
    for t, op in enumerate(ops):
        if a.apply(op) != b.apply(op) or a.observe() != b.observe():
            return t
    return None


# ---------------------------------------------------------------------- walks
PROFILES = ("plain", "through", "resident", "mix")
PROFILE_METHOD = {"plain": ("constant", 0.3), "through": ("clock", None), "resident": ("loss", None), "mix": ("clock", None)}
LOSSES = (0.0, 0.25, 0.5, 0.75, 1.0, 2.0)
CLOCKS = (0.0, 1.0, 3.5, -1.0, 7.0)
WALK_LENGTH = 150
REFUSAL_SHARE = 0.35       # how often a draw the model refuses is kept (the walks stay well under a quarter)


def profile_spec(dtype, profile, offset=0, n=None, seed=1, finite=False, draws=()):
    method, value = PROFILE_METHOD[profile]
    resident = {"resident": (0, 1, 2), "mix": (1,)}.get(profile, ())
    return Spec(dtype, method, value, 0.0, n=n, offset=offset, resident=resident, seed=seed, finite=finite, draws=draws)


def setup_ops(spec):
    """What a walk begins with: the resident learners made so; on finite operands every learner tracks the
    distance from the start (the walk still switches it off and on)."""
    return [("set_resident", i) for i in spec.resident] + \
           [("set_distance", i, 1) for i in range(spec.learners) if spec.finite] + \
           [("set_finite_check", i, 1) for i in range(spec.learners) if "check" in spec.draws] + \
           [("set_param_distance", i, 2) for i in range(spec.learners) if "param" in spec.draws]


NEW_SHARE = 0.22           # of the draws of a walk whose spec asks for the newer calls (Spec.draws)
EVERY = (0, 1, 2, 3)
POISON_WEIGHT, HEAL_WEIGHT = 3.0, 5.0
CHECK_WALK_LENGTH = 165


def _draw_new(rng, m):
    """One of the calls Spec.draws asks for.  Most of the time every learner checks; a learner's parameters
    are poisoned now and then (one element of POISON_AT, one of POISON_KINDS) and healed soon after, so that
    most rounds still average.  A resident learner's parameters are stepped only while they lie in the slot of
    its next publish, which no peer reads."""
    sp = m.spec
    i = rng.randrange(sp.learners)
    l = m.L[i]
    flat = "res" if l.resident else 0
    w = {}
    if "check" in sp.draws:
        w["set_finite_check"] = 0.3 if l.check else 4.0
        if sp.finite and (not l.resident or (l.res_slot == m._next_slot(l) and not m._still_read(i, l.res_slot))):
            dirty = sp.vetoes(m.params(i, m.params_key(i, flat)))
            # (a resident learner is seldom where it may be stepped: it is poisoned more readily there)
            w["heal" if dirty else "poison"] = HEAL_WEIGHT if dirty else POISON_WEIGHT * (6 if l.resident else 1)
    if "param" in sp.draws:
        w["set_param_distance"] = 0.8
    names = sorted(w)
    name = rng.choices(names, [w[k] for k in names])[0]
    if name == "set_finite_check":
        return ("set_finite_check", i, int(not l.check))
    if name == "set_param_distance":
        return ("set_param_distance", i, rng.choice(EVERY))
    if name == "heal":
        return ("step", i, flat, healed(m, i, flat))
    return ("step", i, flat, poisoned(m, i, flat, rng.choice(sorted(POISON_AT[sp.dtype])), rng.choice(POISON_KINDS)))


def _draw(rng, m, profile):
    """One candidate call, drawn from the state: mostly what the loop would do next, sometimes not.  (A spec
    that asks for none of the newer calls draws exactly what it always drew.)"""
    sp = m.spec
    if sp.draws and rng.random() < NEW_SHARE:
        return _draw_new(rng, m)
    i = rng.randrange(sp.learners)
    l = m.L[i]
    peers = [j for j in range(sp.learners) if j != i]
    loss = rng.choice(LOSSES)
    res = l.resident
    flat = ("res" if rng.random() < 0.93 else 0) if res else (0 if rng.random() < 0.85 else 1)
    form = {"plain": "plain", "through": "through", "resident": "through"}.get(profile) or rng.choice(("plain", "through"))
    through = form == "through" and rng.random() < 0.85 or form == "plain" and rng.random() < 0.05

    def publish():
        reuse = form == "through" and rng.random() < 0.8 or rng.random() < 0.1
        return ("publish_reuse" if reuse else "publish", i, flat, loss)

    def fetch():
        j = rng.choice(peers)
        v = m.L[j].version
        if v < 2 and rng.random() < 0.15:
            v += 1                                   # a slot never published
        return ("fetch", i, j, v, rng.choice(FETCH_KINDS))

    def many():
        ready = [k for k in range(sp.learners) if m.L[k].fetch is not None and not m.L[k].fetch.factored]
        if i not in ready:
            ready.append(i)
        if len(ready) < 2:
            ready.append(rng.choice([k for k in range(sp.learners) if k not in ready]))
        rng.shuffle(ready)
        return ("average_many", tuple((k, "res" if m.L[k].resident else 0, rng.choice(LOSSES),
                                       int(form == "through" and rng.random() < 0.6)) for k in ready))

    table = {
        "publish": publish, "fetch": fetch, "many": many,
        "factor": lambda: ("factor", i, loss),
        "lerp": lambda: ("lerp", i, 0 if res else flat),
        "average": lambda: ("average_through" if through else "average", i, flat, loss),
        "cancel": lambda: ("cancel", i),
        "relocate": lambda: ("relocate", i),
        "write_clock": lambda: ("write_clock", i, rng.choice(CLOCKS)),
        "copy_fetched": lambda: ("copy_fetched", i),
        "copy_factor": lambda: ("copy_factor", i),
        "read_snapshot": lambda: ("read_snapshot", i),
        "set_distance": lambda: ("set_distance", i, int(not l.dist_on)),
        "set_header_publish": lambda: ("set_header_publish", i, int(not l.header_on_publish)),
        "set_resident": lambda: ("set_resident", i),
    }
    common = {"write_clock": 0.5, "copy_factor": 0.3, "read_snapshot": 0.5, "set_distance": 0.4,
              "set_header_publish": 0.3 if profile in ("through", "mix") else 0.05,
              "set_resident": 0.15 if (l.resident or l.version) else 0.0}
    if l.fetch is None:
        w = {"fetch": 6, "publish": 3.5, "relocate": 1.0 if res else 0.2, "cancel": 0.3, "factor": 0.3, "average": 0.3,
             "lerp": 0.2, "copy_fetched": 0.2}
    elif not l.fetch.factored:
        w = {"average": 4, "factor": 1.5 if res else 3, "many": 1.5, "cancel": 0.6, "fetch": 0.7, "copy_fetched": 0.8,
             "publish": 1.0, "relocate": 0.2, "lerp": 0.2}
    else:
        w = {"lerp": 4, "cancel": 2.0 if res else 0.8, "fetch": 1.0, "publish": 1.0, "factor": 0.3, "average": 0.3,
             "copy_fetched": 0.5, "relocate": 0.2}
    w.update(common)
    names = sorted(w)
    return table[rng.choices(names, [w[k] for k in names])[0]]()


def walk(seed, dtype, profile, length=WALK_LENGTH, offset=0, finite=False, draws=()):
    """(spec, ops): `length` calls drawn with random.Random from the model's current state.  The model
    is asked beforehand whether a drawn call is legal; a refused one is kept REFUSAL_SHARE of the time."""
    spec = profile_spec(dtype, profile, offset, finite=finite, draws=draws)
    rng = random.Random("%s/%s/%d/%d" % (profile, dtype, offset, seed))
    m = Model(spec)
    ops = setup_ops(spec)
    for op in ops:
        assert m.apply(op) == OK
    while len(ops) < length:
        op = _draw(rng, m, profile)
        trial = m.copy()
        if trial.apply(op) != OK and rng.random() >= REFUSAL_SHARE:
            continue
        m = trial
        ops.append(op)
    return spec, ops


# (profile, dtype, offset in elements, seed, finite operands): the committed walks.  Every dtype meets every
# profile on the hard bit patterns, the element types once 16-byte aligned and once one element past (a
# segmented payload is aligned).  On those operands every distance sum is NaN or infinite, so each profile
# is also walked on finite operands with the distance tracked, where the sums are held to dist_ref.bound.
WALKS = tuple((p, d, o, 1, False) for p in PROFILES for d in DTYPES for o in ((0,) if d == "mixed" else (0, 1))
              if o == 0 or (p, d) in (("plain", "f32"), ("through", "bf16"), ("through", "f32"), ("mix", "f16"))) + (
    ("plain", "bf16", 1, 2, True), ("through", "f32", 0, 2, True), ("resident", "f16", 0, 2, True),
    ("mix", "mixed", 0, 2, True), ("mix", "f32", 1, 2, True))


# (..., what the walk draws besides): the walks with the non-finite check on.  Finite operands, poisoned and
# healed as the walk goes, one walk per profile and one unaligned (where the per-parameter option, which
# refuses unaligned parameters, stays off); one walk draws both options and set_distance together.  (The seeds
# are the first with which the model meets tests/test_walk_host.py's conditions with some room.)  The last
# one runs on the hard bit patterns, where nearly every snapshot holds a NaN or an infinity and nearly every
# checked round is skipped: the long run of consecutive vetoes that a veto outliving its round would hide in.
CHECK_WALKS = (
    ("plain", "f32", 0, 4, True, ("check",)), ("through", "bf16", 0, 9, True, ("check",)),
    ("resident", "f16", 0, 11, True, ("check",)), ("mix", "mixed", 0, 32, True, ("check",)),
    ("mix", "f32", 1, 3, True, ("check",)), ("through", "f32", 0, 9, True, ("check", "param")),
    ("mix", "bf16", 0, 3, False, ("check",)))
ALL_HARD = CHECK_WALKS[-1]


def walk_id(w):
    return "%s-%s-%s-seed%d%s%s" % (w[0], w[1], "aligned" if w[2] == 0 else "off%d" % w[2], w[3], "-finite" if w[4] else "",
                                    "".join("-" + d for d in w[5]) if len(w) > 5 else "")


def walk_of(w):
    """(spec, ops) of an entry of WALKS or CHECK_WALKS."""
    if len(w) == 5:
        return walk(w[3], w[1], w[0], offset=w[2], finite=w[4])
    return walk(w[3], w[1], w[0], length=CHECK_WALK_LENGTH, offset=w[2], finite=w[4], draws=w[5])


# ---------------------------------------------------------------------- directed sequences
def _every_pair():
    """The ten main calls in an order in which every ordered pair of them (a call after itself
    included) occurs: an Euler circuit of the complete digraph with loops (101 calls)."""
    n = len(MAIN)
    nxt = [0] * n
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            circuit.append(stack.pop())
    return [MAIN[v] for v in reversed(circuit)]


def _pair_ops():
    """Learner 0 issues _every_pair() with fixed arguments, legal or not as the state has it; learner 1
    publishes first and again now and then, when it may, so that there is something new to fetch."""
    spec = profile_spec("f32", "through")
    m = Model(spec)
    ops = [("publish", 1, 0, 0.5), ("publish", 0, 0, 1.0)]
    for op in ops:
        assert m.apply(op) == OK
    args = {"publish": (0, 0, 1.0), "publish_reuse": (0, 0, 0.75), "factor": (0, 0.5), "lerp": (0, 0),
            "average": (0, 0, 0.5), "average_through": (0, 0, 2.0), "cancel": (0,), "relocate": (0,),
            "write_clock": (0, 3.5)}
    fetches = 0
    for name in _every_pair():
        if name == "fetch":
            again = ("publish", 1, 0, 0.25)
            if fetches % 3 == 2 and m.copy().apply(again) == OK:
                m.apply(again)
                ops.append(again)
            op = ("fetch", 0, 1, m.L[1].version, FETCH_KINDS[fetches % 4])
            fetches += 1
        else:
            op = (name,) + args[name]
        m.apply(op)
        ops.append(op)
    return spec, ops


def directed():
    """name -> (spec, ops): one sequence per state variable a learner carries between calls."""
    T, P, R = profile_spec, "publish", "publish_reuse"
    seqs = {}
    # wt_header: a factor (then cancelled) between a write-through average and its reusing publish -- the
    # served header must carry the factor's clock, not the average's (the Python layer never issues this
    # order: every fetch there follows a publish)
    seqs["factor-after-ahead-header"] = (T("f32", "through"), [
        (P, 1, 0, 0.5), (P, 1, 0, 0.5), (P, 0, 0, 1.0), ("fetch", 0, 1, 2, "ce"), ("average_through", 0, 0, 0.5),
        ("fetch", 0, 1, 2, "ce"), ("factor", 0, 0.5), ("cancel", 0), (R, 0, 0, 0.75), ("read_snapshot", 0),
        ("fetch", 2, 0, 2, "zc"), ("average", 2, 0, 1.0), (P, 0, 0, 1.0), (P, 0, 0, 1.0), ("read_snapshot", 0)])
    # the same on a resident learner (the factor is allowed there, the lerp is not)
    seqs["factor-after-ahead-header-resident"] = (T("bf16", "mix"), [
        ("set_resident", 1), (P, 0, 0, 0.5), (P, 0, 1, 0.5), (P, 1, "res", 1.0), ("fetch", 1, 0, 2, "zc"),
        ("average", 1, "res", 0.5), ("fetch", 1, 0, 2, "k1"), ("factor", 1, 0.25), ("lerp", 1, 0), ("cancel", 1), (P, 1, "res", 0.75),
        ("read_snapshot", 1)])
    # the clock ring: four places, the ahead clock two places on, write_clock in between
    seqs["clock-ring"] = (T("f16", "through"), [
        (P, 1, 0, 0.5), (P, 0, 0, 1.0), ("fetch", 0, 1, 1, "k512"), ("average_through", 0, 0, 0.5), (R, 0, 0, 0.5),
        ("fetch", 0, 1, 1, "zc"), ("average_through", 0, 0, 0.5), ("write_clock", 0, 3.5), (R, 0, 0, 0.5),
        ("fetch", 0, 1, 1, "ce"), ("factor", 0, 1.0), ("lerp", 0, 0), (R, 0, 0, 0.5), ("fetch", 0, 1, 1, "ce"),
        ("average_through", 0, 0, 0.5), ("fetch", 0, 1, 1, "ce"), ("average_through", 0, 0, 0.5), (R, 0, 0, 0.5),
        ("read_snapshot", 0)])
    # slot parity: three publishes, a reader of each slot
    seqs["slot-parity"] = (T("f32", "plain", offset=1), [
        (P, 0, 0, 1.0), ("fetch", 1, 0, 1, "ce"), (P, 0, 1, 1.0), ("fetch", 2, 0, 2, "zc"), (P, 0, 0, 1.0),
        ("cancel", 1), (P, 0, 0, 1.0), (P, 0, 1, 1.0), ("average", 2, 0, 1.0), (P, 0, 1, 1.0), ("read_snapshot", 0)])
    # written_through / wt_flat: dropped by a lerp, by a plain average, by another flat
    seqs["written-through"] = (T("bf16", "through", offset=1), [
        (P, 1, 0, 0.5), (P, 0, 0, 1.0), ("fetch", 0, 1, 1, "ce"), ("average_through", 0, 0, 0.5),
        ("fetch", 0, 1, 1, "ce"), ("factor", 0, 0.5), ("lerp", 0, 0), (R, 0, 0, 0.75), ("read_snapshot", 0),
        ("fetch", 0, 1, 1, "zc"), ("average_through", 0, 0, 0.5), (R, 0, 1, 0.75), ("read_snapshot", 0),
        ("fetch", 0, 1, 1, "zc"), ("average_through", 0, 1, 0.5), ("fetch", 0, 1, 1, "zc"), ("average", 0, 1, 0.5),
        (R, 0, 1, 0.75), ("read_snapshot", 0), ("set_header_publish", 0, 1), ("fetch", 0, 1, 1, "k1"),
        ("average_through", 0, 0, 0.5), (R, 0, 0, 0.25), ("read_snapshot", 0)])
    # res_slot: relocation by publish and by relocate, the wrong pointer, set_resident refused
    seqs["res-slot"] = (T("f16", "resident"), [
        ("set_resident", 0), ("set_resident", 1), ("set_resident", 2), ("set_resident", 0), (P, 0, "res", 1.0),
        (P, 0, "res", 1.0), ("relocate", 0), ("relocate", 0), (P, 1, "res", 0.5), ("set_resident", 1),
        ("fetch", 0, 1, 1, "zc"), ("relocate", 0), ("average", 0, 0, 0.5), ("average", 0, "res", 0.5), (P, 0, 0, 1.0),
        (P, 0, "res", 1.0), ("fetch", 0, 1, 1, "ce"), ("factor", 0, 0.5), ("lerp", 0, 0), ("cancel", 0),
        ("read_snapshot", 0), ("fetch", 2, 0, 3, "zc"), (P, 0, "res", 1.0), (P, 0, "res", 1.0), ("relocate", 0),
        ("cancel", 2), ("relocate", 0), (P, 0, "res", 1.0)])
    # the reader list: a publish and a write-through average refused while a peer reads the slot
    seqs["slot-readers"] = (T("f32", "through"), [
        (P, 0, 0, 1.0), (P, 1, 0, 0.5), ("fetch", 1, 0, 1, "ce"), (P, 0, 0, 1.0), (P, 0, 0, 1.0),
        ("fetch", 0, 1, 1, "zc"), ("average_through", 0, 0, 0.5), ("average", 0, 0, 0.5), ("cancel", 1),
        ("fetch", 0, 1, 1, "zc"), ("average_through", 0, 0, 0.5), ("fetch", 2, 0, 2, "zc"), ("fetch", 2, 1, 1, "k1"),
        (R, 0, 0, 1.0), (P, 0, 0, 1.0), ("fetch", 1, 0, 4, "zc"), ("fetch", 0, 1, 1, "ce"),
        ("average_many", ((1, 0, 0.5, 0), (0, 0, 0.5, 1))), ("average_many", ((0, 0, 0.5, 0), (1, 0, 0.5, 1), (2, 0, 0.25, 1))),
        ("fetch", 1, 0, 0, "ce"), ("fetch", 1, 2, 1, "ce")])
    # staging: a copy keeps what it pulled while the peer publishes on; a second fetch replaces it
    seqs["staging"] = (T("bf16", "plain"), [
        (P, 1, 0, 0.5), ("fetch", 0, 1, 1, "k1"), ("copy_fetched", 0), ("cancel", 0), (P, 1, 1, 0.25), (P, 1, 0, 0.25),
        ("copy_fetched", 0), ("fetch", 0, 1, 3, "ce"), ("fetch", 0, 1, 3, "k512"), ("copy_fetched", 0),
        ("average", 0, 0, 1.0), ("copy_factor", 0), ("copy_fetched", 0)])
    # the phase: a second fetch before the lerp keeps the factor; factor twice; average after factor
    seqs["fetch-phase"] = (T("f16", "plain", offset=1), [
        (P, 1, 0, 0.5), (P, 2, 1, 0.25), ("lerp", 0, 0), ("fetch", 0, 1, 1, "ce"), ("lerp", 0, 0), ("factor", 0, 1.0),
        ("factor", 0, 1.0), ("average", 0, 0, 1.0), ("fetch", 0, 2, 1, "zc"), ("copy_factor", 0), ("lerp", 0, 0),
        ("lerp", 0, 0), ("fetch", 0, 1, 1, "k512"), ("cancel", 0), ("factor", 0, 1.0), ("average", 0, 0, 1.0)])
    # the distance record: on, off and on again; every form that measures; a no-op round leaves it
    seqs["distance"] = (T("f32", "resident", offset=1, finite=True), [
        ("set_distance", 0, 1), ("set_distance", 2, 1), (P, 1, 0, 0.5), (P, 2, 1, 0.0), (P, 0, 0, 1.0), ("fetch", 0, 1, 1, "ce"),
        ("average", 0, 0, 0.5), ("set_distance", 0, 0), ("fetch", 0, 1, 1, "zc"), ("average_through", 0, 0, 0.5),
        ("set_distance", 0, 1), ("fetch", 0, 1, 1, "zc"), ("factor", 0, 0.25), ("lerp", 0, 0), ("fetch", 0, 2, 1, "zc"),
        ("average", 0, 1, 0.0), ("fetch", 0, 1, 1, "k1"), ("fetch", 2, 1, 1, "zc"),
        ("average_many", ((0, 0, 0.5, 1), (2, 0, 0.75, 0))), (R, 0, 0, 0.5), ("read_snapshot", 0)])
    seqs["distance-mixed"] = (T("mixed", "mix", finite=True), [
        ("set_resident", 1), ("set_distance", 0, 1), ("set_distance", 1, 1), (P, 2, 0, 0.5), (P, 1, "res", 0.5),
        ("fetch", 0, 2, 1, "ce"), ("average_through", 0, 0, 0.5), ("fetch", 1, 2, 1, "zc"), ("average", 1, "res", 0.5),
        ("fetch", 0, 1, 1, "zc"), ("factor", 0, 0.5), ("lerp", 0, 0), (R, 0, 0, 1.0), (P, 1, "res", 1.0),
        ("fetch", 0, 2, 1, "zc"), ("fetch", 1, 2, 1, "ce"), ("average_many", ((0, 0, 0.5, 0), (1, "res", 0.5, 0)))])
    # which operands the record is taken from, 16-byte aligned (the tracked kernel; a shared dispatch): a copy
    # of version 1 stays in staging while version 2 is read in place
    seqs["distance-forms"] = (T("bf16", "through", finite=True), [
        ("set_distance", 0, 1), ("set_distance", 1, 1), ("set_distance", 2, 1), (P, 1, 0, 0.5), (P, 2, 0, 0.25),
        (P, 0, 0, 1.0), ("fetch", 0, 1, 1, "ce"), ("average", 0, 0, 0.5), (P, 1, 1, 0.5), ("fetch", 0, 1, 2, "zc"),
        ("average_through", 0, 0, 0.5), ("fetch", 0, 2, 1, "zc"), ("factor", 0, 0.75), ("lerp", 0, 0),
        ("fetch", 0, 1, 2, "zc"), ("fetch", 2, 1, 2, "k512"), ("average_many", ((0, 0, 0.5, 1), (2, 0, 0.5, 1))),
        (R, 0, 0, 0.5), (R, 2, 0, 0.5), ("read_snapshot", 0)])
    # a fetch of the version before the current one, with no write-through pending on its owner: the reader
    # holds the very slot the owner's next publish, write-through average or relocation rewrites
    seqs["previous-version"] = (T("f32", "mix"), [
        ("set_resident", 1), (P, 0, 0, 1.0), (P, 0, 1, 0.5), (P, 1, "res", 0.5), (P, 1, "res", 0.5),
        ("fetch", 2, 0, 1, "zc"), (P, 0, 0, 1.0), ("fetch", 0, 1, 2, "ce"), ("average_through", 0, 0, 0.5),
        ("copy_fetched", 2), ("cancel", 2), ("average_through", 0, 0, 0.5), (R, 0, 0, 1.0),
        ("fetch", 2, 1, 1, "k1"), ("relocate", 1), (P, 1, "res", 1.0), ("average", 2, 0, 0.5), ("relocate", 1),
        (P, 1, "res", 1.0), ("read_snapshot", 1)])
    # n = 0, which dpwa_learner_create accepts: headers and clocks move, no byte does
    seqs["no-elements"] = (T("f32", "through", n=0), [
        ("set_distance", 0, 1), (P, 1, 0, 0.5), (P, 0, 0, 1.0), ("fetch", 0, 1, 1, "ce"), ("average_through", 0, 0, 0.5),
        (R, 0, 0, 1.0), ("fetch", 0, 1, 1, "zc"), ("factor", 0, 0.5), ("lerp", 0, 0), ("fetch", 2, 0, 2, "k1"),
        ("copy_fetched", 2), ("average", 2, 0, 0.25), ("read_snapshot", 0), ("read_snapshot", 2)])
    # dpwa_learner_average_many prepares every learner before it commits any: learner 1's write-through
    # slot is still read by learner 0, whose average in the same call has not finished its fetch yet
    seqs["many-order"] = (T("f16", "through"), [
        (P, 0, 0, 1.0), (P, 1, 0, 0.5), ("fetch", 0, 1, 1, "zc"), (P, 1, 0, 0.5), ("fetch", 1, 0, 1, "ce"),
        ("average_many", ((0, 0, 0.5, 0), (1, 0, 0.5, 1))), ("average_many", ((1, 0, 0.5, 0), (0, 0, 0.5, 1))),
        ("fetch", 1, 0, 1, "zc"), ("average_through", 1, 0, 0.5), (R, 1, 0, 0.5), (R, 0, 0, 0.5)])
    seqs["every-pair"] = _pair_ops()
    seqs.update(_checked_sequences())
    return seqs


class _Script:
    """A sequence written against the model's state, for the steps that poison or heal what a learner holds."""

    def __init__(self, spec):
        self.spec, self.m, self.ops = spec, Model(spec), []

    def do(self, *ops):
        for op in ops:
            self.m.apply(op)
            self.ops.append(op)

    def poison(self, i, flat, where, kind):
        self.do(("step", i, flat, poisoned(self.m, i, flat, where, kind)))

    def heal(self, i, flat):
        self.do(("step", i, flat, healed(self.m, i, flat)))

    def serve(self, j, where, kind):
        """Learner j publishes what it holds (version 1, finite), then the same with one element poisoned
        (version 2): both stay fetchable while it publishes nothing more."""
        self.do(("publish", j, 0, 0.5))
        self.poison(j, 0, where, kind)
        self.do(("publish", j, 0, 0.5))

    def done(self):
        return self.spec, self.ops


def _skip_every_form(dtype, where, kind):
    """A skipped round and then a finite one in every averaging form, both distance records on: learner 2
    serves (version 1 finite, version 2 poisoned), learner 0 averages from its flat buffer, learner 1 is
    resident.  The dispatch of two is batched for one element type and two launches for a segmented payload."""
    s = _Script(profile_spec(dtype, "mix", finite=True))
    s.do(("set_resident", 1))
    for i in (0, 1):
        s.do(("set_finite_check", i, 1), ("set_distance", i, 1), ("set_param_distance", i, 1))
    s.serve(2, where, kind)
    s.do(("publish", 0, 0, 1.0), ("publish", 1, "res", 1.0))
    for v, kind_ in ((2, "ce"), (1, "ce")):
        s.do(("fetch", 0, 2, v, kind_), ("average", 0, 0, 0.5))
    for v in (2, 1):
        s.do(("fetch", 0, 2, v, "zc"), ("average_through", 0, 0, 0.5), ("publish_reuse", 0, 0, 0.75))
    for v, kind_ in ((2, "zc"), (1, "k1")):
        s.do(("fetch", 1, 2, v, kind_), ("average", 1, "res", 0.5), ("publish", 1, "res", 0.75))
    for v, kind_ in ((2, "k512"), (1, "zc")):
        s.do(("fetch", 0, 2, v, kind_), ("factor", 0, 0.5), ("lerp", 0, 0))
    for v in (2, 1):     # learner 2 does not check; its own parameters are the poisoned ones and stay so
        s.do(("fetch", 0, 2, v, "zc"), ("fetch", 2, 0, s.m.L[0].version, "ce"),
             ("average_many", ((2, 0, 0.5, 0), (0, 0, 0.5, 0))))
    s.do(("read_snapshot", 0), ("read_snapshot", 1))
    return s.done()


_CHECKED = []


def _checked_sequences():
    """The sequences for the non-finite check and the per-parameter distance (built once: they poison what
    the model holds at that point)."""
    if _CHECKED:
        return _CHECKED[0]
    T, P, R = profile_spec, "publish", "publish_reuse"
    seqs = {}
    # the veto's stamp: skipped, finite, skipped, finite in a row on learner 0, the check switched off and on
    # in between; then an average that is prepared (its stamp taken) and refused for a reader of its slot,
    # between two checked rounds
    s = _Script(T("f32", "through", finite=True))
    s.do(("set_finite_check", 0, 1), ("set_distance", 0, 1), (P, 0, 0, 1.0))
    s.serve(1, "first", "snan")
    s.do(("fetch", 0, 1, 2, "ce"), ("average", 0, 0, 0.5), ("fetch", 0, 1, 1, "zc"), ("average", 0, 0, 0.5),
         ("fetch", 0, 1, 2, "zc"), ("average_through", 0, 0, 0.5), ("set_finite_check", 0, 0), ("set_finite_check", 0, 1),
         ("fetch", 0, 1, 1, "ce"), ("average_through", 0, 0, 0.5), (R, 0, 0, 0.75),
         ("fetch", 2, 0, 1, "zc"), ("fetch", 0, 1, 2, "zc"), ("average_through", 0, 0, 0.5), ("cancel", 2),
         ("average_through", 0, 0, 0.5), ("fetch", 0, 1, 1, "k1"), ("average_through", 0, 0, 0.5), (R, 0, 0, 0.5),
         ("read_snapshot", 0))
    seqs["veto-stamp"] = s.done()
    # a second fetch over a checked factor, copied and in place, and switching the check on over an unchecked
    # one: both refused; with the check off the second fetch keeps the factor as it always has
    s = _Script(T("bf16", "plain", finite=True))
    s.do(("set_finite_check", 0, 1), (P, 0, 0, 1.0))
    s.serve(1, "tail-last", "+inf")
    s.do(("fetch", 0, 1, 1, "ce"), ("factor", 0, 0.5), ("fetch", 0, 1, 2, "ce"), ("lerp", 0, 0),
         ("fetch", 0, 1, 1, "zc"), ("factor", 0, 0.5), ("fetch", 0, 1, 2, "zc"), ("lerp", 0, 0),
         ("set_finite_check", 0, 0), ("fetch", 0, 1, 1, "k1"), ("factor", 0, 0.5), ("set_finite_check", 0, 1),
         ("fetch", 0, 1, 2, "zc"), ("lerp", 0, 0))
    s.heal(0, 0)
    s.do(("set_finite_check", 0, 1), ("fetch", 0, 1, 2, "zc"), ("factor", 0, 0.5), ("set_finite_check", 0, 1),
         ("lerp", 0, 0), ("fetch", 0, 1, 1, "zc"), ("factor", 0, 0.5), ("lerp", 0, 0))
    s.poison(1, 0, "gap", "snan")     # (a second poison, in no parameter tensor: the next version is skipped as well)
    s.do((P, 1, 0, 0.5), ("fetch", 0, 1, 3, "ce"), ("average", 0, 0, 0.5))
    seqs["second-fetch-checked"] = s.done()
    seqs["skip-every-form"] = _skip_every_form("f16", "span-last", "qnan")
    seqs["skip-every-form-segmented"] = _skip_every_form("mixed", "bf16-last", "-inf")
    # one dispatch of four: learners 0, 1, 2 check and learner 1's snapshot is poisoned; learner 3 does not
    # check, its snapshot is poisoned too, and it goes non-finite (the documented behaviour)
    s = _Script(Spec("f16", "constant", 0.3, learners=5, finite=True))
    for i in (0, 1, 2):
        s.do(("set_finite_check", i, 1))
    for i in (0, 1, 2, 3):
        s.do((P, i, 0, 1.0))
    s.do(("set_distance", 3, 1), ("set_param_distance", 3, 1))    # the poison lies in no tensor: only the whole-model sums show it
    s.poison(4, 0, "gap", "-inf")
    s.do((P, 4, 0, 0.5), ("fetch", 0, 3, 1, "zc"), ("fetch", 1, 4, 1, "ce"), ("fetch", 2, 0, 1, "ce"), ("fetch", 3, 4, 1, "zc"),
         ("average_many", ((0, 0, 0.5, 0), (1, 0, 0.5, 0), (2, 0, 0.5, 0), (3, 0, 0.5, 0))),
         ("fetch", 1, 2, 1, "zc"), ("fetch", 2, 4, 1, "zc"), ("average_many", ((2, 0, 0.5, 1), (1, 0, 0.5, 1))))
    seqs["many-one-poisoned"] = s.done()
    # a round that is both a ZeroDivision (both clocks 0) and poisoned stays a ZeroDivision and is not counted
    s = _Script(Spec("f32", "clock", finite=True))
    s.do(("set_finite_check", 0, 1), ("write_clock", 1, -1.0))
    s.poison(1, 0, "span-last", "qnan")
    s.do((P, 1, 0, 0.5), ("fetch", 0, 1, 1, "zc"), ("average", 0, 0, 0.5), ("fetch", 0, 1, 1, "ce"), ("factor", 0, 0.5),
         ("lerp", 0, 0), ("write_clock", 0, 3.5), ("fetch", 0, 1, 1, "zc"), ("average_through", 0, 0, 0.5))
    seqs["zero-division-and-poison"] = s.done()
    # every = 3 over ten rounds, the sixth a skipped one; off, a round, on again (the record and the counters
    # start anew), off
    s = _Script(T("f32", "through", finite=True))
    s.do(("set_finite_check", 0, 1), (P, 0, 0, 1.0))
    s.serve(1, "tail-last", "snan")
    s.do(("set_param_distance", 0, 3))
    for r in range(1, 11):
        s.do(("fetch", 0, 1, 2 if r == 6 else 1, FETCH_KINDS[r % 4]))
        s.do(*((("factor", 0, 0.5), ("lerp", 0, 0)) if r % 4 == 1 else (("average_through" if r % 2 else "average", 0, 0, 0.5),)))
    s.do(("set_param_distance", 0, 0), ("fetch", 0, 1, 1, "zc"), ("average", 0, 0, 0.5), ("set_param_distance", 0, 2),
         ("fetch", 0, 1, 1, "zc"), ("average", 0, 0, 0.5), ("fetch", 0, 1, 1, "ce"), ("average", 0, 0, 0.5),
         ("set_param_distance", 0, 0), ("fetch", 0, 1, 1, "ce"), ("average", 0, 0, 0.5))
    seqs["param-every"] = s.done()
    # unaligned parameters while the per-parameter option is on: every averaging call refused, nothing counted;
    # the resident learner's slot is aligned
    seqs["param-unaligned-refused"] = (T("f32", "mix", offset=1, finite=True), [
        ("set_resident", 1), ("set_param_distance", 0, 1), ("set_param_distance", 1, 1), (P, 2, 0, 0.5), (P, 1, "res", 1.0),
        ("fetch", 0, 2, 1, "ce"), ("average", 0, 0, 0.5), ("average_through", 0, 1, 0.5), ("factor", 0, 0.5), ("lerp", 0, 0),
        ("cancel", 0), ("fetch", 0, 2, 1, "zc"), ("fetch", 1, 2, 1, "zc"), ("average_many", ((1, "res", 0.5, 0), (0, 0, 0.5, 0))),
        ("average", 1, 0, 0.5), ("average", 1, "res", 0.5), ("set_param_distance", 0, 0), ("average", 0, 0, 0.5),
        ("fetch", 0, 2, 1, "zc"), ("factor", 0, 0.5), ("lerp", 0, 0)])
    # a learner whose own parameters are poisoned is not skipped; the peer that fetches it is
    s = _Script(T("f16", "plain", finite=True))
    s.do(("set_finite_check", 0, 1), ("set_finite_check", 2, 1), (P, 1, 0, 0.5))
    s.poison(0, 0, "tail-last", "+inf")
    s.do(("fetch", 0, 1, 1, "ce"), ("average", 0, 0, 0.5), (P, 0, 0, 1.0), ("fetch", 2, 0, 1, "zc"), ("average", 2, 0, 0.5),
         ("fetch", 2, 1, 1, "zc"), ("average", 2, 0, 0.5))
    seqs["own-params-poisoned"] = s.done()
    _CHECKED.append(seqs)
    return seqs


def replay_text(spec, ops):
    """An expression that replays the calls against the model on the host (with tests.walk_ref imported)."""
    plain = [op[:3] + (np.asarray(op[3]).tolist(),) if op[0] == "step" else op for op in ops]     # a step's bits as a list
    return ("walk_ref.run(walk_ref.Spec(%r, %r, %r, %r, n=%d, offset=%d, resident=%r, seed=%d, finite=%r, learners=%d, "
            "draws=%r), %r)" % (spec.dtype, spec.method, spec.value, spec.threshold, spec.n, spec.offset, spec.resident,
                                spec.seed, spec.finite, spec.learners, spec.draws, plain))
