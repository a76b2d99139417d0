"""The per-parameter distance to the peer on the GPU (include/dpwa_hip.h ``dpwa_param_range``): the
stand-alone pass and its finishing step through the stateless entries, then through a learner in
every averaging form and through the adapter, against tests/pdist_ref.py (each tensor's float64 terms
summed exactly on the host) within ``dist_ref.bound(n_t)``.

Shapes are the smallest at which it can go wrong (tests/pdist_ref.py): layout A puts three tensors
into the quarters of one 1-KiB span, ends tensors mid-item, on a quarter, one past it and across a
span boundary, and has an empty tensor; A16 is the same for the 16-bit types; M is a segmented
payload; B, the only large one, has three times as many spans in one tensor as a tensor has rows
(the count is read from the sizes entry)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from dpwa_amd import DpwaConnection, DpwaPyTorchAdapter, _lib
from dpwa_amd.devview import device_tensor
from dpwa_amd.flat import c_layout
from dpwa_amd.group import LocalGroup
from dpwa_amd.learner import Learner
from tests import dist_ref, mixed_ref
from tests import pdist_ref as ref
from tests.test_gpu_kernels import ptr, stream
from tests.test_gpu_self_peer import write_self_cfg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "mixed": torch.uint8}
LAYOUTS = {lay.name: lay for lay in ref.small_layouts()}


def c_ranges(lay):
    arr = (_lib.ParamRange * len(lay.tensors))()
    for i, (_, d, off, length) in enumerate(lay.tensors):
        arr[i] = _lib.ParamRange(off, length, dist_ref.CODE[d], 0)
    return arr


def py_ranges(lay):
    return [(name, TORCH[d], off, length) for name, d, off, length in lay.tensors]


def py_layout(lay):
    return tuple((TORCH[d], off, length) for d, off, length in lay.segments) if lay.segments else None


@functools.lru_cache(maxsize=None)
def max_rows():
    z = _lib.ParamSizes()
    _lib.call("dpwa_param_distance_sizes", None, 0, ctypes.byref(z))
    return z.max_rows          # 1024 as built


class Stateless:
    """Table, workspace and record of one layout for the stateless entries; the workspace is zeroed
    once, here: every call must leave it zero."""

    def __init__(self, lay):
        self.lay, self.count = lay, len(lay.tensors)
        z = _lib.ParamSizes()
        arr = c_ranges(lay)
        _lib.call("dpwa_param_distance_sizes", arr, self.count, ctypes.byref(z))
        self.table = torch.zeros(z.table_bytes, dtype=torch.uint8, device=DEV)
        self.workspace = torch.zeros(z.workspace_bytes, dtype=torch.uint8, device=DEV)
        self.record_bytes = z.record_bytes
        _lib.call("dpwa_param_distance_table", arr, self.count, ptr(self.table))

    def measure(self, p, q):
        """[(dist2, norm2)] of the payload bytes p, q (numpy uint8); checks what else the call wrote."""
        dp, dq = torch.from_numpy(p.copy()).to(DEV), torch.from_numpy(q.copy()).to(DEV)
        rec = torch.full((self.record_bytes,), 0xa5, dtype=torch.uint8, device=DEV)   # poisoned: it must be written
        _lib.call("dpwa_measure_param_distance", ptr(self.table), self.count, ptr(dp), ptr(dq), len(p),
                  ptr(self.workspace), ptr(rec), stream(), None, None)
        torch.cuda.synchronize()
        assert np.array_equal(dp.cpu().numpy(), p) and np.array_equal(dq.cpu().numpy(), q)   # it stores to neither
        assert not bool(self.workspace.any()), "the call leaves the accumulators zero"
        return read_record(rec, self.count, clock=0.0)


def read_record(rec, count, clock):
    host = rec.cpu().numpy().tobytes()
    head = np.frombuffer(host[:16], dtype=np.float64)[0], np.frombuffer(host[8:16], dtype=np.int64)[0]
    assert head == (clock, count), head
    return [tuple(row) for row in np.frombuffer(host[16:], dtype=np.float64).reshape(-1, 2).tolist()]


def check(lay, got, want, what):
    for t, (g, w) in enumerate(zip(got, want)):
        print("%s %s tensor %d n=%d: got %r ref %r bound %.3g" % (lay.name, what, t, lay.elements(t), g, w,
                                                                 dist_ref.bound(max(lay.elements(t), 1))))
    bad = ref.problems(lay, got, want)
    assert not bad, (what, bad)


# ---------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_every_input_set_in_every_tensor(name):
    """Every input set of tests/dist_ref.py in every tensor at once (each tensor its own draw), one
    workspace for all of them: a call is not polluted by the one before."""
    lay = LAYOUTS[name]
    dev = Stateless(lay)
    for case in ref.CASE_NAMES:
        p, q = ref.inputs(lay, case)
        check(lay, dev.measure(p, q), ref.reference(lay, p, q), case)
    p, q = ref.inputs(lay, "normal")
    check(lay, dev.measure(q, p), ref.reference(lay, q, p), "the operands swapped, after a NaN and an inf call")


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_one_tensor_differs_and_its_neighbours_do_not_notice(name):
    """A difference in a tensor's last element among equal tensors: every other record is exactly 0.
    A NaN or an inf in one tensor among normal ones: every other record is finite and in bound."""
    lay = LAYOUTS[name]
    dev = Stateless(lay)
    for t in range(len(lay.tensors)):
        if not lay.elements(t):
            continue
        for case, base in (("last-element", "equal"), ("one-nan", "normal"), ("one-inf", "normal")):
            p, q = ref.inputs(lay, case, victim=t, base=base)
            got, want = dev.measure(p, q), ref.reference(lay, p, q)
            check(lay, got, want, "%s in tensor %d" % (case, t))
            for u in range(len(lay.tensors)):
                if u == t:
                    continue
                if base == "equal":
                    assert got[u][0] == 0.0, (case, t, u)
                else:
                    assert math.isfinite(got[u][0]) and math.isfinite(got[u][1]), (case, t, u)
            if case == "last-element":
                assert got[t][0] > 0.0
            if case == "one-nan":
                assert math.isnan(got[t][0]) and math.isnan(got[t][1])
            if case == "one-inf":
                assert got[t][0] == math.inf and math.isfinite(got[t][1])


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_gap_and_padding_bytes_enter_no_sum(name):
    """Every byte of no tensor filled with a NaN pattern on both operands changes no record, and the
    sum of the records over zero-gapped buffers is the whole-model pass's within the two bounds."""
    lay = LAYOUTS[name]
    dev = Stateless(lay)
    p, q = ref.inputs(lay, "normal")
    clean = dev.measure(p, q)
    want = ref.reference(lay, p, q)
    for fill in (0xff, 0x7f):
        pn, qn = ref.inputs(lay, "normal", fill=fill)
        assert ref.gap_mask(lay).any() and (pn[ref.gap_mask(lay)] == fill).all()
        got = dev.measure(pn, qn)
        check(lay, got, want, "gaps filled with %#x" % fill)
        assert all(math.isfinite(x) for pair in got for x in pair)
    # against dpwa_measure_distance(_mixed), which counts the (zero) gaps
    dp, dq = torch.from_numpy(p.copy()).to(DEV), torch.from_numpy(q.copy()).to(DEV)
    ws = ctypes.c_int64()
    _lib.call("dpwa_distance_workspace", ctypes.byref(ws))
    workspace = torch.zeros(ws.value, dtype=torch.uint8, device=DEV)
    rec = torch.zeros(32, dtype=torch.uint8, device=DEV)
    if lay.payload == "mixed":
        _lib.call("dpwa_measure_distance_mixed", ctypes.byref(c_layout(py_layout(lay))), ptr(dp), ptr(dq), ptr(workspace),
                  ptr(rec), stream())
    else:
        _lib.call("dpwa_measure_distance", dist_ref.CODE[lay.payload], ptr(dp), ptr(dq),
                  lay.total_bytes // dist_ref.SIZE[lay.payload], ptr(workspace), ptr(rec), stream())
    torch.cuda.synchronize()
    whole = _lib.Distance.from_buffer_copy(rec.cpu().numpy().tobytes())
    for k, w in enumerate((whole.dist2, whole.norm2)):
        total = math.fsum(pair[k] for pair in clean)
        slack = sum(dist_ref.bound(max(lay.elements(t), 1)) * clean[t][k] for t in range(len(clean)))
        slack += dist_ref.bound(whole.n) * w
        print("%s sum of records %r whole %r slack %.3g" % (lay.name, total, w, slack))
        assert abs(total - w) <= slack, (k, total, w, slack)


def test_more_spans_than_rows():
    """Layout B: one tensor of (3 R + 2) spans plus an item and one element -- R = 1024 rows as built, so
    3075 spans, every row added into three times or more -- and a one-element neighbour behind it, which
    ends the payload inside a 16-byte item.  The neighbour stays exact whatever the large tensor holds."""
    lay = ref.layout_b(max_rows())
    assert lay.elements(0) // dist_ref.SPAN["f32"] >= 3 * max_rows() and lay.total_bytes % 16 == 4
    dev = Stateless(lay)
    assert dev.workspace.numel() == (max_rows() + 1) * _lib.DISTANCE_ACC_STRIDE
    for case in ("normal", "equal", "last-element"):
        p, q = ref.inputs(lay, case)
        check(lay, dev.measure(p, q), ref.reference(lay, p, q), case)
    p, q = ref.inputs(lay, "one-nan", victim=0, base="normal")
    got, want = dev.measure(p, q), ref.reference(lay, p, q)
    check(lay, got, want, "a NaN in the large tensor")
    assert math.isnan(got[0][0]) and math.isfinite(got[1][0]) and got[1][1] == want[1][1]   # one term: exact
    p, q = ref.inputs(lay, "last-element", victim=1, base="equal")
    got = dev.measure(p, q)
    assert got[0][0] == 0.0 and got[1][0] > 0.0


def test_the_finishing_step_alone():
    """dpwa_param_distance_finish with a coef: a status that is not OK leaves the record's bytes and
    still zeroes the rows; OK writes the record with the coef's clock."""
    lay = LAYOUTS["A"]
    dev = Stateless(lay)
    rec = torch.full((dev.record_bytes,), 0xa5, dtype=torch.uint8, device=DEV)
    for status, clock in ((_lib.STATUS_ZERO_DIVISION, 5.5), (_lib.STATUS_OK, 6.5)):
        dev.workspace.view(torch.float64).view(-1, _lib.DISTANCE_ACC_STRIDE // 8)[:, :2] = 1.0   # each row's pair
        coef = _lib.Coef(0.5, clock, 0.5, 0.5, status, 0)
        coef_dev = torch.frombuffer(bytearray(bytes(coef)), dtype=torch.uint8).to(DEV)
        _lib.call("dpwa_param_distance_finish", ptr(dev.table), dev.count, ptr(dev.workspace), ptr(rec), ptr(coef_dev),
                  stream(), None, None)
        torch.cuda.synchronize()
        assert not bool(dev.workspace.any())
        if status != _lib.STATUS_OK:
            assert bool((rec == 0xa5).all())
            continue
        rows = [r for _, r in ref.rows_of(lay, max_rows())[0]]
        assert read_record(rec, dev.count, clock) == [(float(r), float(r)) for r in rows]   # the rows held 1.0 each


# ---------------------------------------------------------------- 2. a learner, every averaging form
def self_cfg(tmp_path, interp="clock"):
    cfg = tmp_path / ("self_%s.yaml" % interp)
    write_self_cfg(cfg, 1.0, interp, 0.0, None)
    return str(cfg)


def to_dev(lay, data):
    t = torch.from_numpy(data.copy()).to(DEV)
    return t if lay.payload == "mixed" else t.view(TORCH[lay.payload])


def raw_record(conn):
    """The learner's per-parameter record as bytes (synchronises)."""
    p, count = ctypes.c_void_p(), ctypes.c_int64()
    _lib.call("dpwa_learner_param_distance", conn._learner.handle, ctypes.byref(p), ctypes.byref(count))
    torch.cuda.synchronize()
    return device_tensor(p.value, 16 + 16 * count.value, torch.uint8, DEV).clone(), count.value


def snapshot_after(conn, params, lay, wrote_through, resident=False):
    """The learner's snapshot after its last average, from the host.  An average that wrote through (or
    a resident one) left the averaged parameters in the slot of the next publish: a header-only publish
    (the reuse guard is off: it moves no payload byte) makes that slot the one dpwa_learner_read_snapshot
    reads.  Otherwise the average wrote no snapshot and this is the one published before it."""
    h = conn._learner.handle
    if wrote_through:
        _lib.call("dpwa_learner_publish" if resident else "dpwa_learner_publish_reuse", h, ptr(params), 9.0, None,
                  stream())                                      # (a resident publish moves no byte either)
    torch.cuda.synchronize()
    out = np.full(lay.total_bytes, 0xEE, dtype=np.uint8)
    hdr, v = ctypes.create_string_buffer(256), ctypes.c_uint64()
    _lib.call("dpwa_learner_read_snapshot", h, hdr, ctypes.c_void_p(out.ctypes.data), out.nbytes, ctypes.byref(v))
    return out


def run_form(cfg, lay, form, track, rounds=2, every=1):
    """`rounds` rounds of one learner whose peer is its own snapshot: the snapshot holds the round's q,
    the parameters its p.  Returns what the rounds left, and per round what the records said."""
    kw = dict(track_distance="per_parameter", parameter_ranges=py_ranges(lay), distance_every=every) if track else {}
    conn = DpwaConnection("w1", cfg, seed=3, group=LocalGroup(), layout=py_layout(lay), **kw)
    sets = [ref.inputs(lay, "normal" if r % 2 == 0 else "subnormal-differences") for r in range(rounds)]
    sets = [(p, q) if r % 2 == 0 else (q, p) for r, (p, q) in enumerate(sets)]
    flat = to_dev(lay, sets[0][1])
    if form == "resident":
        flat = conn.make_resident(flat)
    seen = []
    for r, (p, q) in enumerate(sets):
        if form == "resident":            # the step follows the average: p == q, the slot just published
            conn.parameters.copy_(to_dev(lay, q))
            conn.update_send(conn.parameters, 1.0 + r)
            conn.update_wait_average(conn.parameters, 0.5 + r)
            p = q
        else:
            flat.copy_(to_dev(lay, q))
            conn.update_send(flat, 1.0 + r)
            flat.copy_(to_dev(lay, p))
            if form == "split":
                payload, _ = conn.update_wait(0.5 + r)
                assert payload is not None
                if track and r == 0:
                    assert conn.last_distance is None         # update_wait alone measures nothing
                conn.average(flat)
            else:
                conn.update_wait_average(flat, 0.5 + r, write_through=form == "write-through")
        if track:
            d = conn.last_distance
            whole = d.read()
            parts = [(dt, ref.tensor_bits(lay, t, p), ref.tensor_bits(lay, t, q))
                     for t, (_, dt, _, _) in enumerate(lay.tensors)]
            want = dist_ref.reference_many(parts)
            real = sum(lay.elements(t) for t in range(len(lay.tensors)))
            for got, w in ((whole.dist2, want[0]), (whole.norm2, want[1])):     # the whole-model record, as before
                assert dist_ref.problem(got, w, real) is None, (form, r, dist_ref.problem(got, w, real))
            assert whole.clock == conn.clock
            seen.append((d.parameters, d.parameters.read() if d.parameters is not None else None,
                         d.parameters.clock if d.parameters is not None else None, conn.clock, p, q))
    torch.cuda.synchronize()
    params = conn.parameters if form == "resident" else flat
    out = {"params": params.cpu().view(torch.uint8).numpy().copy(), "clock": conn.clock,
           "coef": bytes(conn._learner.read_coef()), "seen": seen}
    out["snapshot"] = snapshot_after(conn, params, lay, form in ("write-through", "resident"), form == "resident")
    if form in ("write-through", "resident"):
        assert np.array_equal(out["snapshot"], out["params"]), (form, "the snapshot written through is the parameters")
    else:
        assert np.array_equal(out["snapshot"], sets[-1][1]), (form, "the published snapshot is untouched")
    conn.close()
    return out


@pytest.mark.parametrize("form,name", [("plain", "A"), ("write-through", "A"), ("resident", "A"), ("split", "A"),
                                       ("plain", "A16-bf16"), ("write-through", "M"), ("plain", "M"), ("split", "M")])
def test_learner_forms(tmp_path, form, name):
    """Two rounds in one averaging form with the per-parameter distance on and off: parameters, snapshot
    (the slot the last average wrote through, read back after a header-only publish; for the forms that
    write none, the published one), clock and dpwa_coef are bit-equal, the whole-model record is within
    its own bound, and every tensor's record is the reference of that round's operands with the clock
    the round committed."""
    lay = LAYOUTS[name]
    cfg = self_cfg(tmp_path)
    off, on = run_form(cfg, lay, form, False), run_form(cfg, lay, form, True)
    assert np.array_equal(off["params"], on["params"]) and off["clock"] == on["clock"] and off["coef"] == on["coef"]
    assert np.array_equal(off["snapshot"], on["snapshot"]) and not (on["snapshot"] == 0xEE).all()
    assert len(on["seen"]) == 2
    for r, (pd, got, clock, conn_clock, p, q) in enumerate(on["seen"]):
        assert pd is not None and clock == conn_clock
        want = ref.reference(lay, p, q)
        check(lay, [got[n] for n, _, _, _ in lay.tensors], want, "%s round %d" % (form, r))
        if form == "resident":
            assert all(pair[0] == 0.0 for pair in got.values())
    names = [n for n, _, _, _ in lay.tensors]
    assert list(on["seen"][0][1]) == names


def test_two_learners_through_update_wait_average_many(tmp_path):
    """Two learners that average with each other in one batched dispatch, which stays as it is."""
    lay = LAYOUTS["A"]
    cfg = tmp_path / "many.yaml"
    cfg.write_text("\n".join(["- nodes:", "  - {name: a0, host: localhost, port: 46200}",
                              "  - {name: a1, host: localhost, port: 46201}", "- fetch_probability: 1.0",
                              "- timeout_ms: 2500", "- interpolation: clock", "- divergence_threshold: 0",
                              "- constant: { value: 0.5 }", "- clock: 0", "- loss: 0"]) + "\n")
    data = [ref.inputs(lay, "normal"), ref.inputs(lay, "signed-zeros")]
    runs = {}
    for track in (False, True):
        kw = dict(track_distance="per_parameter", parameter_ranges=py_ranges(lay)) if track else {}
        grp = LocalGroup()
        conns = [DpwaConnection("a%d" % g, str(cfg), seed=40 + g, group=grp, **kw) for g in range(2)]
        flats = [to_dev(lay, data[0][g]) for g in range(2)]
        for r in range(2):
            snaps = [data[r][g] for g in range(2)]          # what each learner publishes
            mine = [data[r][1 - g] if r else data[1][g] for g in range(2)]   # what it holds at the average
            for g in range(2):
                flats[g].copy_(to_dev(lay, snaps[g]))
                conns[g].update_send(flats[g], 1.0 + g + r)
            for g in range(2):
                flats[g].copy_(to_dev(lay, mine[g]))
            DpwaConnection.update_wait_average_many(conns, flats, [0.5, 0.75], write_through=bool(r))
            if track:
                for g in range(2):
                    pd = conns[g].last_distance.parameters
                    got = pd.read()
                    check(lay, [got[n] for n, _, _, _ in lay.tensors], ref.reference(lay, mine[g], snaps[1 - g]),
                          "many round %d learner %d" % (r, g))
                    assert pd.clock == conns[g].clock
        torch.cuda.synchronize()
        runs[track] = ([f.cpu().view(torch.uint8).numpy().copy() for f in flats], [c.clock for c in conns],
                       [bytes(c._learner.read_coef()) for c in conns],
                       [snapshot_after(c, f, lay, True) for c, f in zip(conns, flats)])   # the last round wrote through
        assert all(np.array_equal(a, b) for a, b in zip(runs[track][0], runs[track][3]))
        for c in conns:
            c.close()
    assert all(np.array_equal(a, b) for a, b in zip(runs[False][0], runs[True][0]))
    assert runs[False][1:3] == runs[True][1:3]
    assert all(np.array_equal(a, b) for a, b in zip(runs[False][3], runs[True][3]))


def test_three_learners_with_different_options_in_one_dispatch(tmp_path):
    """Three co-resident learners in one batched dispatch, one with the whole-model record, one with
    "per_parameter", one with neither: two rounds, write-through off and then on.  Every learner's
    parameters are bit-equal to the same rounds with every option off; the first learner's record meets
    dist_ref's bound against the exact reference, and so does the record of the same learner when its
    average runs alone (the tracked kernel: the two are compared with the reference, never with each
    other, since the accumulation order is not fixed); the second learner's pairs meet pdist_ref's
    rule; the third has no record."""
    lay = LAYOUTS["A"]
    cfg = tmp_path / "three.yaml"
    cfg.write_text("\n".join(["- nodes:", *["  - {name: a%d, host: localhost, port: %d}" % (g, 46210 + g) for g in range(3)],
                              "- fetch_probability: 1.0", "- timeout_ms: 2500", "- interpolation: clock",
                              "- divergence_threshold: 0", "- constant: { value: 0.5 }", "- clock: 0", "- loss: 0"]) + "\n")
    data = [ref.inputs(lay, case) for case in ("normal", "signed-zeros", "subnormal-differences")]
    measuring = [dict(track_distance=True), dict(track_distance="per_parameter", parameter_ranges=py_ranges(lay)), {}]
    real = sum(lay.elements(t) for t in range(len(lay.tensors)))

    def run(options, alone):
        grp = LocalGroup()
        conns = [DpwaConnection("a%d" % g, str(cfg), seed=40 + g, group=grp, **options[g]) for g in range(3)]
        flats = [to_dev(lay, data[g][0]) for g in range(3)]
        for r in range(2):
            snaps = [data[(g + r) % 3][0] for g in range(3)]    # what each learner publishes
            mine = [data[(g + r) % 3][1] for g in range(3)]     # what it holds at the average
            for g in range(3):
                flats[g].copy_(to_dev(lay, snaps[g]))
                conns[g].update_send(flats[g], 1.0 + g + r)
            for g in range(3):
                flats[g].copy_(to_dev(lay, mine[g]))
            if alone:    # the first learner's average in a launch of its own, the others' in one dispatch
                got = [conns[0].update_wait_average(flats[0], 0.5, write_through=bool(r))]
                got += DpwaConnection.update_wait_average_many(conns[1:], flats[1:], [0.75, 0.6], write_through=bool(r))
            else:
                got = DpwaConnection.update_wait_average_many(conns, flats, [0.5, 0.75, 0.6], write_through=bool(r))
            assert all(snap is not None for snap, _ in got)
            peer = [snaps[int(snap.peer[1:])] for snap, _ in got]   # the snapshot each learner averaged with
            if options[0]:
                whole = conns[0].last_distance.read()
                parts = [(dt, ref.tensor_bits(lay, t, mine[0]), ref.tensor_bits(lay, t, peer[0]))
                         for t, (_, dt, _, _) in enumerate(lay.tensors)]
                want = dist_ref.reference_many(parts)
                for value, w in ((whole.dist2, want[0]), (whole.norm2, want[1])):
                    assert dist_ref.problem(value, w, real) is None, (alone, r, dist_ref.problem(value, w, real))
                assert whole.clock == conns[0].clock and conns[0].last_distance.parameters is None
            if options[1]:
                pd = conns[1].last_distance.parameters
                pairs = pd.read()
                check(lay, [pairs[n] for n, _, _, _ in lay.tensors], ref.reference(lay, mine[1], peer[1]),
                      "three round %d" % r)
                assert pd.clock == conns[1].clock
            assert conns[2].last_distance is None
        torch.cuda.synchronize()
        out = ([f.cpu().view(torch.uint8).numpy().copy() for f in flats], [c.clock for c in conns],
               [bytes(c._learner.read_coef()) for c in conns])
        for c in conns:
            c.close()
        return out

    off = run([{}, {}, {}], False)
    for alone in (False, True):
        on = run(measuring, alone)
        assert all(np.array_equal(a, b) for a, b in zip(off[0], on[0])), alone
        assert off[1:] == on[1:], alone


def test_zero_division_and_gated_off_rounds_leave_the_record(tmp_path):
    lay = LAYOUTS["A"]
    kw = dict(track_distance="per_parameter", parameter_ranges=py_ranges(lay))
    p, q = ref.inputs(lay, "normal")
    conn = DpwaConnection("w1", self_cfg(tmp_path, "loss"), seed=3, group=LocalGroup(), **kw)
    flat = to_dev(lay, q)
    conn.update_send(flat, 1.0)
    flat.copy_(to_dev(lay, p))
    conn.update_wait_average(flat, 0.5)
    first, count = raw_record(conn)
    assert count == len(lay.tensors) and conn.last_distance.parameters.read()["t1"][0] > 0.0
    conn.update_send(flat, 0.0)
    flat.copy_(to_dev(lay, q))
    conn.update_wait_average(flat, 0.0)                       # loss + peer loss == 0: nothing is averaged
    with pytest.raises(ZeroDivisionError):
        conn.synchronize()
    assert torch.equal(raw_record(conn)[0], first)
    conn.update_send(flat, 1.0)                               # and its rows were zeroed: the next round is its own
    flat.copy_(to_dev(lay, p))
    conn.update_wait_average(flat, 0.5)
    got = conn.last_distance.parameters.read()
    check(lay, [got[n] for n, _, _, _ in lay.tensors], ref.reference(lay, p, q), "the round after")
    conn.close()
    cfg = tmp_path / "off.yaml"
    write_self_cfg(cfg, 0.0, "clock", 0.0, None)              # fetch_probability 0: no round averages
    conn = DpwaConnection("w1", str(cfg), seed=3, group=LocalGroup(), **kw)
    flat = to_dev(lay, q)
    conn.update_send(flat, 1.0)
    before = raw_record(conn)[0]
    for _ in range(2):
        conn.update_send(flat, 1.0)
        conn.update_wait_average(flat, 1.0)
    assert conn.last_distance is None and torch.equal(raw_record(conn)[0], before)
    conn.close()


def test_first_measured_round_divides_by_zero(tmp_path):
    """The host knows which round launched the pass, not whether it averaged: ``parameters`` appears with
    the first measured round, and ``written`` says (with a sync) that this one wrote nothing."""
    lay = LAYOUTS["A"]
    kw = dict(track_distance="per_parameter", parameter_ranges=py_ranges(lay), distance_every=2)
    p, q = ref.inputs(lay, "normal")
    conn = DpwaConnection("w1", self_cfg(tmp_path, "loss"), seed=3, group=LocalGroup(), **kw)
    flat = to_dev(lay, q)
    for r, loss in enumerate((1.0, 0.0, 1.0, 1.0)):            # round 2, the first measured one, is the no-op
        flat.copy_(to_dev(lay, q))
        conn.update_send(flat, loss)
        flat.copy_(to_dev(lay, p))
        conn.update_wait_average(flat, loss)
        pd = conn.last_distance.parameters
        assert (pd is None) == (r == 0)
        if r == 1:
            with pytest.raises(ZeroDivisionError):
                conn.synchronize()
        if pd is not None:
            assert pd.measured_rounds() == (r + 1) // 2
            assert pd.written == (r == 3)
            if r < 3:
                assert pd.clock == 0.0 and not bool(pd.tensor().any())
    got = pd.read()
    check(lay, [got[n] for n, _, _, _ in lay.tensors], ref.reference(lay, p, q), "the second measured round")
    conn.close()


def test_distance_every_three(tmp_path):
    """distance_every=3 over 7 averaging rounds: the record's clock changes after rounds 3 and 6 only,
    each record is that round's operands', and the whole-model record follows every round."""
    lay = LAYOUTS["A"]
    kw = dict(track_distance="per_parameter", parameter_ranges=py_ranges(lay), distance_every=3)
    conn = DpwaConnection("w1", self_cfg(tmp_path), seed=3, group=LocalGroup(), **kw)
    flat = to_dev(lay, ref.inputs(lay, "normal")[0])
    conn.update_send(flat, 1.0)
    last = raw_record(conn)[0]
    changed = []
    for r in range(1, 8):
        p, q = ref.inputs(lay, ref.CASE_NAMES[r % 6])
        flat.copy_(to_dev(lay, q))
        conn.update_send(flat, 1.0)
        flat.copy_(to_dev(lay, p))
        conn.update_wait_average(flat, 1.0, write_through=bool(r % 2))
        now = raw_record(conn)[0]
        assert conn.last_distance.clock == conn.clock          # the whole-model record: every round
        if r < 3:
            assert conn.last_distance.parameters is None
        if not torch.equal(now, last):
            changed.append(r)
            pd = conn.last_distance.parameters
            got = pd.read()
            check(lay, [got[n] for n, _, _, _ in lay.tensors], ref.reference(lay, p, q), "round %d" % r)
            assert pd.clock == conn.clock
        last = now
    assert changed == [3, 6]
    conn.close()


# ---------------------------------------------------------------- 3. the adapter
def test_adapter_fp32_norms_in_a_bf16_body(tmp_path):
    cfg = tmp_path / "adapter.yaml"
    write_self_cfg(cfg, 1.0, "loss", 0.0, None)
    net = mixed_ref.mixed_net(torch.bfloat16).to(DEV)
    assert {p.dtype for p in net.parameters()} == {torch.float32, torch.bfloat16}
    ad = DpwaPyTorchAdapter(net, "w1", str(cfg), seed=3, group=LocalGroup(), track_distance="per_parameter",
                            distance_every=2)
    g = torch.Generator().manual_seed(9)
    names = [n for n, _ in net.named_parameters()]
    state_keys = sorted(ad.connection.state_dict()) if hasattr(ad.connection, "state_dict") else None
    for r in range(1, 5):
        ad.update_send(1.0)
        snap = {n: p.detach().cpu().clone() for n, p in net.named_parameters()}
        with torch.no_grad():
            for p in net.parameters():
                p.copy_((p.detach().cpu().float() + 0.05 * torch.randn(p.shape, generator=g)).to(p.dtype))
        host = {n: p.detach().cpu().clone() for n, p in net.named_parameters()}
        ad.update_wait(0.5)
        assert ad.last_distance is not None
        pd = ad.last_distance.parameters
        if r == 1:
            assert pd is None                                  # no measured round has averaged yet
            continue
        if r % 2:
            continue                                           # (the record is still round r - 1's)
        got, rel = pd.read(), pd.relative()
        assert list(got) == names == list(rel)
        t = pd.tensor()
        assert t.dtype == torch.float64 and t.device == DEV and tuple(t.shape) == (len(names), 2)
        assert sorted(map(tuple, t.cpu().tolist())) == sorted(got.values())
        assert pd.clock == ad.connection.clock
        for n in names:
            kind = "f32" if host[n].dtype == torch.float32 else "bf16"
            want = dist_ref.reference(kind, mixed_ref.tensor_bits(host[n]), mixed_ref.tensor_bits(snap[n]))
            for k in range(2):
                why = dist_ref.problem(got[n][k], want[k], host[n].numel())
                assert why is None, (r, n, why)
            assert rel[n] == (got[n][0] / got[n][1]) ** 0.5
            assert abs(rel[n] - (want[0] / want[1]) ** 0.5) <= 2 * dist_ref.bound(host[n].numel()) * rel[n]
    if state_keys is not None:
        assert sorted(ad.connection.state_dict()) == state_keys
    ad.connection.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals():
    lay = LAYOUTS["A"]
    n = lay.total_bytes // 4
    lib = _lib.load()
    arr = c_ranges(lay)
    me = Learner(DEV, n, torch.float32, _lib.Interp(_lib.INTERP_CLOCK, 0, 0.0, 0.0))
    p, count = ctypes.c_void_p(), ctypes.c_int64()
    assert lib.dpwa_learner_param_distance(me.handle, ctypes.byref(p), ctypes.byref(count)) == _lib.ERR_STATE
    assert lib.dpwa_learner_set_param_distance(me.handle, arr, len(lay.tensors), 0) == _lib.ERR_ARG      # every < 1
    assert b"every" in lib.dpwa_last_error()
    short = Learner(DEV, n - 64, torch.float32, _lib.Interp(_lib.INTERP_CLOCK, 0, 0.0, 0.0))
    assert lib.dpwa_learner_set_param_distance(short.handle, arr, len(lay.tensors), 1) == _lib.ERR_ARG   # do not fit
    assert b"outside the payload" in lib.dpwa_last_error()
    short.close()
    half = Learner(DEV, 2 * n, torch.bfloat16, _lib.Interp(_lib.INTERP_CLOCK, 0, 0.0, 0.0))
    assert lib.dpwa_learner_set_param_distance(half.handle, arr, len(lay.tensors), 1) == _lib.ERR_ARG    # another dtype
    half.close()
    # the relay's fused second phase on a learner that has it on (the other order, switching it on while
    # a fused phase is pending, needs a relay of two ranks: the test below)
    _lib.call("dpwa_learner_set_param_distance", me.handle, arr, len(lay.tensors), 1)
    _lib.call("dpwa_learner_relay_enable", me.handle, 2, 0)
    picks = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    assert lib.dpwa_learner_relay_phase2(me.handle, ptr(picks), 1, 1, 1, 1) == _lib.ERR_STATE
    assert b"dpwa_learner_set_param_distance" in lib.dpwa_last_error()
    _lib.call("dpwa_learner_set_param_distance", me.handle, None, 0, 1)                                  # off again
    # an unaligned parameter buffer: refused at the average, nothing queued, the fetch still pending
    _lib.call("dpwa_learner_set_param_distance", me.handle, arr, len(lay.tensors), 1)
    s = torch.cuda.current_stream()
    base = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
    me.attach_local(0, me)
    me.publish(base[:n], 1.0, s)
    me.fetch(0, me.version, True, s)
    for fn in ("dpwa_learner_average", "dpwa_learner_average_through"):
        rc = getattr(lib, fn)(me.handle, ptr(base[1:n + 1]), ctypes.c_double(1.0), None, ctypes.c_void_p(s.cuda_stream))
        assert rc == _lib.ERR_ARG and b"16-byte aligned" in lib.dpwa_last_error(), fn
    _lib.call("dpwa_learner_average", me.handle, ptr(base[:n]), 1.0, None, ctypes.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    me.close()


def test_set_param_distance_with_a_fused_relay_phase_pending():
    """Two ranks of a relay (tests/pdist_relay_worker.py) reach dpwa_learner_relay_phase2(fuse != 0):
    dpwa_learner_set_param_distance is then DPWA_ERR_STATE naming the pending phase and allocates
    nothing; after the fused average it is accepted, and the next fused second phase is refused."""
    from tests import pdist_relay_worker
    from tests.test_gpu_relay import first_failure, run_world
    reports = run_world(2, target=pdist_relay_worker.rank_main)
    assert first_failure(reports) is None, first_failure(reports)
    assert reports == {0: ("ok", 2), 1: ("ok", 2)}, reports
