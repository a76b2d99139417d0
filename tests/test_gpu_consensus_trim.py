"""The trimmed consensus on the GPU (include/dpwa_hip.h ``dpwa_consensus_trimmed``) against the plain numpy
model of its rule in tests/consensus_trim_ref.py: the centres bit for bit (NaN positions equal), the sums
within consensus_ref's summation bound -- stateless for one dtype over consensus_trim_ref.grid() (every
member count and trim, every input set, the sizes of consensus_ref), every ordering of the members' values
at once, a segmented payload for every member count, permutations of the members, through
``DpwaConnection.consensus(trim=...)`` for float32 and for groups of 6, 7 and 8 16-bit learners, across
lock-step ranks, and every refusal."""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

from dpwa_amd import DpwaConnection, _lib
from dpwa_amd.flat import c_layout
from dpwa_amd.group import LocalGroup
from tests import consensus_ref as ref
from tests import consensus_trim_ref as tr
from tests import consensus_worker as worker
from tests import dist_ref as dr
from tests import dist_worker
from tests.consensus_trim_ref import members_of, model
from tests.test_gpu_consensus import (DEV, TORCH, bits_of, fresh_record, mixed_members, pointers, poisoned, read_record,
                                      to_dev, workspace, write_cfg)
from tests.test_gpu_group_dtypes import free_port, run_job
from tests.test_gpu_kernels import ptr, stream

pytestmark = pytest.mark.gpu


def check(what, dtype, G, t, n, got_bits, rec_t, want):
    if got_bits is not None:
        assert ref.same_mean(dtype, got_bits, want[0]), (what, np.flatnonzero(got_bits != want[0])[:8])
    if rec_t is not None:
        rec, got = read_record(rec_t)
        assert (rec.n, rec.members, rec.reserved, rec.version) == (n, G, t, 0), what
        why = ref.sums_problem(got, want[1], n, G)
        assert why is None, (what, why)


def call(dtype, srcs, t, n, out, ws, rec):
    _lib.call("dpwa_consensus_trimmed", dr.CODE[dtype], pointers(srcs), len(srcs), t, n, ptr(out) if out is not None else None,
              ptr(ws) if ws is not None else None, ptr(rec) if rec is not None else None, stream(), None, None)


@pytest.mark.parametrize("size", range(5))
@pytest.mark.parametrize("G,t", [(3, 1), (4, 1), (5, 1), (5, 2), (8, 1), (8, 3)])
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_stateless_matches_the_model(dtype, G, t, size):
    ws, n = workspace(), ref.SMALL[dtype][size]
    for finite in (False, True):            # the hard values (a kept NaN: every sum is NaN), then sums that are numbers
        members = members_of(dtype, G, t, n, finite)
        want = model(dtype, members, t)
        assert math.isnan(want[1]["norm2"]) != finite
        srcs = [to_dev(dtype, m) for m in members]
        out, alone, rec, rec2 = poisoned(dtype, n), poisoned(dtype, n), fresh_record(), fresh_record()
        call(dtype, srcs, t, n, out, ws, rec)               # store + record, store only, record only
        call(dtype, srcs, t, n, alone, None, None)
        call(dtype, srcs, t, n, None, ws, rec2)
        check((finite, "full"), dtype, G, t, n, bits_of(dtype, out), rec, want)
        check((finite, "store"), dtype, G, t, n, bits_of(dtype, alone), None, want)
        check((finite, "record"), dtype, G, t, n, None, rec2, want)
    assert not bool(ws.any()), "the workspace was not left zero"


def test_stateless_mixed_matches_the_model_segment_by_segment():
    G, t = 5, 2
    lay, total, parts, raw = mixed_members(G)
    layout = c_layout(tuple((TORCH[d], off, length) for d, off, length, _ in lay))
    srcs = [torch.from_numpy(raw[i].copy()).to(DEV) for i in range(G)]
    out, rec_t = torch.full((total,), 0xff, dtype=torch.uint8, device=DEV), fresh_record()
    _lib.call("dpwa_consensus_trimmed_mixed", ctypes.byref(layout), pointers(srcs), G, t, ptr(out), ptr(workspace()),
              ptr(rec_t), stream(), None, None)
    got, (rec, sums) = out.cpu().numpy(), read_record(rec_t)
    wants = [model(d, [parts[i][k] for i in range(G)], t) for k, (d, _, _, _) in enumerate(lay)]
    for (d, off, length, count), want in zip(lay, wants):
        seg = got[off:off + length]
        assert ref.same_mean(d, seg[:count * dr.SIZE[d]].view(dr.BITS[d]), want[0]), d
        assert not seg[count * dr.SIZE[d]:].any(), "%s: the padding's centre is not zeros" % d
    assert (rec.members, rec.reserved) == (G, t)
    elements = sum(count for _, _, _, count in lay)
    want = {"norm2": sum(w[1]["norm2"] for w in wants), "spread2": sum(w[1]["spread2"] for w in wants),
            "member": [sum(w[1]["member"][i] for w in wants) for i in range(G)]}
    assert ref.sums_problem(sums, want, elements + 3, G) is None, ref.sums_problem(sums, want, elements + 3, G)
    assert not bool(workspace().any())


def test_member_order_does_not_matter():
    dtype, G, t, n = "bf16", 5, 1, 513
    members = members_of(dtype, G, t, n, finite=True)
    want = model(dtype, members, t)
    perm = [3, 0, 4, 2, 1]
    out, rec = poisoned(dtype, n), fresh_record()
    call(dtype, [to_dev(dtype, members[p]) for p in perm], t, n, out, workspace(), rec)
    permuted = dict(want[1], member=[want[1]["member"][p] for p in perm])
    check("permuted", dtype, G, t, n, bits_of(dtype, out), rec, (want[0], permuted))


NAMES, N = ["w1", "w2", "w3", "w4"], 4099


def published(tmp_path, count):
    """`count` connections of one LocalGroup after one update_send; w2 has a slice scaled by 2**20 and a NaN."""
    cfg = tmp_path / "trim.yaml"
    write_cfg(cfg, NAMES[:count])
    rng = np.random.default_rng(21)
    x = rng.standard_normal((count, N)).astype(np.float32)
    x[1, 1000:1500] *= 2.0 ** 20
    x[1, 7] = np.nan
    group = LocalGroup()
    conns = [DpwaConnection(NAMES[g], str(cfg), seed=g, group=group) for g in range(count)]
    flats = [torch.from_numpy(x[g].copy()).to(DEV) for g in range(count)]
    for c, f in zip(conns, flats):
        c.update_send(f, 1.0)
    return conns, flats, x


def test_through_the_public_interface(tmp_path):
    conns, flats, x = published(tmp_path, 3)
    members = [x[g].view(np.uint32) for g in range(3)]
    before = [(c.clock, c._learner.version) for c in conns]
    c = conns[0].consensus(trim="median")
    want = model("f32", members, 1)
    assert c.trim == 1 and c.members == NAMES[:3] and c.read().reserved == 1 and c.version == 1
    assert ref.same_mean("f32", bits_of("f32", c.tensor()), want[0]) and bool(torch.isfinite(c.tensor()).all())
    rec = c.read()
    got = {"norm2": rec.norm2, "spread2": rec.spread2, "member": list(rec.member_spread2)[:3]}
    assert ref.sums_problem(got, want[1], N, 3) is None, ref.sums_problem(got, want[1], N, 3)
    # the bad member by name: its own NaN makes its sum NaN (the rule's diagnostic), which counts as the largest
    sp = c.member_spread2
    assert max(sp, key=lambda k: math.inf if math.isnan(sp[k]) else sp[k]) == "w2" and math.isnan(sp["w2"])
    assert all(math.isfinite(sp[k]) for k in ("w1", "w3"))
    plain = conns[0].consensus()                                     # no trim: the mean, unchanged
    assert plain.trim == 0 and plain.read().reserved == 0
    assert ref.same_mean("f32", bits_of("f32", plain.tensor()), ref.model("f32", members)[0])
    assert [(c.clock, c._learner.version) for c in conns] == before
    assert all(np.array_equal(bits_of("f32", f), m) for f, m in zip(flats, members))
    with pytest.raises(ValueError, match="G = 3 members: the largest trim is 1"):
        conns[0].consensus(trim=2)
    for conn in conns:
        conn.close()


def test_every_refusal_returns_its_error_and_queues_nothing(tmp_path):
    lib = _lib.load()
    conns, flats, _ = published(tmp_path, 4)
    ids = (ctypes.c_int32 * 4)(*[pid for _, pid in conns[0]._group.consensus_sources(conns[0], None)])
    srcs = pointers([torch.ones(N, device=DEV) for _ in range(4)])
    out, rec, ws = torch.full((N + 8,), 7.0, device=DEV), fresh_record(), workspace()
    handle, s, odd = conns[0]._learner.handle, stream(), ctypes.c_void_p(out.data_ptr() + 4)
    for count, t, o in [(2, 1, ptr(out)), (4, 0, ptr(out)), (4, 2, ptr(out)), (4, 1, odd)]:
        assert lib.dpwa_consensus_trimmed(_lib.F32, srcs, count, t, N, o, ptr(ws), ptr(rec), s, None, None) == _lib.ERR_ARG
        assert b"dpwa_consensus_trimmed:" in lib.dpwa_last_error()
        assert lib.dpwa_learner_consensus_trimmed(handle, ids, count, t, 1, o, ptr(rec), s) == _lib.ERR_ARG
        assert b"dpwa_learner_consensus_trimmed:" in lib.dpwa_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((rec == 0xa5).all()) and not bool(ws.any())
    for conn in conns:
        conn.close()


# ---------------------------------------------------------------- every member count, trim and input set
def run_sets(dtype, G, t, n, only):
    """Every wanted set of one (dtype, G, t, n) through the three call forms against one model each."""
    ws, spent = workspace(), 0.0
    for name, members in tr.cases(dtype, G, t, n, only):
        start = time.perf_counter()
        want = model(dtype, members, t)             # once, shared by the calls below
        spent += time.perf_counter() - start
        srcs = [to_dev(dtype, m) for m in members]
        out, alone, rec, rec2 = poisoned(dtype, n), poisoned(dtype, n), fresh_record(), fresh_record()
        call(dtype, srcs, t, n, out, ws, rec)               # store + record, store only, record only
        call(dtype, srcs, t, n, alone, None, None)
        call(dtype, srcs, t, n, None, ws, rec2)
        got = read_record(rec)[1]
        print("%s: norm2 %r ref %r, spread2 %r ref %r, bound %.3g" % ((dtype, G, t, n, name), got["norm2"], want[1]["norm2"],
                                                                      got["spread2"], want[1]["spread2"], dr.bound(G * n)))
        check((name, "full"), dtype, G, t, n, bits_of(dtype, out), rec, want)
        check((name, "store"), dtype, G, t, n, bits_of(dtype, alone), None, want)
        check((name, "record"), dtype, G, t, n, None, rec2, want)
        for s, m in zip(srcs, members):             # read-only
            assert np.array_equal(bits_of(dtype, s), m), name
    torch.cuda.synchronize()
    assert not bool(ws.any()), "the workspace was not left zero"
    print("host model: %.2f s" % spent)


@pytest.mark.parametrize("dtype,G,t,n,only", tr.grid(),
                         ids=lambda v: "+".join(w[0] if len(w) < 12 else w.split("-")[-1] for w in v) if isinstance(v, tuple) else str(v))
def test_the_grid_matches_the_model(dtype, G, t, n, only):
    run_sets(dtype, G, t, n, only)


@pytest.mark.parametrize("G", range(3, 9))
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_every_ordering_of_the_members_values(dtype, G):
    """`orders`, whole: every permutation and every single tie in both halves of a dword, at the smallest
    and the largest trim."""
    for t in sorted({1, (G - 1) // 2}):
        run_sets(dtype, G, t, tr.orders_size(G), ("orders",))


def mixed_from(G, t, name):
    """G segmented payloads of consensus_ref.mixed_layout: every segment's elements are the set `name` of its
    dtype and count, the padding zeros."""
    lay = ref.mixed_layout()
    total = lay[-1][1] + lay[-1][2]
    parts = [[None] * len(lay) for _ in range(G)]
    raw = np.zeros((G, total), dtype=np.uint8)
    for k, (d, off, _, count) in enumerate(lay):
        for i, b in enumerate(dict(tr.cases(d, G, t, count, (name,)))[name]):
            parts[i][k] = b
            raw[i, off:off + count * dr.SIZE[d]] = b.view(np.uint8)
    return lay, total, parts, raw


@pytest.mark.parametrize("G,t", sorted({(G, t) for G in range(3, 9) for t in (1, (G - 1) // 2)}))
def test_stateless_mixed_matches_the_model_for_every_member_count(G, t):
    for name in ("finite", "specials", "orders"):
        lay, total, parts, raw = mixed_from(G, t, name)
        layout = c_layout(tuple((TORCH[d], off, length) for d, off, length, _ in lay))
        srcs = [torch.from_numpy(raw[i].copy()).to(DEV) for i in range(G)]
        out, alone = (torch.full((total,), 0xff, dtype=torch.uint8, device=DEV) for _ in range(2))      # NaN bytes everywhere
        rec_t = fresh_record()
        _lib.call("dpwa_consensus_trimmed_mixed", ctypes.byref(layout), pointers(srcs), G, t, ptr(out), ptr(workspace()),
                  ptr(rec_t), stream(), None, None)
        _lib.call("dpwa_consensus_trimmed_mixed", ctypes.byref(layout), pointers(srcs), G, t, ptr(alone), None, None,
                  stream(), None, None)
        got, (rec, sums) = out.cpu().numpy(), read_record(rec_t)
        wants = [model(d, [parts[i][k] for i in range(G)], t) for k, (d, _, _, _) in enumerate(lay)]
        for (d, off, length, count), want in zip(lay, wants):
            seg = got[off:off + length]
            assert ref.same_mean(d, seg[:count * dr.SIZE[d]].view(dr.BITS[d]), want[0]), (name, d)
            assert not seg[count * dr.SIZE[d]:].any(), "%s: the padding's centre is not zeros" % d
        assert np.array_equal(alone.cpu().numpy(), got), name
        slots = sum(length // dr.SIZE[d] for d, _, length, _ in lay)
        assert (rec.n, rec.members, rec.reserved, rec.version) == (slots, G, t, 0), name
        elements = sum(count for _, _, _, count in lay)
        want = {"norm2": sum(w[1]["norm2"] for w in wants), "spread2": sum(w[1]["spread2"] for w in wants),
                "member": [sum(w[1]["member"][i] for w in wants) for i in range(G)]}
        print("mixed %s: got %r want %r" % (name, sums, want))
        assert ref.sums_problem(sums, want, elements + 3, G) is None, (name, ref.sums_problem(sums, want, elements + 3, G))
        for s, r in zip(srcs, raw):
            assert np.array_equal(s.cpu().numpy(), r)
    assert not bool(workspace().any())


@pytest.mark.parametrize("G,t", tr.PAIRS)
def test_member_order_does_not_matter_for_any_pair(G, t):
    dtype, n = "bf16", 513
    members = members_of(dtype, G, t, n, finite=True)
    want = model(dtype, members, t)
    for perm in (list(np.random.default_rng(60 + 10 * G + t).permutation(G)), list(reversed(range(G)))):
        out, rec = poisoned(dtype, n), fresh_record()
        call(dtype, [to_dev(dtype, members[p]) for p in perm], t, n, out, workspace(), rec)
        permuted = dict(want[1], member=[want[1]["member"][p] for p in perm])
        check(("permuted", perm), dtype, G, t, n, bits_of(dtype, out), rec, (want[0], permuted))


@pytest.mark.parametrize("dtype,count", [("bf16", 6), ("bf16", 7), ("f16", 8)])
def test_16_bit_learners_through_the_public_interface(tmp_path, dtype, count):
    """A LocalGroup of 6, 7 and 8 16-bit connections (the networks of 6, 7 and 8 behind the learner entry):
    w2 has a slice scaled up and a NaN, as in published()."""
    names = ["w%d" % (g + 1) for g in range(count)]
    cfg = tmp_path / "trim16.yaml"
    write_cfg(cfg, names)
    rng = np.random.default_rng(22 + count)
    x = rng.standard_normal((count, N)).astype(np.float32)
    x[1, 1000:1500] *= 2.0 ** (20 if dtype == "bf16" else 10)
    x[1, 7] = np.nan
    group = LocalGroup()
    conns = [DpwaConnection(names[g], str(cfg), seed=g, group=group) for g in range(count)]
    flats = [torch.from_numpy(x[g].copy()).to(TORCH[dtype]).to(DEV) for g in range(count)]
    members = [bits_of(dtype, f) for f in flats]
    for c, f in zip(conns, flats):
        c.update_send(f, 1.0)
    before = [(c.clock, c._learner.version) for c in conns]
    for trim, t in ((1, 1), ("median", (count - 1) // 2)):
        c = conns[count - 1].consensus(trim=trim)
        want = model(dtype, members, t)
        rec = c.read()
        assert c.trim == t and c.members == names and rec.reserved == t and c.version == 1 and rec.members == count
        assert c.tensor().dtype == TORCH[dtype] and rec.n == N
        assert ref.same_mean(dtype, bits_of(dtype, c.tensor()), want[0]) and bool(torch.isfinite(c.tensor()).all())
        got = {"norm2": rec.norm2, "spread2": rec.spread2, "member": list(rec.member_spread2)[:count]}
        assert ref.sums_problem(got, want[1], N, count) is None, (trim, ref.sums_problem(got, want[1], N, count))
        assert math.isnan(c.member_spread2["w2"]) and all(math.isfinite(v) for k, v in c.member_spread2.items() if k != "w2")
        assert list(rec.member_spread2)[count:] == [0.0] * (8 - count)
    assert [(c.clock, c._learner.version) for c in conns] == before
    assert all(np.array_equal(bits_of(dtype, f), m) for f, m in zip(flats, members))
    for conn in conns:
        conn.close()


def test_every_ranks_median_is_the_model_at_every_round(tmp_path):
    """Three lock-step ranks, ``consensus(trim="median")``: the remote acquire in front of the trimmed kernel."""
    world, pull = 3, "kernel:64"
    names = ["w%d" % (g + 1) for g in range(world)]
    cfg = str(tmp_path / "dist.yaml")
    dist_worker.write_cfg(cfg, names, 1.0, "constant", 0.0)
    reports = run_job("consensus-trim-%d" % world, world, worker.lockstep_main, (pull, free_port(), cfg, str(tmp_path), False, "median"))
    assert reports == {r: ("ok", worker.ROUNDS) for r in range(world)}, reports
    runs = [np.load(tmp_path / ("rank%d.npz" % g)) for g in range(world)]
    for r in range(worker.ROUNDS):
        want = model("f16", [runs[g]["snaps"][r] for g in range(world)], 1)
        for g in range(world):
            assert ref.same_mean("f16", runs[g]["means"][r], want[0]), (g, r)
            got = {"norm2": runs[g]["sums"][r][0], "spread2": runs[g]["sums"][r][1], "member": list(runs[g]["sums"][r][2:2 + world])}
            assert ref.sums_problem(got, want[1], worker.N, world) is None, (g, r, ref.sums_problem(got, want[1], worker.N, world))
