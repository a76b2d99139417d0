"""The trimmed consensus on the GPU (include/dpwa_hip.h ``dpwa_consensus_trimmed``) against a plain numpy
model of its rule: the centres bit for bit (NaN positions equal), the sums within consensus_ref's
summation bound -- stateless for one dtype and for a segmented payload, under a permutation of the
members, through ``DpwaConnection.consensus(trim=...)``, and every refusal."""
import ctypes
import math

import numpy as np
import pytest
import torch

from dpwa_amd import DpwaConnection, _lib
from dpwa_amd.flat import c_layout
from dpwa_amd.group import LocalGroup
from tests import consensus_ref as ref
from tests import dist_ref as dr
from tests.test_gpu_consensus import (DEV, TORCH, bits_of, fresh_record, mixed_members, pointers, poisoned, read_record,
                                      to_dev, workspace, write_cfg)
from tests.test_gpu_kernels import ptr, stream

pytestmark = pytest.mark.gpu


def model(dtype, members, t):
    """(centre bits, sums) of the members' bit patterns: the header's rule in numpy."""
    G, top = len(members), 8 * dr.SIZE[dtype] - 1
    b = np.stack(members).astype(np.uint64)
    key = b ^ np.where(b >> top, (1 << (top + 1)) - 1, 1 << top).astype(np.uint64)
    x = np.stack([dr.widen(dtype, m) for m in members])
    y = np.take_along_axis(x, np.argsort(key, axis=0, kind="stable"), axis=0)
    with np.errstate(all="ignore"):
        s = np.full(x.shape[1], -0.0)
        for i in range(t, G - t):
            s = s + y[i]
        m = s * (1.0 / (G - 2 * t))
        bits = ref.round16(dtype, m.astype(np.float32))
        spread = [(xi - m) * (xi - m) for xi in x]
        sums = {"norm2": dr.fsum(m * m), "member": [dr.fsum(v) for v in spread], "spread2": dr.fsum(np.concatenate(spread))}
    return bits, sums


def members_of(dtype, G, t, n, finite=False):
    """One seeded normal draw; member 1 scaled by 2**20; then, in fixed columns -- the last full lane and
    the tail element among them -- duplicates, +0 against -0, a subnormal, one NaN member, +inf and -inf
    in two members, and t + 1 NaNs of one sign (one of them is kept: the centre must be NaN, and with it
    every sum).  `finite`: without the NaNs and infinities, so that the sums are numbers to compare."""
    rng = np.random.default_rng(1000 * G + 10 * t + n)
    vals = rng.standard_normal((G, n))
    vals[1] *= 2.0 ** 20
    with np.errstate(over="ignore"):
        B = np.stack([dr.to_bits(dtype, v) for v in vals])
    neg, nan, inf, sub = dr.NEG_ZERO[dtype], dr.NAN[dtype], dr.INF[dtype], dr.SUBNORMAL[dtype]
    plants = [(slice(0, t + 1), nan), ([0, 2], [inf, inf | neg]), (G - 1, nan), ([0, 1], [sub, sub | neg]),
              (slice(None), np.where(np.arange(G) % 2 == 0, 0, neg)), None]        # (rows, their bits); None: duplicates
    whole = n // dr.ITEM[dtype] * dr.ITEM[dtype]
    for k in reversed(range(3 if finite else 0, 6)):            # (plant 0 last: it wins the tail element and the last full lane)
        for j in {(5 + 37 * k) % n, (whole - 1 - k) % n, (n - 1 - k) % n}:
            if plants[k] is None:
                B[1:3, j] = B[0, j]
            else:
                B[plants[k][0], j] = plants[k][1]
    return list(B)


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
