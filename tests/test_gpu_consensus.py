"""The consensus of a group on the GPU (include/dpwa_hip.h ``dpwa_consensus``) against the host model of
tests/consensus_ref.py: the means bit for bit (NaN positions equal), the sums within the model's derived
summation bound; the stateless entries for one dtype and for a segmented payload, every refusal, the
learner entry through ``DpwaConnection.consensus`` in a LocalGroup (plain, write-through and resident
rounds against the snapshots oracle.gossip.simulate gives, and a run with the calls bit-equal to one
without), the adapter's parameter views, and lock-step ranks of a DistGroup (tests/consensus_worker.py).

Shapes are the smallest at which each case can go wrong (consensus_ref.grid says which input sets run at
which size and why).  Measured on the device, per dtype: see the printed figures of each case.

The segmented case fills the members' padding with zeros, as the layout's contract says it is (the layout
carries no element counts, so a kernel cannot tell padding from elements), and `out`'s padding with NaN
bytes before the call: the mean of the padding must be zeros and no sum may feel it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dpwa_amd import DpwaConnection, DpwaPyTorchAdapter, _lib
from dpwa_amd.flat import c_layout
from dpwa_amd.group import LocalGroup
from oracle import gossip as ogossip
from oracle import lerp as olerp
from tests import consensus_ref as ref
from tests import consensus_worker as worker
from tests import dist_ref as dr
from tests import dist_worker
from tests.test_gpu_group_dtypes import free_port, run_job
from tests.test_gpu_kernels import ptr, stream
from tests.test_gpu_self_peer import write_self_cfg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@functools.lru_cache(maxsize=None)
def workspace():
    """One zeroed workspace for every stateless call of this module: each call must leave it zero."""
    b = ctypes.c_int64()
    _lib.call("dpwa_consensus_workspace", ctypes.byref(b))
    return torch.zeros(b.value, dtype=torch.uint8, device=DEV)


def to_dev(dtype, bits):
    signed = np.ascontiguousarray(bits).view(np.int32 if dtype == "f32" else np.int16)
    return torch.from_numpy(signed.copy()).view(TORCH[dtype]).to(DEV)


def bits_of(dtype, t):
    t = t.detach().contiguous().cpu().reshape(-1)
    return t.view(torch.int32).numpy().view(np.uint32) if dtype == "f32" else t.view(torch.int16).numpy().view(np.uint16)


def poisoned(dtype, n):
    return to_dev(dtype, np.full(n, ref.POISON[dtype], dtype=dr.BITS[dtype]))


def fresh_record():
    return torch.full((128,), 0xa5, dtype=torch.uint8, device=DEV)


def read_record(t):
    rec = _lib.ConsensusRecord.from_buffer_copy(t.cpu().numpy().tobytes())
    return rec, {"norm2": rec.norm2, "spread2": rec.spread2, "member": list(rec.member_spread2)[:rec.members]}


def pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def call(dtype, srcs, n, out, ws, rec):
    _lib.call("dpwa_consensus", dr.CODE[dtype], pointers(srcs), len(srcs), n, ptr(out) if out is not None else None,
              ptr(ws) if ws is not None else None, ptr(rec) if rec is not None else None, stream(), None, None)


def check(what, dtype, G, n, got_bits, rec_t, want):
    bits, _, sums = want
    if got_bits is not None:
        assert ref.same_mean(dtype, got_bits, bits), (what, np.flatnonzero(got_bits != bits)[:8])
    if rec_t is not None:
        rec, got = read_record(rec_t)
        print("%s: norm2 %r ref %r, spread2 %r ref %r, bound %.3g" % (what, got["norm2"], sums["norm2"], got["spread2"],
                                                                      sums["spread2"], dr.bound(G * n)))
        assert (rec.n, rec.members, rec.reserved, rec.version) == (n, G, 0, 0), what
        assert list(rec.member_spread2)[G:] == [0.0] * (8 - G) and list(rec.pad) == [0, 0, 0], what
        why = ref.sums_problem(got, sums, n, G)
        assert why is None, (what, why)


@pytest.mark.parametrize("dtype,G,n,only", ref.grid(), ids=lambda v: "%s+%d" % (v[0], len(v) - 1) if isinstance(v, tuple) else str(v))
def test_stateless_matches_the_model(dtype, G, n, only):
    ws = workspace()
    for name, members in ref.cases(dtype, G, n, only):
        what = (dtype, G, n, name)
        want = ref.model(dtype, members)            # once, shared by the calls below
        srcs = [to_dev(dtype, m) for m in members]
        out, rec = poisoned(dtype, n), fresh_record()
        call(dtype, srcs, n, out, ws, rec)
        check(what, dtype, G, n, bits_of(dtype, out), rec, want)
        for s, m in zip(srcs, members):             # read-only
            assert np.array_equal(bits_of(dtype, s), m), what
        if name != "normal":
            continue
        # the mean alone and the measurement alone are the full call's; two calls back to back
        alone, rec2 = poisoned(dtype, n), fresh_record()
        call(dtype, srcs, n, alone, None, None)
        call(dtype, srcs, n, None, ws, rec2)
        assert np.array_equal(bits_of(dtype, alone), bits_of(dtype, out)), what
        check(what + ("measure-only",), dtype, G, n, None, rec2, want)
        rec3 = fresh_record()
        call(dtype, srcs, n, out, ws, rec3)
        check(what + ("again",), dtype, G, n, bits_of(dtype, out), rec3, want)
    torch.cuda.synchronize()
    assert not bool(ws.any()), "the workspace was not left zero"


def mixed_members(G, seed=3):
    """G segmented payloads of consensus_ref.mixed_layout: N(0,1) elements, zero padding."""
    lay = ref.mixed_layout()
    total = lay[-1][1] + lay[-1][2]
    rng = np.random.default_rng(seed)
    parts = [[dr.to_bits(d, rng.standard_normal(count)) for d, _, _, count in lay] for _ in range(G)]
    raw = np.zeros((G, total), dtype=np.uint8)
    for i in range(G):
        for (d, off, _, count), b in zip(lay, parts[i]):
            raw[i, off:off + count * dr.SIZE[d]] = b.view(np.uint8)
    return lay, total, parts, raw


def test_stateless_mixed_matches_the_model_segment_by_segment():
    G = 3
    lay, total, parts, raw = mixed_members(G)
    layout = c_layout(tuple((TORCH[d], off, length) for d, off, length, _ in lay))
    srcs = [torch.from_numpy(raw[i].copy()).to(DEV) for i in range(G)]
    out = torch.full((total,), 0xff, dtype=torch.uint8, device=DEV)          # NaN bytes everywhere
    rec_t = fresh_record()
    _lib.call("dpwa_consensus_mixed", ctypes.byref(layout), pointers(srcs), G, ptr(out), ptr(workspace()), ptr(rec_t),
              stream(), None, None)
    got = out.cpu().numpy()
    rec, sums = read_record(rec_t)
    wants = [ref.model(d, [parts[i][k] for i in range(G)]) for k, (d, _, _, _) in enumerate(lay)]
    slots = 0
    for (d, off, length, count), want in zip(lay, wants):
        seg = got[off:off + length]
        assert ref.same_mean(d, seg[:count * dr.SIZE[d]].view(dr.BITS[d]), want[0]), d
        assert not seg[count * dr.SIZE[d]:].any(), "%s: the padding's mean is not zeros" % d
        slots += length // dr.SIZE[d]
    assert (rec.n, rec.members, rec.version) == (slots, G, 0)
    elements = sum(count for _, _, _, count in lay)
    want = {"norm2": sum(w[2]["norm2"] for w in wants), "spread2": sum(w[2]["spread2"] for w in wants),
            "member": [sum(w[2]["member"][i] for w in wants) for i in range(G)]}
    print("mixed: got %r want %r" % (sums, want))
    assert ref.sums_problem(sums, want, elements + 3, G) is None, ref.sums_problem(sums, want, elements + 3, G)
    for s, r in zip(srcs, raw):
        assert np.array_equal(s.cpu().numpy(), r)
    # the mean alone and the measurement alone
    alone, rec2 = torch.full_like(out, 0xff), fresh_record()
    _lib.call("dpwa_consensus_mixed", ctypes.byref(layout), pointers(srcs), G, ptr(alone), None, None, stream(), None, None)
    _lib.call("dpwa_consensus_mixed", ctypes.byref(layout), pointers(srcs), G, None, ptr(workspace()), ptr(rec2), stream(),
              None, None)
    assert np.array_equal(alone.cpu().numpy(), got)
    assert ref.sums_problem(read_record(rec2)[1], want, elements + 3, G) is None
    assert not bool(workspace().any())


def test_every_refusal_returns_its_error_and_queues_nothing():
    lib = _lib.load()
    n = 1000
    srcs = [torch.ones(n, device=DEV) for _ in range(9)]
    out, rec, ws = torch.full((n + 8,), 7.0, device=DEV), fresh_record(), workspace()
    F32 = _lib.F32

    def refused(code, *args):
        assert lib.dpwa_consensus(*args) == code, (args, lib.dpwa_last_error())
        assert b"dpwa_consensus" in lib.dpwa_last_error()
    o, w, r, s = ptr(out), ptr(ws), ptr(rec), stream()
    two = pointers(srcs[:2])
    refused(_lib.ERR_ARG, F32, pointers(srcs), 0, n, o, w, r, s, None, None)
    refused(_lib.ERR_ARG, F32, pointers(srcs), 9, n, o, w, r, s, None, None)
    refused(_lib.ERR_ARG, F32, None, 2, n, o, w, r, s, None, None)
    refused(_lib.ERR_ARG, F32, (ctypes.c_void_p * 2)(srcs[0].data_ptr(), None), 2, n, o, w, r, s, None, None)
    refused(_lib.ERR_ARG, F32, (ctypes.c_void_p * 2)(srcs[0].data_ptr(), srcs[1].data_ptr() + 4), 2, n - 1, o, w, r, s,
            None, None)
    refused(_lib.ERR_ARG, F32, two, 2, n, ctypes.c_void_p(out.data_ptr() + 4), w, r, s, None, None)
    refused(_lib.ERR_ARG, F32, two, 2, n, ptr(srcs[1]), w, r, s, None, None)                       # out is a source
    refused(_lib.ERR_ARG, F32, two, 2, n, ctypes.c_void_p(srcs[0].data_ptr() + 16), w, r, s, None, None)   # overlaps one
    refused(_lib.ERR_ARG, F32, two, 2, n, o, None, r, s, None, None)
    refused(_lib.ERR_ARG, F32, two, 2, n, o, w, None, s, None, None)
    refused(_lib.ERR_ARG, F32, two, 2, n, None, None, None, s, None, None)
    refused(_lib.ERR_ARG, F32, two, 2, -1, o, w, r, s, None, None)
    refused(_lib.ERR_ARG, 7, two, 2, n, o, w, r, s, None, None)
    refused(_lib.ERR_ARG, _lib.MIXED, two, 2, n, o, w, r, s, None, None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((rec == 0xa5).all()) and not bool(ws.any())
    assert all(bool((t == 1.0).all()) for t in srcs)


# ---------------------------------------------------------------- learners of one process
NAMES = ["w1", "w2", "w3"]
N, T = 4099, 6


def write_cfg(path, names=NAMES):
    dist_worker.write_cfg(str(path), names, 1.0, "constant", 0.0)


def inputs():
    rng = np.random.default_rng(11)
    init = rng.standard_normal((len(NAMES), N)).astype(np.float32)
    deltas = (0.01 * rng.standard_normal((T, len(NAMES), N))).astype(np.float32)
    loss = [[1.0] * len(NAMES) for _ in range(T)]
    return init, deltas, loss


def run_rounds(tmp_path, form, with_calls):
    """Six rounds of three learners; what every round left, and what consensus() said after every
    update_send (`with_calls`)."""
    init, deltas, loss = inputs()
    cfg = tmp_path / ("c-%s-%d.yaml" % (form, with_calls))
    write_cfg(cfg)
    group = LocalGroup()
    G = len(NAMES)
    conns = [DpwaConnection(NAMES[g], str(cfg), seed=10 + g, group=group) for g in range(G)]
    flats = [torch.from_numpy(init[g].copy()).to(DEV) for g in range(G)]
    if form == "resident":
        for g in range(G):
            conns[g].make_resident(flats[g])
    params, clocks, peers, said = np.zeros((T, G, N), np.float32), np.zeros((T, G)), [], []
    for r in range(T):
        for g in range(G):
            conns[g].update_send(conns[g].parameters if form == "resident" else flats[g], loss[r][g],
                                 reuse_snapshot=form == "through" and r > 0)
        if with_calls:
            c = [conns[g].consensus() for g in range(G)]
            c.append(conns[1].consensus(out=False))                     # measure only
            c.append(conns[2].consensus(distance=False, members=["w3", "w1"]))
            said.append(c)
        if form != "resident":
            for g in range(G):
                flats[g].add_(torch.from_numpy(deltas[r, g]).to(DEV))
        row = []
        for g in range(G):
            buf = conns[g].parameters if form == "resident" else flats[g]
            payload, _ = conns[g].update_wait_average(buf, loss[r][g], write_through=form == "through")
            row.append(payload.peer if payload is not None else "")
        peers.append(row)
        if form == "resident":
            for g in range(G):
                params[r, g] = conns[g].parameters.cpu().numpy()
                conns[g].parameters.add_(torch.from_numpy(deltas[r, g]).to(DEV))
        else:
            for g in range(G):
                params[r, g] = flats[g].cpu().numpy()
        for g in range(G):
            clocks[r, g] = conns[g].clock
    results = []
    for c in said:
        results.append([(x.members, bits_of("f32", x.tensor()) if x._out is not None else None,
                         (x.read().norm2, x.read().spread2, list(x.read().member_spread2), x.version, x.distance,
                          x.relative, x.member_spread2) if x._record is not None else None) for x in c])
    for c in conns:
        c.close()
    return params, clocks, peers, results


@pytest.mark.parametrize("form", ["plain", "through", "resident"])
def test_learners_consensus_is_the_model_over_simulates_snapshots_and_changes_nothing(tmp_path, form):
    init, deltas, loss = inputs()
    G = len(NAMES)
    want = ogossip.simulate(NAMES, init, deltas, loss, loss, "constant", 0.5, 0.0, 1.0, [10, 11, 12],
                            train_after_wait=form == "resident")
    with_calls = run_rounds(tmp_path, form, True)
    without = run_rounds(tmp_path, form, False)
    for a, b in zip(with_calls[:2], without[:2]):               # every parameter and clock bit-equal
        assert a.tobytes() == b.tobytes()
    assert with_calls[2] == without[2]                          # and every peer choice
    assert olerp.bits_equal(with_calls[0], want["params"]) and np.array_equal(with_calls[1], want["clocks"])
    for r in range(T):
        if r == 0:
            snaps = init
        elif form == "resident":
            snaps = (want["params"][r - 1] + deltas[r - 1]).astype(np.float32)
        else:
            snaps = want["params"][r - 1]
        members = [snaps[g].view(np.uint32) for g in range(G)]
        model = ref.model("f32", members)
        for k, (names, bits, rec) in enumerate(with_calls[3][r]):
            what = (form, r, k)
            if k == 4:                                          # members=["w3", "w1"]: YAML order, two of them
                assert names == ["w1", "w3"] and rec is None, what
                assert ref.same_mean("f32", bits, ref.model("f32", [members[0], members[2]])[0]), what
                continue
            assert names == NAMES, what
            if k == 3:
                assert bits is None, what
            else:
                assert ref.same_mean("f32", bits, model[0]), what
            norm2, spread2, member, version, distance, relative, by_name = rec
            got = {"norm2": norm2, "spread2": spread2, "member": member[:G]}
            assert ref.sums_problem(got, model[2], N, G) is None, (what, ref.sums_problem(got, model[2], N, G))
            assert version == r + 1 and member[G:] == [0.0] * (8 - G), what
            assert distance == (spread2 / G) ** 0.5 and relative == (spread2 / (G * norm2)) ** 0.5, what
            assert list(by_name) == NAMES and list(by_name.values()) == member[:G], what


def test_a_self_peer_is_counted_once_and_a_member_behind_raises(tmp_path):
    cfg = tmp_path / "self.yaml"
    write_self_cfg(cfg, 1.0, "constant", 0.0, 0.5, port=48170)
    conn = DpwaConnection("w1", str(cfg), seed=20, group=LocalGroup())
    rng = np.random.default_rng(2)
    x = rng.standard_normal(N).astype(np.float32)
    flat = torch.from_numpy(x.copy()).to(DEV)
    conn.update_send(flat, 1.0)
    c = conn.consensus()
    assert c.members == ["w1"] and c.version == 1
    assert np.array_equal(bits_of("f32", c.tensor()), x.view(np.uint32)) and c.spread2 == 0.0
    why = dr.problem(c.norm2, dr.fsum(x.astype(np.float64) ** 2), N)
    assert why is None, why
    # the C entry: the self-peer's slot and -1 are one slot
    conn.update_wait_average(flat, 1.0)                # (attaches the self-peer as peer 0)
    ids = (ctypes.c_int32 * 2)(-1, 0)
    lib = _lib.load()
    out = torch.zeros(N, device=DEV)
    assert lib.dpwa_learner_consensus(conn._learner.handle, ids, 2, 1, ptr(out), None, stream()) == _lib.ERR_ARG
    assert b"same slot" in lib.dpwa_last_error()
    ids = (ctypes.c_int32 * 1)(5)
    assert lib.dpwa_learner_consensus(conn._learner.handle, ids, 1, 1, ptr(out), None, stream()) == _lib.ERR_ARG
    assert b"not attached" in lib.dpwa_last_error()
    ids = (ctypes.c_int32 * 1)(-1)
    assert lib.dpwa_learner_consensus(conn._learner.handle, ids, 1, 2, ptr(out), None, stream()) == _lib.ERR_STATE
    assert lib.dpwa_learner_consensus(conn._learner.handle, ids, 1, 1, None, None, stream()) == _lib.ERR_ARG
    assert lib.dpwa_learner_consensus(conn._learner.handle, ids, 0, 1, ptr(out), None, stream()) == _lib.ERR_ARG
    nine = (ctypes.c_int32 * 9)(-1, 0, 1, 2, 3, 4, 5, 6, 7)
    assert lib.dpwa_learner_consensus(conn._learner.handle, nine, 9, 1, ptr(out), None, stream()) == _lib.ERR_ARG
    assert b"9 members" in lib.dpwa_last_error()
    torch.cuda.synchronize()
    assert not bool(out.any())
    conn.close()
    # two learners, one a version behind
    cfg2 = tmp_path / "two.yaml"
    write_cfg(cfg2, NAMES[:2])
    group = LocalGroup()
    a = DpwaConnection("w1", str(cfg2), seed=1, group=group)
    b = DpwaConnection("w2", str(cfg2), seed=2, group=group)
    fa, fb = torch.from_numpy(x.copy()).to(DEV), torch.from_numpy(x.copy()).to(DEV)
    a.update_send(fa, 1.0)
    with pytest.raises(ValueError, match="w2"):
        a.consensus()
    assert a.consensus(members=["w1"]).members == ["w1"]
    b.update_send(fb, 1.0)
    assert a.consensus().members == ["w1", "w2"]
    with pytest.raises(ValueError, match="nobody"):
        a.consensus(members=["nobody"])
    a.update_wait_average(fa, 1.0)
    a.update_send(fa, 1.0)
    with pytest.raises(ValueError, match="w2"):
        a.consensus()
    a.close()
    b.close()


def test_nine_members_are_refused_eight_are_averaged_and_an_unlike_member_is_named(tmp_path):
    names = ["w%d" % (g + 1) for g in range(9)]
    cfg = tmp_path / "nine.yaml"
    write_cfg(cfg, names)
    group = LocalGroup()
    n = 517
    rng = np.random.default_rng(9)
    x = rng.standard_normal((9, n)).astype(np.float32)
    conns = [DpwaConnection(names[g], str(cfg), seed=g, group=group) for g in range(9)]
    flats = [torch.from_numpy(x[g].copy()).to(DEV) for g in range(9)]
    for g in range(9):
        conns[g].update_send(flats[g], 1.0)
    with pytest.raises(ValueError, match="at most 8 members"):
        conns[0].consensus()
    c = conns[4].consensus(members=names[:8])
    want = ref.model("f32", [x[g].view(np.uint32) for g in range(8)])
    assert c.members == names[:8] and ref.same_mean("f32", bits_of("f32", c.tensor()), want[0])
    rec = c.read()
    got = {"norm2": rec.norm2, "spread2": rec.spread2, "member": list(rec.member_spread2)}
    assert ref.sums_problem(got, want[2], n, 8) is None, ref.sums_problem(got, want[2], n, 8)
    for conn in conns:
        conn.close()
    # a member that holds another n cannot be attached: named, as a ValueError
    cfg2 = tmp_path / "unlike.yaml"
    write_cfg(cfg2, names[:2])
    group = LocalGroup()
    a = DpwaConnection("w1", str(cfg2), seed=1, group=group)
    b = DpwaConnection("w2", str(cfg2), seed=2, group=group)
    a.update_send(flats[0], 1.0)
    b.update_send(torch.zeros(n + 4, device=DEV), 1.0)
    with pytest.raises(ValueError, match="w2"):
        a.consensus()
    a.close()
    b.close()


def test_the_adapter_gives_the_parameters_of_the_consensus_model(tmp_path):
    """A bfloat16 body with float32 norms (a segmented payload), two adapters: parameters() tensor by
    tensor against the model of each parameter's own dtype, and load_into."""
    cfg = tmp_path / "ad.yaml"
    write_cfg(cfg, NAMES[:2])

    def net(seed):
        torch.manual_seed(seed)
        return torch.nn.Sequential(torch.nn.Linear(37, 11).bfloat16(), torch.nn.LayerNorm(11),
                                   torch.nn.Linear(11, 5).bfloat16()).to(DEV)
    nets = [net(1), net(2)]
    with torch.no_grad():
        for m in nets:
            m[1].weight.add_(torch.randn_like(m[1].weight))
    adapters = [DpwaPyTorchAdapter(nets[g], NAMES[g], str(cfg), seed=3 + g) for g in range(2)]
    before = [[p.detach().clone() for p in m.parameters()] for m in nets]
    for ad in adapters:
        ad.update_send(1.0)
    c = adapters[0].consensus()
    mean = c.parameters()
    assert list(mean) == [name for name, _ in nets[0].named_parameters()]
    total = 0.0
    for k, (name, p) in enumerate(nets[0].named_parameters()):
        d = "f32" if p.dtype == torch.float32 else "bf16"
        assert mean[name].shape == p.shape and mean[name].dtype == p.dtype, name
        want = ref.model(d, [bits_of(d, before[g][k]) for g in range(2)])
        assert ref.same_mean(d, bits_of(d, mean[name]), want[0]), name
        total += want[2]["spread2"]
    # G * elements terms on the device; `total` adds one exactly rounded sum per tensor
    terms = 2 * sum(p.numel() for p in nets[0].parameters()) + len(before[0])
    assert dr.problem(c.spread2, total, terms) is None, dr.problem(c.spread2, total, terms)
    for g in range(2):                                            # nothing changed
        for p, q in zip(nets[g].parameters(), before[g]):
            assert torch.equal(p.detach(), q)
    fresh = net(9)
    c.load_into(fresh)
    for (name, p) in fresh.named_parameters():
        assert torch.equal(p.detach(), mean[name]), name
    for ad in adapters:
        ad.close()


# ---------------------------------------------------------------- lock-step ranks
@pytest.mark.parametrize("world,pull,vmm", [(2, "copy", False), (3, "kernel:64", False), (3, "copy", True)])
def test_every_ranks_consensus_is_the_model_at_every_round(tmp_path, monkeypatch, world, pull, vmm):
    """DistGroup over gloo on one device, 10,243 float16 elements: every rank's mean of every round is
    bit-identical to the model over that round's snapshots (so to every other rank's), its sums within
    the bound; `vmm`: fd-shared slots."""
    if vmm:
        monkeypatch.setenv("DPWA_VMM", "1")
    names = ["w%d" % (g + 1) for g in range(world)]
    cfg = str(tmp_path / "dist.yaml")
    dist_worker.write_cfg(cfg, names, 1.0, "constant", 0.0)
    reports = run_job("consensus-%d-%s-%d" % (world, pull, vmm), world, worker.lockstep_main,
                      (pull, free_port(), cfg, str(tmp_path), vmm))
    assert reports == {r: ("ok", worker.ROUNDS) for r in range(world)}, reports
    runs = [np.load(tmp_path / ("rank%d.npz" % g)) for g in range(world)]
    for r in range(worker.ROUNDS):
        members = [runs[g]["snaps"][r] for g in range(world)]
        want = ref.model("f16", members)
        for g in range(world):
            assert ref.same_mean("f16", runs[g]["means"][r], want[0]), (g, r)
            got = {"norm2": runs[g]["sums"][r][0], "spread2": runs[g]["sums"][r][1],
                   "member": list(runs[g]["sums"][r][2:2 + world])}
            assert ref.sums_problem(got, want[2], worker.N, world) is None, (g, r, ref.sums_problem(got, want[2], worker.N, world))


def test_free_running_ranks_relay_avg_and_the_wire_are_refused(tmp_path):
    names = ["w1", "w2"]
    cfg = str(tmp_path / "refuse.yaml")
    dist_worker.write_cfg(cfg, names, 1.0, "constant", 0.0)
    reports = run_job("consensus-refusals", 2, worker.refusals_main, (free_port(), cfg))
    assert reports == {0: ("ok", 3), 1: ("ok", 3)}, reports
