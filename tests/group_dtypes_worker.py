"""One rank of a job of tests/test_gpu_group_dtypes.py: a float16 or mixed-dtype (segmented) model through
DpwaConnection under the lock-step DistGroup or the free-running AsyncDistGroup (torch.distributed over
gloo, every rank on GPU 0), or two learners of unlike layouts or dtypes that must refuse each other's
exported handle.  The cases, inputs and expected values are tests/group_ref.py's.

The group jobs record every round's parameters, clock and peer and leave the comparing to the parent, as
tests/dist_worker.py does.  Processes start and end through tests/relay_worker.rank_main: a report to the
parent whatever happens, and no rank frees memory before every rank's GPU work is over.
"""
import datetime
import os
import struct

import numpy as np

from tests import group_ref as ref
from tests import mixed_ref, relay_worker
from tests.relay_worker import HANDLE

DIST_TIMEOUT_S = 90        # of every gloo collective: a rank that has stopped ends the others, not a hang


def to_device(kind, a, dev):
    """A payload (float16 bit patterns, or a segmented payload's bytes) as a device tensor."""
    import torch
    a = np.array(a)
    if kind == "f16":
        return torch.from_numpy(a.view(np.int16)).to(dev).view(torch.float16)
    return torch.from_numpy(a).to(dev)


def to_host(kind, t):
    import torch
    if kind == "f16":
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def train(kind, flat, delta):
    """The training step: ``add_`` in every segment's own dtype."""
    if kind == "f16":
        flat.add_(delta)
        return
    for d, off, _, n in ref.segments(kind)[0]:
        end = off + n * mixed_ref.SIZE[d]
        flat[off:end].view(mixed_ref.TORCH[d]).add_(delta[off:end].view(mixed_ref.TORCH[d]))


def torch_layout(kind):
    lay = ref.layout(kind)
    return None if lay is None else tuple((mixed_ref.TORCH[d], off, length) for d, off, length in lay)


def _init_group(rank, world, port):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=DIST_TIMEOUT_S))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    return dist, dev


def run_lockstep(shared, rank, world, args):
    """The lock-step jobs (group_ref "walk", "resident", "vmm"): the pulls of the case's phases in one
    connection, switched with set_pull on every rank before the same round."""
    job, kind, port, cfg_path, out_dir = args
    import torch
    dist, dev = _init_group(rank, world, port)
    from dpwa_amd import DpwaConnection
    from dpwa_amd.dpwa import MIXED_RELAY_AVG
    from dpwa_amd.group import DistGroup
    c = ref.case(job, kind, world)
    T = ref.rounds(c)
    init, deltas, send, wait = ref.case_inputs(c)
    resident = job == "resident"
    conn = DpwaConnection(ref.names(c)[rank], cfg_path, seed=ref.seeds(c)[rank], pull="relay:8", group="lockstep",
                          layout=torch_layout(kind))
    assert type(conn._group) is DistGroup
    flat = to_device(kind, init[rank], dev)
    steps = [to_device(kind, deltas[r, rank], dev) for r in range(T)]
    params, clocks, peers = np.zeros((T,) + init.shape[1:], init.dtype), np.zeros(T), []
    for r in range(T):
        pull, first = ref.pull_at(c, r)
        if first:
            conn.set_pull(pull)
            if kind == "mixed":          # refused before the bind and after it, and nothing changes
                try:
                    conn.set_pull("relay-avg:8")
                except ValueError as e:
                    assert str(e) == MIXED_RELAY_AVG, str(e)
                else:
                    raise AssertionError("round %d: a mixed connection accepted set_pull('relay-avg:8')" % r)
                assert conn._pull == pull
            if resident and r == 0:
                conn.make_resident(flat)
        if resident:
            assert conn.parameters.dtype == flat.dtype and conn.parameters.numel() == flat.numel()
            conn.update_send(conn.parameters, send[r][rank])
            payload, _ = conn.update_wait_average(conn.parameters, wait[r][rank])
            params[r] = to_host(kind, conn.parameters)
            clocks[r] = conn.clock
            train(kind, conn.parameters, steps[r])                     # the step, after update_wait
        else:
            conn.update_send(flat, send[r][rank])
            train(kind, flat, steps[r])
            if r % 2:
                payload, _ = conn.update_wait(wait[r][rank])           # split: factor kernel, then lerp
                if payload is not None:
                    conn.average(flat)
            else:
                payload, _ = conn.update_wait_average(flat, wait[r][rank])
            params[r] = to_host(kind, flat)
            clocks[r] = conn.clock
        peers.append(payload.peer if payload is not None else "")
        if r == 0:                       # the slots are shared the way the job says
            fds, _ = conn._learner.export_fds(0)
            for fd in fds:
                os.close(fd)
            assert bool(fds) == (job == "vmm"), (job, len(fds))
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), params=params, clocks=clocks, peers=np.array(peers))
    torch.cuda.synchronize()
    dist.barrier()
    conn.close()
    dist.destroy_process_group()
    return T


def lockstep_main(rank, world, shared, args):
    relay_worker.rank_main(rank, world, shared, args, run=run_lockstep)


def run_board(shared, rank, world, args):
    """Free-running rounds with write-through snapshots (tests/dist_worker.async_wt_worker's shape):
    update_send publishes what the last average left, the "training step" sets the parameters to
    base(rank, r), the average writes the next snapshot."""
    kind, port, cfg_path, out_dir = args
    import torch
    dist, dev = _init_group(rank, world, port)
    from dpwa_amd import DpwaConnection
    from dpwa_amd.group import AsyncDistGroup
    from oracle.async_check import async_loss
    c = ref.case("board", kind, world)
    T, pull = ref.rounds(c), c.phases[0][0]
    n = ref.N_F16 if kind == "f16" else ref.nbytes(kind)
    base = ref.base(kind)
    conn = DpwaConnection(ref.names(c)[rank], cfg_path, seed=ref.seeds(c)[rank], pull=pull, layout=torch_layout(kind))
    assert type(conn._group) is AsyncDistGroup            # the default under torch.distributed
    rng = np.random.default_rng(rank + 10)
    flat = to_device(kind, base(rank, -1, n), dev)
    bases = [to_device(kind, base(rank, r, n), dev) for r in range(T)]
    params, clocks, peers, versions = np.zeros((T, n), base(rank, 0, n).dtype), np.zeros(T), [], []
    for r in range(T):
        conn.update_send(flat, async_loss(rank, r), reuse_snapshot=True)
        flat.copy_(bases[r])
        torch.cuda._sleep(int(rng.integers(0, 400_000)))
        payload, _ = conn.update_wait_average(flat, async_loss(rank, r, wait=True), write_through=True)
        peers.append(payload.peer if payload is not None else "")
        versions.append(conn._info()[2] if payload is not None else 0)
        params[r] = to_host(kind, flat)
        clocks[r] = conn.clock
        if r == 0:
            # the one meeting of the run: every rank has published once, so from round 1 on a fetch always
            # finds a snapshot, however far apart the processes started (these payloads take microseconds)
            shared.wait()
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), params=params, clocks=clocks, peers=np.array(peers),
             versions=np.array(versions, dtype=np.int64))
    shared.wait()                        # no collective per round; nobody reads this rank's slots any more
    conn.close()
    return T


def board_main(rank, world, shared, args):
    relay_worker.rank_main(rank, world, shared, args, run=run_board)


# ---------------------------------------------------------------- refusals across processes, learner level
_FMT = "<4q64s"      # address length, fds, chunk bytes, pid, address: on the board in the header's place


def _exchange(shared, rank, lr):
    """Publishes this rank's exported handle (and serves its fds, if its slots are fd-shared) and returns
    what attaching the other rank's gave: None, or the DpwaError.  Both ranks leave together."""
    from dpwa_amd import _lib
    from dpwa_amd.group import _FdServer, _fetch_fds
    other = 1 - rank
    fds, chunk = lr.export_fds(0)
    server = _FdServer(fds, 1) if fds else None
    address = server.address.encode() if server else b""
    shared.put(rank, 0, lr.ipc_handle())
    shared.put(rank, 2 * HANDLE, struct.pack(_FMT, len(address), len(fds), chunk, os.getpid(), address))
    error = None
    try:
        shared.wait()
        alen, n_fds, chunk_other, pid, addr = struct.unpack(_FMT, shared.get(other, 2 * HANDLE, struct.calcsize(_FMT)))
        if server is not None:
            server.allow([pid])
        theirs = _fetch_fds(addr[:alen].decode(), n_fds) if alen else []
        try:
            if n_fds:
                lr.attach_fds(0, shared.get(other, 0, HANDLE), theirs, chunk_other)
            else:
                lr.attach_ipc(0, shared.get(other, 0, HANDLE))
        except _lib.DpwaError as e:
            error = e
        finally:
            for fd in theirs:
                os.close(fd)
    except BaseException:
        if server is not None:
            server.abort()
            server.thread.join(5)
            for fd in server.fds:
                os.close(fd)
            server.fds = []
        raise
    if server is not None:
        server.finish()
    shared.wait()                        # both have attached, or been refused: the handles are done with
    return error, bool(fds)


def run_refusals(shared, rank, world, vmm):
    """Rank 0 and rank 1 hold learners that must not average with each other -- two layouts of equal
    bytes, then float16 against bfloat16 at equal n: each rank's attach of the other's handle is
    DPWA_ERR_ARG naming the reason, and a fetch of that peer says it is not attached.  Then a control pair
    of equal layouts attaches, fetches and averages."""
    import torch
    from dpwa_amd import _lib
    from dpwa_amd.learner import Learner
    assert world == 2
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, ref.CONTROL_FACTOR, 0.0)
    fn = "dpwa_learner_attach_fds" if vmm else "dpwa_learner_attach_ipc"

    def learner(spec=None, dtype=None):
        if spec is None:
            return Learner(dev, ref.REFUSED_N, mixed_ref.TORCH[dtype], cfg)
        lay, total = ref.layout_of(spec)
        return Learner(dev, total, torch.uint8, cfg, layout=tuple((mixed_ref.TORCH[d], off, n) for d, off, n in lay))

    def refused(lr, why):
        error, shared_as_fds = _exchange(shared, rank, lr)
        assert shared_as_fds == bool(vmm), "the slots are %sshared as fds" % ("" if shared_as_fds else "not ")
        assert error is not None, "%s: the attach was accepted" % why
        assert error.code == _lib.ERR_ARG and fn in str(error) and why in str(error), str(error)
        try:
            lr.fetch(0, 1, False, stream)
        except _lib.DpwaError as e:
            assert e.code == _lib.ERR_ARG and "not attached" in str(e), str(e)
        else:
            raise AssertionError("%s: a fetch of the refused peer was accepted" % why)
        lr.close()

    refused(learner(spec=ref.REFUSED_LAYOUTS[rank]), "layout")
    refused(learner(dtype=ref.REFUSED_DTYPES[rank]), "peer holds")

    # the control pair
    spec = ref.REFUSED_LAYOUTS[0]
    lr = learner(spec=spec)
    mine, theirs = ref.control_payload(rank), ref.control_payload(1 - rank)
    flat = torch.from_numpy(np.array(mine)).to(dev)
    lr.ipc_handle()                      # exported before it publishes, as a group's learner is
    lr.publish(flat, 1.0 + rank, stream)
    torch.cuda.synchronize()
    error, _ = _exchange(shared, rank, lr)          # (its second barrier: both have published)
    assert error is None, str(error)
    lr.fetch(0, 1, False, stream)
    lr.average(flat, 1.0 + rank, stream)
    torch.cuda.synchronize()
    bad = mixed_ref.same(spec, flat.cpu().numpy(), mixed_ref.lerp(spec, mine, theirs, ref.CONTROL_FACTOR))
    assert bad is None, "the control pair's average: %s" % bad
    shared.wait()                        # the other rank has read this rank's slot
    lr.close()
    return 3


def refusals_main(rank, world, shared, vmm):
    relay_worker.rank_main(rank, world, shared, vmm, run=run_refusals)
