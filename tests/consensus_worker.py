"""One rank of a job of tests/test_gpu_consensus.py: ``DpwaConnection.consensus`` under the lock-step
DistGroup (torch.distributed over gloo, every rank on GPU 0), or the refusals of the groups that have no
consensus.  A lock-step rank records, for every round, the snapshot it published, the mean it got and the
sums, and leaves the comparing to the parent.  Processes start and end through
tests/relay_worker.rank_main, as tests/group_dtypes_worker.py's do."""
import os

import numpy as np

from tests import relay_worker
from tests.group_dtypes_worker import _init_group

N = 10_243
ROUNDS = 4


def run_lockstep(shared, rank, world, args):
    pull, port, cfg_path, out_dir, vmm = args
    import torch
    dist, dev = _init_group(rank, world, port)
    from dpwa_amd import DpwaConnection
    from dpwa_amd.group import DistGroup
    names = ["w%d" % (g + 1) for g in range(world)]
    conn = DpwaConnection(names[rank], cfg_path, seed=30 + rank, pull=pull, group="lockstep")
    assert type(conn._group) is DistGroup
    rng = np.random.default_rng(40 + rank)
    flat = torch.from_numpy(rng.standard_normal(N).astype(np.float16)).to(dev)
    snaps, means, sums = np.zeros((ROUNDS, N), np.uint16), np.zeros((ROUNDS, N), np.uint16), np.zeros((ROUNDS, 10))
    for r in range(ROUNDS):
        snaps[r] = flat.view(torch.int16).cpu().numpy().view(np.uint16)
        conn.update_send(flat, 1.0)
        c = conn.consensus()
        assert c.members == names and c.version == r + 1, (c.members, c.version)
        means[r] = c.tensor().view(torch.int16).cpu().numpy().view(np.uint16)
        rec = c.read()
        sums[r] = [rec.norm2, rec.spread2] + list(rec.member_spread2)
        flat.add_(torch.from_numpy((0.01 * rng.standard_normal(N)).astype(np.float16)).to(dev))
        conn.update_wait_average(flat, 1.0)
        if r == 0:                       # the slots are shared the way the job says
            fds, _ = conn._learner.export_fds(0)
            for fd in fds:
                os.close(fd)
            assert bool(fds) == bool(vmm), (vmm, len(fds))
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), snaps=snaps, means=means, sums=sums)
    torch.cuda.synchronize()
    dist.barrier()
    conn.close()
    dist.destroy_process_group()
    return ROUNDS


def lockstep_main(rank, world, shared, args):
    relay_worker.rank_main(rank, world, shared, args, run=run_lockstep)


def run_refusals(shared, rank, world, args):
    """Free-running ranks, the relay's fused average and the wire transport refuse by name, before anything is
    launched.  Then a round of a relay-avg connection: with its fused second phase pending the learner entry
    itself is DPWA_ERR_STATE and stores nothing."""
    port, cfg_path = args
    import ctypes

    import torch
    dist, dev = _init_group(rank, world, port)
    from dpwa_amd import DpwaConnection, _lib
    from dpwa_amd.bridge import WireConnection
    from dpwa_amd.consensus import RELAY_AVG
    from dpwa_amd.group import AsyncDistGroup
    name = "w%d" % (rank + 1)
    seen = 0
    for make, word in ((lambda: DpwaConnection(name, cfg_path, seed=1, group="async"), "lock-step"),
                       (lambda: DpwaConnection(name, cfg_path, seed=1, group="lockstep", pull="relay-avg:8"), "relay-avg"),
                       (lambda: WireConnection(name, cfg_path, seed=1, serve=False), "wire")):
        conn = make()
        if word == "lock-step":
            assert type(conn._group) is AsyncDistGroup
        try:
            conn.consensus()
        except ValueError as e:
            assert word in str(e), (word, str(e))
            seen += 1
        finally:
            conn.close()
    conn = DpwaConnection(name, cfg_path, seed=5 + rank, group="lockstep", pull="relay-avg:8")
    flat = torch.from_numpy(np.random.default_rng(rank).standard_normal(N).astype(np.float16)).to(dev)
    conn.update_send(flat, 1.0)                  # fetch_probability 1: the fused second phase is pending now
    assert conn.fetching
    try:
        conn.consensus()
    except ValueError as e:
        assert str(e) == RELAY_AVG, str(e)
    else:
        raise AssertionError("a relay-avg connection gave a consensus")
    lib = _lib.load()
    out = torch.zeros(N, dtype=torch.float16, device=dev)
    ids = (ctypes.c_int32 * 1)(-1)
    rc = lib.dpwa_learner_consensus(conn._learner.handle, ids, 1, 1, ctypes.c_void_p(out.data_ptr()), None,
                                    _lib.stream_handle(None))
    assert rc == _lib.ERR_STATE and b"fused relay phase" in lib.dpwa_last_error(), (rc, lib.dpwa_last_error())
    conn.update_wait_average(flat, 1.0)
    torch.cuda.synchronize()
    assert not bool(out.any())
    dist.barrier()
    conn.close()
    dist.destroy_process_group()
    return seen


def refusals_main(rank, world, shared, args):
    relay_worker.rank_main(rank, world, shared, args, run=run_refusals)
