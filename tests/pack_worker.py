"""One rank of tests/test_gpu_pack.py's lock-step job: two ranks on GPU 0 under DistGroup (torch.distributed
over gloo), one connection created with pull="packed" and switched with set_pull before every round.  The
ranks record every round's parameters, clock and peer and leave the comparing to the parent, as
tests/group_dtypes_worker.py does; processes start and end through tests/relay_worker.rank_main.

Before the job each rank also finds a fetch from a peer whose packed images it never attached refused."""
import os

import numpy as np

from tests import relay_worker
from tests.group_dtypes_worker import _init_group, to_device, to_host
from tests.relay_worker import HANDLE

NAMES = ["w1", "w2"]
SEEDS = [31, 32]
PULLS = ["copy", "packed", "packed:2", "copy"]       # the round's pull
SEND = [[1.0, 0.9], [0.8, 0.7], [0.6, 0.5], [0.4, 0.3]]
WAIT = [[0.95, 0.85], [0.75, 0.65], [0.55, 0.45], [0.35, 0.25]]
SIZES = {"f16": 10243, "f32": 2049}


def inputs(dtype):
    """(init, deltas): float32 values, or float16 bit patterns (uint16)."""
    n, T = SIZES[dtype], len(PULLS)
    rng = np.random.default_rng(n)
    init = rng.standard_normal((2, n)).astype(np.float32)
    deltas = (0.01 * rng.standard_normal((T, 2, n))).astype(np.float32)
    if dtype == "f16":
        return init.astype(np.float16).view(np.uint16), deltas.astype(np.float16).view(np.uint16)
    return init, deltas


def unattached_peer_is_refused(shared, rank, dev):
    """Two bare learners that map each other's slots but not each other's images: DPWA_PULL_PACKED is
    accepted, and the fetch is DPWA_ERR_STATE by name, with nothing queued."""
    import torch
    from dpwa_amd import _lib
    from dpwa_amd.learner import Learner
    lr = Learner(dev, 1024, torch.float32, _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0))
    shared.put(rank, 0, lr.ipc_handle())
    shared.wait()
    lr.attach_ipc(1 - rank, shared.get(1 - rank, 0, HANDLE))
    _lib.call("dpwa_learner_pack_enable", lr.handle)
    _lib.call("dpwa_learner_set_pull", lr.handle, _lib.PULL_PACKED, 8)
    flat = torch.zeros(1024, device=dev)
    lr.publish(flat, 1.0, torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    shared.wait()
    try:
        lr.fetch(1 - rank, 1, False, torch.cuda.current_stream(dev))
    except _lib.DpwaError as e:
        assert e.code == _lib.ERR_STATE and "packed images are not attached" in str(e), str(e)
    else:
        raise AssertionError("a fetch from a peer without attached images was accepted")
    torch.cuda.synchronize()
    shared.wait()                       # nobody maps this rank's slots any more once both have closed
    lr.close()
    shared.wait()


def run_walk(shared, rank, world, args):
    dtype, port, cfg_path, out_dir = args
    import torch
    dist, dev = _init_group(rank, world, port)
    from dpwa_amd import DpwaConnection
    from dpwa_amd.group import DistGroup
    if os.environ.get("DPWA_VMM") != "1":      # (its bare learners exchange hipIpc handles)
        unattached_peer_is_refused(shared, rank, dev)
    init, deltas = inputs(dtype)
    from dpwa_amd.dpwa import GROUP_PACKED, RELAY_PACKED
    try:                                # free-running ranks: refused at construction, before any collective
        DpwaConnection(NAMES[rank], cfg_path, seed=SEEDS[rank], pull="packed", group="async")
    except ValueError as e:
        assert str(e) == GROUP_PACKED, str(e)
    else:
        raise AssertionError("an AsyncDistGroup connection accepted pull='packed'")
    conn = DpwaConnection(NAMES[rank], cfg_path, seed=SEEDS[rank], pull="packed", group="lockstep")
    assert type(conn._group) is DistGroup

    def relay_is_refused(when):
        try:
            conn.set_pull("relay:8")
        except ValueError as e:
            assert str(e) == RELAY_PACKED and conn._pull.startswith(("packed", "copy")), (when, str(e))
        else:
            raise AssertionError("a packed-created connection accepted set_pull('relay:8') " + when)

    relay_is_refused("before the bind")
    flat = to_device(dtype, init[rank], dev)
    T = len(PULLS)
    params, clocks, peers = np.zeros((T,) + init.shape[1:], init.dtype), np.zeros(T), []
    for r in range(T):
        conn.set_pull(PULLS[r])
        conn.update_send(flat, SEND[r][rank])
        flat.add_(to_device(dtype, deltas[r, rank], dev))
        payload, _ = conn.update_wait_average(flat, WAIT[r][rank])
        params[r] = to_host(dtype, flat)
        clocks[r] = conn.clock
        peers.append(payload.peer if payload is not None else "")
        if r == 0:                      # the images are shared the way the job says
            fds, _ = conn._learner.export_fds(2)
            for fd in fds:
                os.close(fd)
            assert bool(fds) == (os.environ.get("DPWA_VMM") == "1"), len(fds)
    relay_is_refused("after the bind")
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), params=params, clocks=clocks, peers=np.array(peers))
    torch.cuda.synchronize()
    dist.barrier()
    conn.close()
    dist.destroy_process_group()
    return T


def walk_main(rank, world, shared, args):
    relay_worker.rank_main(rank, world, shared, args, run=run_walk)
