"""One rank of tests/test_gpu_pack_avg.py's lock-step job: tests/pack_worker.py's two ranks, walking set_pull
through both packed modes.  The last round has rank 0 tracking the distance, so its fetch is expanded first."""
import os

import numpy as np

from tests import relay_worker
from tests.group_dtypes_worker import _init_group, to_device, to_host
from tests.pack_worker import NAMES, SEEDS, inputs

PULLS = ["copy", "packed", "packed-avg", "packed-avg:2", "packed-avg", "copy", "packed-avg"]   # the round's pull
T = len(PULLS)
SEND = [[1.0 - 0.1 * r, 0.95 - 0.1 * r] for r in range(T)]
WAIT = [[0.9 - 0.1 * r, 0.85 - 0.1 * r] for r in range(T)]


def deltas_of(dtype):
    """(init, deltas): pack_worker's, its four rounds of deltas repeated to this walk's length."""
    init, deltas = inputs(dtype)
    return init, deltas[np.arange(T) % len(deltas)]


def run_walk(shared, rank, world, args):
    dtype, resident, port, cfg_path, out_dir = args
    import torch
    dist, dev = _init_group(rank, world, port)
    from dpwa_amd import DpwaConnection, _lib
    from dpwa_amd.devview import device_tensor
    from dpwa_amd.dpwa import PeerDistance
    init, deltas = deltas_of(dtype)
    conn = DpwaConnection(NAMES[rank], cfg_path, seed=SEEDS[rank], pull="packed-avg", group="lockstep")
    flat = to_device(dtype, init[rank], dev)
    params, clocks, peers = np.zeros((T,) + init.shape[1:], init.dtype), np.zeros(T), []
    staged = np.zeros((T, init[0].nbytes), np.uint8)    # the staging payload after each round: who wrote it?
    for r in range(T):
        conn.set_pull(PULLS[r])
        if resident and r == 0:
            conn.make_resident(flat)
        if r == T - 1 and rank == 0:        # a tracking learner: the landing image is expanded for the distance pass
            _lib.call("dpwa_learner_set_distance", conn._learner.handle, 1)
        if resident:                        # the resident order: the step comes after update_wait
            conn.update_send(conn.parameters, SEND[r][rank])
            payload, _ = conn.update_wait_average(conn.parameters, WAIT[r][rank])
            params[r] = to_host(dtype, conn.parameters)
            conn.parameters.add_(to_device(dtype, deltas[r, rank], dev))
        else:
            conn.update_send(flat, SEND[r][rank])
            flat.add_(to_device(dtype, deltas[r, rank], dev))
            payload, _ = conn.update_wait_average(flat, WAIT[r][rank], write_through=r % 2 == 1)
            params[r] = to_host(dtype, flat)
        clocks[r] = conn.clock
        staged[r] = device_tensor(conn._learner.staging_payload_ptr, staged.shape[1], torch.uint8, dev).cpu().numpy()
        peers.append(payload.peer if payload is not None else "")
    rec = PeerDistance(conn._learner).read() if rank == 0 else None
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), params=params, clocks=clocks, peers=np.array(peers),
             staged=staged, dist=np.array([rec.dist2, rec.norm2] if rec else [0.0, 0.0]))
    torch.cuda.synchronize()
    dist.barrier()
    conn.close()
    dist.destroy_process_group()
    return T


def walk_main(rank, world, shared, args):
    relay_worker.rank_main(rank, world, shared, args, run=run_walk)
