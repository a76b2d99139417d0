"""One rank of tests/test_gpu_pack_sr.py's lock-step job: tests/pack_worker.py's two ranks in one 'packed-avg' round,
rank 0 alone publishing stochastically rounded images.  The comparing is the parent's."""
import os

import numpy as np

from tests import relay_worker
from tests.group_dtypes_worker import _init_group, to_device, to_host
from tests.pack_worker import NAMES, SEEDS, SIZES

SEND, WAIT = [[1.0, 0.9]], [[0.95, 0.85]]


def inputs():
    rng = np.random.default_rng(SIZES["f32"] + 1)
    return (rng.standard_normal((2, SIZES["f32"])).astype(np.float32),
            (0.01 * rng.standard_normal((1, 2, SIZES["f32"]))).astype(np.float32))


def run_round(shared, rank, world, args):
    port, cfg_path, out_dir = args
    import torch
    dist, dev = _init_group(rank, world, port)
    from dpwa_amd import DpwaConnection
    for bad in ({"pull": "packed-avg", "pack_rounding": "up"}, {"pull": "copy", "pack_rounding": "stochastic"},
                {"pack_rounding": "stochastic"}):     # refused at construction, before any collective
        try:
            DpwaConnection(NAMES[rank], cfg_path, seed=SEEDS[rank], group="lockstep", **bad)
        except ValueError as e:
            assert "pack_rounding" in str(e), str(e)
        else:
            raise AssertionError("accepted %r" % (bad,))
    init, deltas = inputs()
    conn = DpwaConnection(NAMES[rank], cfg_path, seed=SEEDS[rank], pull="packed-avg", group="lockstep",
                          pack_rounding="stochastic" if rank == 0 else "nearest")
    flat = to_device("f32", init[rank], dev)
    conn.set_pull("copy")                # set_pull keeps the rounding mode, whichever transports it walks through
    conn.set_pull("packed-avg")
    conn.update_send(flat, SEND[0][rank])
    flat.add_(to_device("f32", deltas[0, rank], dev))
    payload, _ = conn.update_wait_average(flat, WAIT[0][rank])
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), params=to_host("f32", flat), clock=conn.clock,
             peer=np.array(payload.peer if payload is not None else ""))
    torch.cuda.synchronize()
    dist.barrier()
    conn.close()
    dist.destroy_process_group()
    return 1


def round_main(rank, world, shared, args):
    relay_worker.rank_main(rank, world, shared, args, run=run_round)
