"""One rank of a two-rank relay job for tests/test_gpu_pdist.py: the order of the relay-avg refusal
that a single learner cannot reach -- dpwa_learner_set_param_distance while a fused second phase
(dpwa_learner_relay_phase2 with fuse != 0) is pending.  The ranks are tests/relay_worker.py's
(its Learners: all on GPU 0, each other's slots and relay buffers mapped over IPC; its Shared:
barriers with a limit, the report queue), and so is the order of the round up to phase 2.

The round: publish, barrier, phase 1, barrier, phase 2 fused -- pending.  Switching the per-parameter
distance on is then DPWA_ERR_STATE naming the pending phase and changes nothing; switching it off
(count 0) is accepted.  The fused average consumes the fetch; after it switching on succeeds, and
the next fused second phase of this learner is DPWA_ERR_STATE, the other order, at a real relay.
"""
import ctypes
import os
import sys
import threading
import traceback
import types

from tests import pdist_ref, relay_worker
from tests.dist_ref import CODE


def run(shared, rank, world):
    import torch
    from dpwa_amd import _lib
    lay = pdist_ref.layout_a()
    job = types.SimpleNamespace(world=world, nbytes=lay.total_bytes, dtype="f32", n=lay.total_bytes // 4, blocks=1)
    ls = relay_worker.Learners(shared, rank, job, resident=False)
    lib, h = _lib.load(), ls.h
    arr = (_lib.ParamRange * len(lay.tensors))(*[_lib.ParamRange(off, length, CODE[d], 0)
                                                 for _, d, off, length in lay.tensors])
    count = len(lay.tensors)
    picks = [1 - r for r in range(world)]
    rec, got = ctypes.c_void_p(), ctypes.c_int64()
    for version in (1, 2):
        ls.flat.copy_(torch.full((job.nbytes,), 0x3c + rank, dtype=torch.uint8))      # finite float32 patterns
        _lib.call("dpwa_learner_publish", h, ctypes.c_void_p(ls.flat.data_ptr()), 1.0, None, ls.stream())
        torch.cuda.synchronize()
        shared.wait()
        _lib.call("dpwa_learner_relay_wait", h, ls.stream())
        ls.picks.copy_(torch.tensor(picks, dtype=torch.int32))
        _lib.call("dpwa_learner_relay_phase1", h, ctypes.c_void_p(ls.picks.data_ptr()), version, job.blocks, ls.stream())
        ls.side.synchronize()
        shared.wait()
        rc = lib.dpwa_learner_relay_phase2(h, ctypes.c_void_p(ls.picks.data_ptr()), picks[rank], version, job.blocks, 1)
        if version == 2:                 # the per-parameter distance is on: the fused phase is refused, nothing is pending
            assert rc == _lib.ERR_STATE and b"dpwa_learner_set_param_distance" in lib.dpwa_last_error(), (rc, lib.dpwa_last_error())
            _lib.call("dpwa_learner_relay_phase2", h, ctypes.c_void_p(ls.picks.data_ptr()), picks[rank], version, job.blocks, 0)
            _lib.call("dpwa_learner_average", h, ctypes.c_void_p(ls.flat.data_ptr()), 1.0, None, ls.stream())
            torch.cuda.synchronize()
            shared.wait()
            break
        assert rc == _lib.OK, (rc, lib.dpwa_last_error())
        # a fused second phase is pending
        rc = lib.dpwa_learner_set_param_distance(h, arr, count, 1)
        msg = lib.dpwa_last_error()
        assert rc == _lib.ERR_STATE and b"dpwa_learner_set_param_distance" in msg and b"pending" in msg, (rc, msg)
        assert lib.dpwa_learner_param_distance(h, ctypes.byref(rec), ctypes.byref(got)) == _lib.ERR_STATE   # nothing was allocated
        assert lib.dpwa_learner_set_param_distance(h, None, 0, 1) == _lib.OK          # off: always accepted
        _lib.call("dpwa_learner_average", h, ctypes.c_void_p(ls.flat.data_ptr()), 1.0, None, ls.stream())   # the fused average
        torch.cuda.synchronize()
        _lib.call("dpwa_learner_set_param_distance", h, arr, count, 1)                # no longer pending
        _lib.call("dpwa_learner_param_distance", h, ctypes.byref(rec), ctypes.byref(got))
        assert got.value == count
        shared.wait()
    ls.close()
    return 2


def rank_main(rank, world, shared, only=None):
    """Process entry, as tests/relay_worker.py's: a report to the parent, a last barrier, then exit."""
    status, report = 0, None
    try:
        import torch
        torch.cuda.set_device(0)
        report = ("ok", run(shared, rank, world))
    except threading.BrokenBarrierError:
        status, report = 2, ("stopped", "another rank broke the barrier, or one never arrived")
    except AssertionError as e:
        status, report = 1, ("failed", str(e))
    except BaseException:
        status, report = 1, ("failed", traceback.format_exc())
    if status:
        shared.barrier.abort()
    shared.reports.put((rank,) + report)
    shared.reports.close()
    shared.reports.join_thread()
    try:                                 # every rank's GPU work is over before any rank's memory goes
        shared.leave.wait(relay_worker.BARRIER_S)
    except threading.BrokenBarrierError:
        pass
    sys.stdout.flush()
    os._exit(status)
