"""Float16 and mixed-dtype (segmented) models through the multi-process groups: DpwaConnection under the
lock-step DistGroup (IPC-mapped and fd-shared slots; copy, kernel, relay and relay-avg pulls walked in one
connection; resident parameters) and the free-running AsyncDistGroup (write-through snapshots), and the
dtype and layout checks of a handle exported by one process and attached in another.

Every rank is a process of its own on GPU 0 over gloo (tests/group_dtypes_worker.py), four at the most.
The cases, inputs and expected values are tests/group_ref.py's: every round's parameters bit-equal to
oracle.gossip.simulate with the host references of each dtype (no tolerance and no exempt element:
tests/test_group_dtypes_host.py shows that no expected value is a NaN or an inf), clocks and peers exact;
the board's averages against the exact snapshot version read.  The host test also shows that these rounds
tell every wrong implementation of group_ref.MUTANTS from the reference.

A job runs under a time limit.  One that ends by a signal, an abort or the limit stops the module: the
tests after it fail unstarted.
"""
import multiprocessing
import queue
import socket
import time

import numpy as np
import pytest

from oracle.async_check import AsyncRuns
from tests import dist_worker
from tests import group_dtypes_worker as worker
from tests import group_ref as ref
from tests import relay_worker

pytestmark = pytest.mark.gpu

JOB_S = 150.0                            # a cap against a hang, not an expectation
ABNORMAL = (134, 139, 124, 137)          # abort, segmentation fault, a time limit's two codes

_stopped = []      # the job that ended abnormally: nothing more is started on the GPU after it


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_job(name, world, target, args):
    """Spawns the ranks, collects their reports under JOB_S and returns {rank: (verdict, detail)}."""
    if _stopped:
        pytest.fail("not started: job %r ended abnormally" % _stopped[0])
    ctx = multiprocessing.get_context("spawn")
    shared = relay_worker.Shared(ctx, world)
    procs = [ctx.Process(target=target, args=(r, world, shared, args)) for r in range(world)]
    began = time.monotonic()
    for p in procs:
        p.start()
    reports, overrun = {}, []
    try:
        while len(reports) < world and time.monotonic() - began < JOB_S:
            try:
                rank, verdict, detail = shared.reports.get(timeout=0.5)
            except queue.Empty:
                if not any(p.is_alive() for p in procs) and shared.reports.empty():
                    break
                continue
            reports[rank] = (verdict, detail)
        for p in procs:
            p.join(max(0.1, min(relay_worker.BARRIER_S + 10.0, JOB_S - (time.monotonic() - began))))
    finally:
        for r, p in enumerate(procs):
            if p.is_alive():
                overrun.append(r)
                p.terminate()
                p.join(10.0)
                if p.is_alive():
                    p.kill()
                    p.join(10.0)
    print("%s: %.1f s, exit codes %r" % (name, time.monotonic() - began, [p.exitcode for p in procs]))
    codes = [p.exitcode for p in procs]
    if overrun or any(code is None or code < 0 or code in ABNORMAL for code in codes):
        _stopped.append(name)
        pytest.fail("%s: ended abnormally (exit codes %r, ranks stopped at the time limit %r); the module stops "
                    "here\n%r" % (name, codes, overrun, reports))
    for r, p in enumerate(procs):
        reports.setdefault(r, ("failed", "no report; exit code %r" % (p.exitcode,)))
    failed = sorted(r for r, (verdict, _) in reports.items() if verdict == "failed")
    assert not failed, "%s: rank %d: %s" % (name, failed[0], reports[failed[0]][1])
    return reports


def lockstep(tmp_path, job, kind, world):
    c = ref.case(job, kind, world)
    T = ref.rounds(c)
    cfg = str(tmp_path / "group.yaml")
    dist_worker.write_cfg(cfg, ref.names(c), c.fp, c.interp, c.thr)
    reports = run_job("%s-%s-%d" % (job, kind, world), world, worker.lockstep_main,
                      (job, kind, free_port(), cfg, str(tmp_path)))
    assert reports == {r: ("ok", T) for r in range(world)}, reports
    exp = ref.reference(c)
    for g in range(world):
        got = np.load(tmp_path / ("rank%d.npz" % g))
        assert list(got["peers"]) == [exp["peers"][r][g] for r in range(T)], g
        assert np.array_equal(got["clocks"], exp["clocks"][:, g]), (g, got["clocks"], exp["clocks"][:, g])
        assert got["params"].dtype == exp["params"].dtype and got["params"].shape == exp["params"][:, g].shape
        for r in range(T):
            bad = ref.same(kind, got["params"][r], exp["params"][r, g])
            assert bad is None, "rank %d, round %d (%s, peer %s): %s" % (g, r, ref.pull_at(c, r)[0],
                                                                         exp["peers"][r][g] or "-", bad)


@pytest.mark.parametrize("kind,world", [("f16", 2), ("f16", 3), ("mixed", 3), ("mixed", 4)])
def test_phase_walk_matches_simulate(tmp_path, kind, world):
    """copy, kernel:64, relay:8 (and for float16 relay-avg:8), four rounds each in one connection created
    with pull="relay:8" and switched by set_pull on every rank before the same round; fetch_probability
    0.8; even rounds fused, odd rounds update_wait then average.  The mixed ranks also find
    set_pull("relay-avg:8") refused at every switch, and the rounds after it still match."""
    lockstep(tmp_path, "walk", kind, world)


@pytest.mark.parametrize("kind", ["f16", "mixed"])
def test_resident_matches_simulate(tmp_path, kind):
    """Resident parameters (make_resident, the step after update_wait) at world 3, eight rounds: float16
    through the relay's fused average, the segmented uint8 buffer through the gathered relay; rounds
    without a fetch relocate."""
    lockstep(tmp_path, "resident", kind, 3)


def test_mixed_over_fd_shared_slots(tmp_path, monkeypatch):
    """DPWA_VMM=1: the slots and relay buffers of a segmented payload shared as fds; copy and relay:8."""
    monkeypatch.setenv("DPWA_VMM", "1")
    lockstep(tmp_path, "vmm", "mixed", 3)


@pytest.mark.parametrize("kind,world", [("f16", 3), ("mixed", 2)])
def test_board_write_through(tmp_path, kind, world):
    """The gossip board, update_send(reuse_snapshot=True) then update_wait_average(write_through=True), 16
    rounds: every average is the host references' lerp of this round's base with exactly the version of
    the peer's snapshot that was read (rebuilt from the publisher's own recorded results); clocks exact."""
    c = ref.case("board", kind, world)
    T, names = ref.rounds(c), ref.names(c)
    cfg = str(tmp_path / "board.yaml")
    dist_worker.write_cfg(cfg, names, c.fp, c.interp, c.thr)
    reports = run_job("board-%s-%d" % (kind, world), world, worker.board_main, (kind, free_port(), cfg, str(tmp_path)))
    assert reports == {r: ("ok", T) for r in range(world)}, reports
    runs = {g: np.load(tmp_path / ("rank%d.npz" % g)) for g in range(world)}
    base = ref.base(kind)
    n = runs[0]["params"].shape[1]

    def published(q, v, n_):
        return base(q, -1, n_) if v == 1 else runs[q]["params"][v - 2]

    check = AsyncRuns(names, {g: runs[g]["peers"] for g in range(world)}, {g: runs[g]["versions"] for g in range(world)},
                      c.interp, ref.VALUE, c.thr, published=published, base=base, lerp=ref.lerp(kind))
    for g in range(world):
        bad = check.check_rank(g, runs[g]["params"], runs[g]["clocks"], n)
        assert not bad, (g, bad[:5])
        # the ranks meet once after round 0: every peer has published by then, and fetch_probability is 1
        assert all(p != "" for p in runs[g]["peers"][1:]), (g, list(runs[g]["peers"]))
        for r in range(T):               # the same once more under this payload's own comparison rule
            want = check.expected_params(g, r, n)
            assert ref.finite(kind, want), (g, r)
            bad = ref.same(kind, runs[g]["params"][r], want)
            assert bad is None, "rank %d, round %d (peer %s): %s" % (g, r, runs[g]["peers"][r] or "-", bad)


@pytest.mark.parametrize("how", ["ipc", "fds"])
def test_unlike_learners_refuse_each_others_handle(monkeypatch, how):
    """Two processes, learner level, no process group: layouts of equal bytes and other digests, then float16
    against bfloat16 at equal n -- each rank's attach of the other's exported handle is DPWA_ERR_ARG
    naming the layout or what the peer holds, and a fetch of that peer says "not attached"; a control pair
    of equal layouts attaches, fetches and averages to mixed_ref.lerp.  Once over hipIpc handles, once
    (fresh processes: the variable is read at allocation) over fd-shared slots."""
    if how == "fds":
        monkeypatch.setenv("DPWA_VMM", "1")
    reports = run_job("refusals-%s" % how, 2, worker.refusals_main, how == "fds")
    assert reports == {0: ("ok", 3), 1: ("ok", 3)}, reports
