"""The relay's stripe kernels -- k_relay_phase1, k_relay_phase2 (relay_copy, stripe_len), k_lerp_relay
with StripeSrc and launch_average_relay -- and the learner code that feeds them (the stripe size of
dpwa_learner_relay_enable, relay_args' slot parity, the deferred phase 2 and relay_materialize) at
the stripe edges and copy16 edge sizes of tests/relay_ref.py, against its host model, byte for byte.

The relay needs IPC-attached peers, so each test spawns one process per rank (tests/relay_worker.py)
on GPU 0; the ranks loop over the sizes, the three dtypes and the five forms (gathered, fused plain,
fused write-through, fused resident, fused then copied out) with the picks of relay_ref.PICKS, hard
operands (forms_ref.operands) and loss interpolation, and every rank checks what it observes against
the model.  tests/test_relay_host.py shows without a GPU that these cases tell the model from every
wrong kernel of relay_ref.RELAY_MUTANTS.

A rank that finds a mismatch reports it and stops all ranks; the parent shows the first report."""
import multiprocessing
import queue

import pytest

from tests import relay_ref as ref
from tests import relay_worker

pytestmark = pytest.mark.gpu

JOIN_S = 300.0


def run_world(world, target=relay_worker.rank_main, only=None):
    """Spawns the ranks, waits (with a limit) and returns their reports: {rank: (verdict, detail)}."""
    ctx = multiprocessing.get_context("spawn")
    shared = relay_worker.Shared(ctx, world)
    procs = [ctx.Process(target=target, args=(r, world, shared, only)) for r in range(world)]
    for p in procs:
        p.start()
    reports = {}
    try:
        for _ in range(world):
            try:
                rank, verdict, detail = shared.reports.get(timeout=JOIN_S)
            except queue.Empty:
                break
            reports[rank] = (verdict, detail)
        for p in procs:
            p.join(relay_worker.BARRIER_S + 10.0)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(10.0)
    for r, p in enumerate(procs):
        reports.setdefault(r, ("failed", "no report; exit code %r" % (p.exitcode,)))
    return reports


def first_failure(reports):
    """The report to show: the first rank that found something itself, not one stopped by another's."""
    failed = sorted(r for r, (verdict, _) in reports.items() if verdict == "failed")
    return None if not failed else "rank %d: %s" % (failed[0], reports[failed[0]][1])


@pytest.mark.parametrize("world", ref.WORLDS)
def test_relay_matches_the_host_model(world):
    """Every size of relay_ref.sizes(world) (the stripe edges; the last stripe at copy16's four-deep
    and remainder boundaries for one and two workgroups per stripe), float32, bfloat16 and float16,
    every form, three or four rounds of dictated picks: each rank's staged bytes, averaged bits,
    bands, clock, coefficients and snapshots are the model's."""
    reports = run_world(world)
    assert first_failure(reports) is None, first_failure(reports)
    rounds = len(ref.cases(world)) * len(ref.FORMS) * len(ref.PICKS[world])
    assert reports == {r: ("ok", rounds) for r in range(world)}, reports
