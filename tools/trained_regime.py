#!/usr/bin/env python3
"""The averaging kernel's cache policy in the trained regime: the parameters warm from a writer, the
peer's snapshot cold, a reader afterwards.  That is what the reference order (update_send -> step ->
update_wait) gives a model small enough for the Infinity Cache: the optimizer writes every parameter
just before the average reads it, and the forward pass reads every parameter just after the average
wrote it.  bench.py measures neither neighbour (its loop is averages back to back, its cold legs have
nobody touch the parameters at all).

One learner in the write-through form at configs[1]'s size (11,173,962 float32).  Per round:
  writer   flat.add_(g): every parameter rewritten
  average  dpwa_average with the next snapshot written through (the product's kernel), timed by the
           events the ABI records around the dispatch itself
  reader   flat.sum(): every parameter consumed
over learner sets (parameters and two snapshot slots) rotated so that at least three cache sizes of
other bytes pass between two uses of a set: the snapshot is read from HBM, as in bench.py's
value_cold.  The two slots of a set trade places every round, as a learner's do.

Every (policy, repeat) is a fresh child process with DPWA_LERP_POLICY set, the policies taking turns;
--rounds timed rounds after --warmup.  Prints one JSON line per child and a summary: the average's
median and p10-p90 and the wall time of writer + average + reader per round.

    python tools/trained_regime.py [--policies 8,0,1] [--repeats 3] [--rounds 300] [--warmup 10] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CACHE = 256 << 20
NUMEL = 11_173_962


def stats(us):
    srt = sorted(us)
    return {"median_us": round(statistics.median(us), 3), "p10_us": round(srt[len(srt) // 10], 3),
            "p90_us": round(srt[(9 * len(srt)) // 10], 3), "min_us": round(srt[0], 3), "max_us": round(srt[-1], 3)}


def child(args):
    import torch

    from dpwa_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("trained_regime.py needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    n = args.numel
    hdr = _lib.SLOT_PAYLOAD_OFFSET // 4
    n_sets = -(-3 * CACHE // (3 * 4 * n)) + 1

    class LearnerSet:
        def __init__(self):
            self.flat = torch.empty(n, device=dev).normal_()
            self.slots = [torch.zeros(hdr + n, device=dev), torch.zeros(hdr + n, device=dev)]
            self.slots[0][hdr:].normal_()

    sets = [LearnerSet() for _ in range(n_sets)]
    g = torch.empty(n, device=dev).normal_().mul_(1e-3)
    sink = torch.zeros((), device=dev)
    clock = torch.zeros(2, device=dev, dtype=torch.float64)
    coef = torch.zeros(4, device=dev, dtype=torch.float64)
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    s = _lib.stream_handle(None)
    total = args.warmup + args.rounds
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(total)]
    for a, b in ev:   # create them (the dispatch then records into them)
        a.record()
        b.record()

    def one_round(i):
        b = sets[i % n_sets]
        b.flat.add_(g)                                       # the writer
        peer, nxt = b.slots
        rc = lib.dpwa_average(_lib.F32, b.flat.data_ptr(), peer.data_ptr(), n, ctypes.byref(cfg), clock.data_ptr(),
                              1.0, coef.data_ptr(), nxt[hdr:].data_ptr(), s, ev[i][0].cuda_event, ev[i][1].cuda_event)
        if rc:
            raise _lib.DpwaError("dpwa_average", rc, lib.dpwa_last_error().decode())
        b.slots.reverse()
        sink.add_(b.flat.sum())                              # the reader

    torch.cuda.synchronize()
    for i in range(args.warmup):
        one_round(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.warmup, total):
        one_round(i)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    us = [1e3 * a.elapsed_time(b) for a, b in ev[args.warmup:]]
    row = {"policy": os.environ.get("DPWA_LERP_POLICY"), "repeat": args.child, "numel": n, "sets": n_sets,
           "rounds": args.rounds, "average": stats(us), "round_wall_us": round(1e6 * (t2 - t0) / args.rounds, 3),
           "round_issue_us": round(1e6 * (t1 - t0) / args.rounds, 3), "sink": float(sink)}
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", default="8,0,1")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--numel", type=int, default=NUMEL)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    policies = args.policies.split(",")
    rows = []
    for rep in range(args.repeats):
        for k in range(len(policies)):   # the policies take turns, a different one first in every repeat
            pol = policies[(k + rep) % len(policies)]
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(rep), "--rounds", str(args.rounds),
                   "--warmup", str(args.warmup), "--numel", str(args.numel)]
            out = subprocess.run(cmd, env=dict(os.environ, DPWA_LERP_POLICY=pol), cwd=ROOT, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True, timeout=300)
            if out.returncode != 0:
                print(json.dumps({"policy": pol, "repeat": rep, "error": out.stderr[-800:]}), flush=True)
                return 1
            row = json.loads(out.stdout.strip().splitlines()[-1])
            rows.append(row)
            print(json.dumps(row), flush=True)
    summary = {}
    for pol in policies:
        mine = [r for r in rows if r["policy"] == pol]
        summary[pol] = {"average_median_us": [r["average"]["median_us"] for r in mine],
                        "average_p10_p90_us": [[r["average"]["p10_us"], r["average"]["p90_us"]] for r in mine],
                        "round_wall_us": [r["round_wall_us"] for r in mine],
                        "average_median_of_medians_us": statistics.median(r["average"]["median_us"] for r in mine),
                        "round_wall_median_us": statistics.median(r["round_wall_us"] for r in mine)}
    print(json.dumps({"summary": summary}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"what": "writer (flat.add_) + write-through average + reader (flat.sum) per round over rotated "
                               "learner sets, DPWA_LERP_POLICY forced per child process",
                       "rows": rows, "summary": summary}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
