"""What healing costs: the write-through guarded average (dpwa_average_guarded) against the unguarded product
kernel (dpwa_average) of the same build on the same buffers, interleaved launch by launch in one process,
each launch timed by the events the ABI records around the dispatch itself (tools/distance_cost.py's
method).  The yardstick is the unguarded kernel's own p10-p90 in the same run.

Per size (11,173,962 float32 and 2^26 bfloat16), three repeats of --launches launches of each kernel after
--warmup, on clean inputs -- the path every round pays:
  warm   one buffer set (parameters, peer slot, next snapshot), launches back to back
  cold   buffer sets rotated so that at least three Infinity-Cache sizes of other bytes pass between two
         uses of a set: every launch reads from HBM
and one more warm run per size with 1 % of the peer's elements NaN (refused: the parameters stay finite from
launch to launch), which prices the counting and its atomics.

    python tools/heal_cost.py [--launches K] [--warmup W] [--repeats R] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dpwa_amd import _lib  # noqa: E402
from tools.distance_cost import CACHE, SIZES, BufferSet, events, stats  # noqa: E402


def compare(lib, code, tdtype, n, n_sets, launches, warmup, dev, rec, bad_share=0.0):
    """One repeat: `launches` timed launches of each kernel, interleaved, over `n_sets` rotated sets."""
    sets = [BufferSet(n, tdtype, dev) for _ in range(n_sets)]
    if bad_share:
        esize = sets[0].param.element_size()
        hdr = _lib.SLOT_PAYLOAD_OFFSET // esize
        for b in sets:      # by bit pattern: a 16-bit set's bits are read as bfloat16, whose NaN is not float16's
            bits = b.slot.view(torch.int32 if esize == 4 else torch.int16)[hdr:]
            bits[torch.rand(n, device=dev) < bad_share] = 0x7fc00000 if esize == 4 else 0x7fc0
    clock = torch.zeros(2, device=dev, dtype=torch.float64)
    coef = torch.zeros(4, device=dev, dtype=torch.float64)
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    s = _lib.stream_handle(None)
    total = warmup + launches
    ev = {"unguarded": events(total), "guarded": events(total)}
    torch.cuda.synchronize()
    j = 0
    for i in range(total):
        order = ("unguarded", "guarded") if i % 2 == 0 else ("guarded", "unguarded")   # neither always follows the other
        for name in order:
            b = sets[j % n_sets]
            j += 1
            a0, a1 = ev[name][i]
            head = (code, b.param.data_ptr(), b.slot.data_ptr(), n, ctypes.byref(cfg), clock.data_ptr(), 1.0,
                    coef.data_ptr(), b.snap.data_ptr())
            if name == "unguarded":
                rc = lib.dpwa_average(*head, s, a0.cuda_event, a1.cuda_event)
            else:
                rc = lib.dpwa_average_guarded(*head, rec.data_ptr(), s, a0.cuda_event, a1.cuda_event)
            if rc:
                raise _lib.DpwaError("dpwa_average(_guarded)", rc, lib.dpwa_last_error().decode())
    torch.cuda.synchronize()
    return {name: [1e3 * a.elapsed_time(b) for a, b in pairs[warmup:]] for name, pairs in ev.items()}


def place(g, u):
    """Where the guarded median falls relative to the unguarded kernel's own spread."""
    if g < u["p10_us"]:
        return "below p10"
    return "inside p10-p90" if g <= u["p90_us"] else "above p90"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="heal_cost.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("heal_cost.py needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    rec = torch.zeros(4, dtype=torch.int64, device=dev)
    out = {"what": "dpwa_average_guarded (write-through) against dpwa_average of the same build on the same buffers, "
                   "interleaved launch by launch; the yardstick is the unguarded kernel's p10-p90 of the same run",
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "launches": args.launches,
           "repeats": args.repeats, "sizes": {}}
    for name, code, tdtype, n in SIZES:
        esize = torch.empty((), dtype=tdtype).element_size()
        set_bytes = 3 * esize * n
        cold_sets = -(-3 * CACHE // set_bytes) + 1
        entry = {"numel": n, "bytes_per_launch": 4 * esize * n, "set_bytes": set_bytes, "cold_sets": cold_sets}
        for mode, n_sets, share, repeats in (("warm", 1, 0.0, args.repeats), ("cold", cold_sets, 0.0, args.repeats),
                                             ("warm_1pct_bad", 1, 0.01, 1)):
            reps = []
            for _ in range(repeats):
                before = rec.cpu().tolist()
                us = compare(lib, code, tdtype, n, n_sets, args.launches, args.warmup, dev, rec, share)
                r = {k: stats(v) for k, v in us.items()}
                u, g = r["unguarded"], r["guarded"]
                r["guarded_over_unguarded_median"] = round(g["median_us"] / u["median_us"], 4)
                r["guarded_median_is"] = place(g["median_us"], u)
                r["refused_per_launch"] = (rec.cpu().tolist()[1] - before[1]) / (args.warmup + args.launches)
                reps.append(r)
                torch.cuda.empty_cache()
            entry[mode] = {"repeats": reps,
                           "guarded_over_unguarded_median": statistics.median(r["guarded_over_unguarded_median"] for r in reps)}
        out["sizes"][name] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({name: {mode: (e[mode]["guarded_over_unguarded_median"], [r["guarded_median_is"] for r in e[mode]["repeats"]])
                             for mode in ("warm", "cold", "warm_1pct_bad")} for name, e in out["sizes"].items()}))


if __name__ == "__main__":
    main()
