"""What the consensus pass costs: dpwa_consensus over G = 2 members in its three forms -- full (mean and
sums), mean only, measure only -- against dpwa_stream_mix(nr=2, nw=1), the same bytes with no arithmetic,
on the same buffers, interleaved launch by launch in one process, each launch timed by the events the ABI
records around the dispatch itself (hipExtLaunchKernelGGL).  The measure-only form stores nothing, so the
mix moves n*s more bytes than it does; the other two move the mix's bytes.

Per size (11,173,962 float32 and 2^26 bfloat16), three repeats of --launches launches of each after --warmup:
  warm   one buffer set, launches back to back
  cold   buffer sets rotated so that at least three Infinity Cache sizes of other bytes pass between two
         uses of a set
Also G = 8 at the float32 size (no baseline: dpwa_stream_mix takes two sources) and the finishing kernel
alone (a call with n = 0 launches nothing else; timed by an event pair around the launch, so it includes
the dispatch gaps the other figures do not).

    python tools/consensus_cost.py [--launches K] [--warmup W] [--repeats R] [--out FILE]
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
from tools.distance_cost import CACHE, SIZES, events, stats  # noqa: E402

FORMS = ("mix", "full", "mean_only", "measure_only")


class BufferSet:
    def __init__(self, n, tdtype, dev, members):
        host = torch.float32 if torch.empty((), dtype=tdtype).element_size() == 4 else torch.float16
        self.src = [torch.empty(n, device=dev, dtype=host).normal_() for _ in range(members)]
        self.out = torch.empty(n, device=dev, dtype=host)
        self.srcs = (ctypes.c_void_p * members)(*[t.data_ptr() for t in self.src])
        self.dst = (ctypes.c_void_p * 1)(self.out.data_ptr())


def launch(lib, form, code, b, members, n, nbytes, work, rec, s, a0, a1):
    if form == "mix":
        rc = lib.dpwa_stream_mix(b.dst, 1, b.srcs, 2, nbytes, s, a0.cuda_event, a1.cuda_event)
    else:
        out = None if form == "measure_only" else b.out.data_ptr()
        w, r = (None, None) if form == "mean_only" else (work.data_ptr(), rec.data_ptr())
        rc = lib.dpwa_consensus(code, b.srcs, members, n, out, w, r, s, a0.cuda_event, a1.cuda_event)
    if rc:
        raise _lib.DpwaError(form, rc, lib.dpwa_last_error().decode())


def compare(lib, code, tdtype, n, members, forms, n_sets, launches, warmup, dev, work, rec):
    """One repeat: `launches` timed launches of each form, interleaved, over `n_sets` rotated sets."""
    sets = [BufferSet(n, tdtype, dev, members) for _ in range(n_sets)]
    nbytes = n * sets[0].out.element_size() // 16 * 16
    s = _lib.stream_handle(None)
    total = warmup + launches
    ev = {f: events(total) for f in forms}
    torch.cuda.synchronize()
    j = 0
    for i in range(total):
        k = i % len(forms)
        for form in forms[k:] + forms[:k]:          # no form always follows the same other one
            b = sets[j % n_sets]
            j += 1
            launch(lib, form, code, b, members, n, nbytes, work, rec, s, *ev[form][i])
    torch.cuda.synchronize()
    return {f: [1e3 * a.elapsed_time(b) for a, b in pairs[warmup:]] for f, pairs in ev.items()}


def finish_times(lib, launches, warmup, dev, work, rec):
    b = BufferSet(64, torch.float32, dev, 2)
    s = _lib.stream_handle(None)
    ev = events(warmup + launches)
    torch.cuda.synchronize()
    for a0, a1 in ev:
        a0.record()
        rc = lib.dpwa_consensus(_lib.F32, b.srcs, 2, 0, None, work.data_ptr(), rec.data_ptr(), s, None, None)
        a1.record()
        if rc:
            raise _lib.DpwaError("dpwa_consensus", rc, lib.dpwa_last_error().decode())
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in ev[warmup:]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="consensus_cost.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("consensus_cost.py needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    nbytes = ctypes.c_int64()
    _lib.call("dpwa_consensus_workspace", ctypes.byref(nbytes))
    work = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
    rec = torch.zeros(128, dtype=torch.uint8, device=dev)
    out = {"what": "dpwa_consensus (G = 2: full, mean only, measure only) against dpwa_stream_mix(nr=2, nw=1) on the "
                   "same buffers, interleaved launch by launch; dispatch begin/end events",
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "launches": args.launches,
           "repeats": args.repeats, "sizes": {}}
    for name, code, tdtype, n in SIZES:
        esize = torch.empty((), dtype=tdtype).element_size()
        set_bytes = 3 * esize * n
        cold_sets = -(-3 * CACHE // set_bytes) + 1
        entry = {"numel": n, "bytes_per_launch": 3 * esize * n, "cold_sets": cold_sets}
        for mode, n_sets in (("warm", 1), ("cold", cold_sets)):
            reps = []
            for _ in range(args.repeats):
                us = compare(lib, code, tdtype, n, 2, FORMS, n_sets, args.launches, args.warmup, dev, work, rec)
                r = {k: stats(v) for k, v in us.items()}
                for f in FORMS[1:]:
                    r[f + "_over_mix_median"] = round(r[f]["median_us"] / r["mix"]["median_us"], 4)
                reps.append(r)
                torch.cuda.empty_cache()
            entry[mode] = {"repeats": reps}
            for f in FORMS[1:]:
                entry[mode][f + "_over_mix_median"] = statistics.median(r[f + "_over_mix_median"] for r in reps)
        out["sizes"][name] = entry
    name, code, tdtype, n = SIZES[0]
    out["g8_f32"] = {"numel": n, "bytes_per_launch": 9 * 4 * n}
    for mode, n_sets in (("warm", 1), ("cold", -(-3 * CACHE // (9 * 4 * n)) + 1)):
        out["g8_f32"][mode] = [{k: stats(v) for k, v in compare(lib, code, tdtype, n, 8, ("full",), n_sets, args.launches,
                                                                  args.warmup, dev, work, rec).items()}
                               for _ in range(args.repeats)]
        torch.cuda.empty_cache()
    out["finish_event_pair"] = [stats(finish_times(lib, args.launches, args.warmup, dev, work, rec))
                                for _ in range(args.repeats)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    brief = {nm: {mode: {f: e[mode][f + "_over_mix_median"] for f in FORMS[1:]} for mode in ("warm", "cold")}
             for nm, e in out["sizes"].items()}
    print(json.dumps({"over_mix_median": brief,
                      "mix_median_us": {nm: {m: [r["mix"]["median_us"] for r in e[m]["repeats"]] for m in ("warm", "cold")}
                                        for nm, e in out["sizes"].items()},
                      "g8_f32_median_us": {m: [r["full"]["median_us"] for r in out["g8_f32"][m]] for m in ("warm", "cold")},
                      "finish_median_us": [r["median_us"] for r in out["finish_event_pair"]]}))


if __name__ == "__main__":
    main()
