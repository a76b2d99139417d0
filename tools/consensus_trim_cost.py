"""What the trimmed consensus costs: dpwa_consensus_trimmed at t = 1 and at the median against
dpwa_consensus (the mean) on the same buffers, G = 3, 5, 8, store + distance and store only, interleaved
launch by launch in one process, each launch timed by the events the ABI records around the dispatch
itself.  Buffer sets are rotated so that at least three Infinity Cache sizes of other bytes pass between
two uses of a set (the consensus of a finished run reads cold snapshots).  --parent-lib: a libdpwa_hip.so
built from the parent commit, whose dpwa_consensus takes its turns in the same rotation.

    python tools/consensus_trim_cost.py [--launches K] [--warmup W] [--parent-lib FILE] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dpwa_amd import _lib  # noqa: E402
from tools.consensus_cost import BufferSet  # noqa: E402
from tools.distance_cost import CACHE, SIZES, events, stats  # noqa: E402

GROUPS = (3, 5, 8)


def forms_of(G, parent):
    """[(name, library, trim, measured)]: the mean, t = 1 and the median (one form where they are the same)."""
    trims = [("mean", 0), ("t1", 1)] + ([("median", (G - 1) // 2)] if G > 4 else [])
    out = [("%s_%s" % (name, "full" if full else "store"), "this", t, full) for name, t in trims for full in (True, False)]
    if parent:
        out += [("parent_mean_full", "parent", 0, True), ("parent_mean_store", "parent", 0, False)]
    return out


def launch(libs, form, code, b, G, n, work, rec, s, a0, a1):
    name, which, t, full = form
    w, r = (work.data_ptr(), rec.data_ptr()) if full else (None, None)
    lib = libs[which]
    if t:
        rc = lib.dpwa_consensus_trimmed(code, b.srcs, G, t, n, b.out.data_ptr(), w, r, s, a0.cuda_event, a1.cuda_event)
    else:
        rc = lib.dpwa_consensus(code, b.srcs, G, n, b.out.data_ptr(), w, r, s, a0.cuda_event, a1.cuda_event)
    if rc:
        raise _lib.DpwaError(name, rc, lib.dpwa_last_error().decode())


def compare(libs, code, tdtype, n, G, forms, n_sets, launches, warmup, dev, work, rec):
    sets = [BufferSet(n, tdtype, dev, G) for _ in range(n_sets)]
    s = _lib.stream_handle(None)
    total = warmup + launches
    ev = {f[0]: events(total) for f in forms}
    torch.cuda.synchronize()
    j = 0
    for i in range(total):
        k = i % len(forms)
        for form in forms[k:] + forms[:k]:          # no form always follows the same other one
            launch(libs, form, code, sets[j % n_sets], G, n, work, rec, s, *ev[form[0]][i])
            j += 1
    torch.cuda.synchronize()
    return {f: [1e3 * a.elapsed_time(b) for a, b in pairs[warmup:]] for f, pairs in ev.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default="consensus_trim_cost.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("consensus_trim_cost.py needs a GPU")
    dev = torch.device("cuda", 0)
    libs = {"this": _lib.load()}
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.dpwa_consensus.argtypes = _lib.SIGNATURES["dpwa_consensus"]
        parent.dpwa_last_error.restype = ctypes.c_char_p
        libs["parent"] = parent
    nbytes = ctypes.c_int64()
    _lib.call("dpwa_consensus_workspace", ctypes.byref(nbytes))
    work = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
    rec = torch.zeros(128, dtype=torch.uint8, device=dev)
    out = {"what": "dpwa_consensus_trimmed (t = 1, median) against dpwa_consensus (the mean; this build and, with "
                   "parent_*, the parent commit's) on the same cold buffers, interleaved launch by launch; dispatch "
                   "begin/end events; full = store + distance, store = the centre only",
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "launches": args.launches, "sizes": {}}
    brief = {}
    for name, code, tdtype, n in SIZES:
        esize = torch.empty((), dtype=tdtype).element_size()
        out["sizes"][name] = {"numel": n}
        for G in GROUPS:
            forms = forms_of(G, args.parent_lib)
            n_sets = -(-3 * CACHE // ((G + 1) * esize * n)) + 1
            us = compare(libs, code, tdtype, n, G, forms, n_sets, args.launches, args.warmup, dev, work, rec)
            entry = {f: stats(v) for f, v in us.items()}
            entry["bytes_per_launch"], entry["cold_sets"] = (G + 1) * esize * n, n_sets
            for f in us:
                if not f.startswith("mean"):
                    base = "mean_full" if f.endswith("full") else "mean_store"
                    entry[f + "_over_mean_median"] = round(entry[f]["median_us"] / entry[base]["median_us"], 4)
            out["sizes"][name]["G%d" % G] = entry
            brief["%s G%d" % (name, G)] = {k: v for k, v in entry.items() if k.endswith("_over_mean_median")}
            brief["%s G%d" % (name, G)]["mean_full_us"] = entry["mean_full"]["median_us"]
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
