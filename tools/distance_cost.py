"""What distance tracking costs: the write-through tracked average (dpwa_average_tracked) against the
untracked product kernel (dpwa_average) on the same buffers, interleaved launch by launch in one
process, each launch timed by the events the ABI records around the dispatch itself
(hipExtLaunchKernelGGL).  The baseline is always the untracked kernel of the same run.

Per size (11,173,962 float32 and 2^26 bfloat16 by default), three repeats of --launches launches of
each kernel after --warmup:
  warm   one buffer set (parameters, peer slot, next snapshot), launches back to back: part of every
         launch's operands is still in the 256 MiB Infinity Cache, for both kernels alike
  cold   buffer sets rotated so that at least three cache sizes of other bytes pass between two uses
         of a set: every launch reads from HBM
The tracked figure is the averaging kernel alone; the finishing step (dpwa_distance_finish: one
workgroup that sums and zeroes the accumulators) is timed separately the same way, and the adapter's
round is timed with and without track_distance (tools/host_round.py's loop: host issue time at a
small model, wall time per round at the float32 size).

    python tools/distance_cost.py [--launches K] [--warmup W] [--repeats R] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from dpwa_amd import DpwaPyTorchAdapter, _lib  # noqa: E402
from dpwa_amd.group import LocalGroup  # noqa: E402

CACHE = 256 << 20
SIZES = [("f32", _lib.F32, torch.float32, 11_173_962), ("bf16", _lib.BF16, torch.bfloat16, 1 << 26)]


def stats(us):
    srt = sorted(us)
    return {"median_us": round(statistics.median(us), 3), "p10_us": round(srt[len(srt) // 10], 3),
            "p90_us": round(srt[(9 * len(srt)) // 10], 3), "min_us": round(srt[0], 3), "max_us": round(srt[-1], 3),
            "launches": len(us)}


def events(count):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(count)]
    for a, b in ev:                 # create them (the dispatch then records into them)
        a.record()
        b.record()
    return ev


class BufferSet:
    def __init__(self, n, tdtype, dev):
        esize = torch.empty((), dtype=tdtype).element_size()
        hdr = _lib.SLOT_PAYLOAD_OFFSET // esize
        self.param = torch.empty(n, device=dev, dtype=torch.float32 if esize == 4 else torch.float16).normal_()
        self.slot = torch.zeros(hdr + n, device=dev, dtype=self.param.dtype)
        self.slot[hdr:].normal_()
        self.snap = torch.empty(hdr + n, device=dev, dtype=self.param.dtype)[hdr:]


def compare(lib, code, tdtype, n, n_sets, launches, warmup, dev, work, rec):
    """One repeat: `launches` timed launches of each kernel, interleaved, over `n_sets` rotated sets."""
    sets = [BufferSet(n, tdtype, dev) for _ in range(n_sets)]
    clock = torch.zeros(2, device=dev, dtype=torch.float64)
    coef = torch.zeros(4, device=dev, dtype=torch.float64)
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    s = _lib.stream_handle(None)
    total = warmup + launches
    ev = {"untracked": events(total), "tracked": events(total)}
    torch.cuda.synchronize()
    j = 0
    for i in range(total):
        order = ("untracked", "tracked") if i % 2 == 0 else ("tracked", "untracked")   # neither always follows the other
        for name in order:
            b = sets[j % n_sets]
            j += 1
            a0, a1 = ev[name][i]
            head = (code, b.param.data_ptr(), b.slot.data_ptr(), n, ctypes.byref(cfg), clock.data_ptr(), 1.0,
                    coef.data_ptr(), b.snap.data_ptr())
            if name == "untracked":
                rc = lib.dpwa_average(*head, s, a0.cuda_event, a1.cuda_event)
            else:
                rc = lib.dpwa_average_tracked(*head, work.data_ptr(), rec.data_ptr(), s, a0.cuda_event, a1.cuda_event)
            if rc:
                raise _lib.DpwaError("dpwa_average(_tracked)", rc, lib.dpwa_last_error().decode())
    torch.cuda.synchronize()
    return {name: [1e3 * a.elapsed_time(b) for a, b in pairs[warmup:]] for name, pairs in ev.items()}


def finish_times(lib, launches, warmup, work, rec):
    s = _lib.stream_handle(None)
    ev = events(warmup + launches)
    torch.cuda.synchronize()
    for a, b in ev:
        rc = lib.dpwa_distance_finish(work.data_ptr(), rec.data_ptr(), None, 0, s, a.cuda_event, b.cuda_event)
        if rc:
            raise _lib.DpwaError("dpwa_distance_finish", rc, lib.dpwa_last_error().decode())
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in ev[warmup:]]


def adapter_rounds(numel, rounds, repeats, dev):
    """The adapter's round (update_send + update_wait, write-through default) with and without
    tracking, the two adapters taking turns in blocks of `rounds`: host issue time per round
    (perf_counter over the block, before the device is waited for) and wall time per round."""
    tmp = tempfile.mkdtemp(prefix="dpwa_distance_")
    ads = {}
    for k, track in enumerate((False, True)):
        cfg = os.path.join(tmp, "a%d.yaml" % k)
        bench.write_config(cfg, ["a1"], "constant", self_peer=True, base_port=45900 + 10 * k)
        net = torch.nn.Module()
        net.register_parameter("w", torch.nn.Parameter(torch.randn(numel, device=dev)))
        ads["tracked" if track else "untracked"] = DpwaPyTorchAdapter(net, "a1", cfg, seed=3000, group=LocalGroup(),
                                                                     track_distance=track)
    out = {name: {"issue_us": [], "wall_us": []} for name in ads}
    for ad in ads.values():
        for _ in range(50):
            ad.update_send(1.0)
            ad.update_wait(1.0)
    torch.cuda.synchronize()
    for rep in range(repeats):
        for name in (("untracked", "tracked") if rep % 2 == 0 else ("tracked", "untracked")):
            ad = ads[name]
            t0 = time.perf_counter()
            for _ in range(rounds):
                ad.update_send(1.0)
                ad.update_wait(1.0)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            out[name]["issue_us"].append(round(1e6 * (t1 - t0) / rounds, 3))
            out[name]["wall_us"].append(round(1e6 * (t2 - t0) / rounds, 3))
    for ad in ads.values():
        ad.connection.close()
    res = {"numel": numel, "rounds_per_block": rounds, "blocks": repeats}
    for name, d in out.items():
        res[name] = dict(d, issue_us_median=statistics.median(d["issue_us"]), wall_us_median=statistics.median(d["wall_us"]))
    res["tracked_over_untracked_wall"] = round(res["tracked"]["wall_us_median"] / res["untracked"]["wall_us_median"], 4)
    res["tracked_over_untracked_issue"] = round(res["tracked"]["issue_us_median"] / res["untracked"]["issue_us_median"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="distance_cost.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distance_cost.py needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    nbytes = ctypes.c_int64()
    _lib.call("dpwa_distance_workspace", ctypes.byref(nbytes))
    work = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
    rec = torch.zeros(32, dtype=torch.uint8, device=dev)
    out = {"what": "dpwa_average_tracked (write-through) against dpwa_average on the same buffers, interleaved launch "
                   "by launch; the baseline is the untracked kernel of the same run",
           "device": torch.cuda.get_device_name(0), "workspace_bytes": nbytes.value,
           "accumulators": nbytes.value // _lib.DISTANCE_ACC_STRIDE, "warmup": args.warmup, "launches": args.launches,
           "repeats": args.repeats, "sizes": {}}
    for name, code, tdtype, n in SIZES:
        esize = torch.empty((), dtype=tdtype).element_size()
        set_bytes = 3 * esize * n
        cold_sets = -(-3 * CACHE // set_bytes) + 1
        entry = {"numel": n, "bytes_per_launch": 4 * esize * n, "set_bytes": set_bytes, "cold_sets": cold_sets}
        for mode, n_sets in (("warm", 1), ("cold", cold_sets)):
            reps = []
            for _ in range(args.repeats):
                us = compare(lib, code, tdtype, n, n_sets, args.launches, args.warmup, dev, work, rec)
                r = {k: stats(v) for k, v in us.items()}
                u, t = r["untracked"], r["tracked"]
                r["tracked_over_untracked_median"] = round(t["median_us"] / u["median_us"], 4)
                r["tracked_median_within_untracked_p10_p90"] = u["p10_us"] <= t["median_us"] <= u["p90_us"]
                reps.append(r)
                torch.cuda.empty_cache()
            entry[mode] = {"repeats": reps,
                           "tracked_over_untracked_median": statistics.median(r["tracked_over_untracked_median"] for r in reps)}
        out["sizes"][name] = entry
    out["finish"] = [stats(finish_times(lib, args.launches, args.warmup, work, rec)) for _ in range(args.repeats)]
    out["adapter_round_small"] = adapter_rounds(4096, 2000, 2 * args.repeats, dev)
    out["adapter_round_f32"] = adapter_rounds(SIZES[0][3], 300, 2 * args.repeats, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    brief = {name: {mode: e[mode]["tracked_over_untracked_median"] for mode in ("warm", "cold")}
             for name, e in out["sizes"].items()}
    print(json.dumps({"tracked_over_untracked_median": brief, "finish_median_us": [r["median_us"] for r in out["finish"]],
                      "adapter_round_small": out["adapter_round_small"]["tracked_over_untracked_issue"],
                      "adapter_round_f32": out["adapter_round_f32"]["tracked_over_untracked_wall"]}))


if __name__ == "__main__":
    main()
