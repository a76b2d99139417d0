"""What the per-parameter distance costs: its pass (dpwa_measure_param_distance) against the existing
stand-alone whole-model pass (dpwa_measure_distance, whose code it leaves alone) on the same buffers,
interleaved launch by launch in one process.  The baseline is always the whole-model pass of the same
run.

The whole-model entry takes no events, so the comparison ("call") is an event pair recorded on the
stream around each entry -- pass plus finishing step, for both alike, neither launch recording events
of its own.  The new pass and its finishing step are also timed alone, in launches of their own, by
the events the ABI records around the dispatch itself (hipExtLaunchKernelGGL): "param_pass", "finish".

Layouts:
  resnet18   ResNet-18's 62 tensors, 11,173,962 float32, each on its 256-byte boundary
  one-bf16   one tensor of 2^26 bfloat16: the same bytes and the same 1024 rows as the baseline, so any
             gap is the table lookup and the branch
  16k-f32    16,384 tensors of 1,000 float32: most spans hold two tensors (baseline: the _mixed entry
             with the payload as one float32 segment)
Per layout, three repeats of --launches launches of each after --warmup:
  warm   one buffer pair, launches back to back (part of it still in the 256 MiB Infinity Cache)
  cold   buffer pairs rotated so that at least three cache sizes of other bytes pass between two uses
and the adapter's wall time per round (tools/host_round.py's loop) at ResNet-18 with
track_distance=True against "per_parameter" with distance_every 1 and 100.

    python tools/param_distance_cost.py [--launches K] [--warmup W] [--repeats R] [--out FILE]
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
for path in (ROOT, os.path.join(ROOT, "examples")):
    if path not in sys.path:
        sys.path.insert(0, path)

import torch  # noqa: E402

import bench  # noqa: E402
from dpwa_amd import DpwaPyTorchAdapter, _lib  # noqa: E402
from dpwa_amd.group import LocalGroup  # noqa: E402
from distance_cost import CACHE, events, stats  # noqa: E402  (tools/ is the script's directory)
from resnet18_gossip import resnet18  # noqa: E402


def ranges_of(sizes, esize):
    """[(byte offset, byte length)] of tensors of `sizes` elements, each on a 256-byte boundary, and
    the payload's bytes (dpwa_amd/flat.py's single-dtype layout)."""
    out, off = [], 0
    for n in sizes:
        out.append((off, n * esize))
        off += -(-n * esize // 256) * 256
    return out, off


def layouts():
    with torch.device("meta"):
        resnet = [p.numel() for p in resnet18().parameters()]
    assert sum(resnet) == 11_173_962 and len(resnet) == 62
    return [("resnet18", _lib.F32, 4, resnet), ("one-bf16", _lib.BF16, 2, [1 << 26]), ("16k-f32", _lib.F32, 4, [1000] * 16384)]


class Layout:
    def __init__(self, name, code, esize, sizes, dev):
        self.name, self.code, self.esize = name, code, esize
        ranges, self.total = ranges_of(sizes, esize)
        self.count = len(ranges)
        arr = (_lib.ParamRange * self.count)(*[_lib.ParamRange(o, b, code, 0) for o, b in ranges])
        self.sizes = _lib.ParamSizes()
        _lib.call("dpwa_param_distance_sizes", arr, self.count, ctypes.byref(self.sizes))
        self.table = torch.zeros(self.sizes.table_bytes, dtype=torch.uint8, device=dev)
        self.work = torch.zeros(self.sizes.workspace_bytes, dtype=torch.uint8, device=dev)
        self.rec = torch.zeros(self.sizes.record_bytes, dtype=torch.uint8, device=dev)
        _lib.call("dpwa_param_distance_table", arr, self.count, self.table.data_ptr())
        self.segment = _lib.Layout()          # the payload as one float32 segment (16k-f32's baseline)
        self.segment.count = 1
        self.segment.seg[0] = _lib.Segment(code, 0, 0, self.total)
        self.as_mixed = name == "16k-f32"
        assert not self.as_mixed or self.total % _lib.LAYOUT_ALIGN == 0

    def pair(self, dev):
        t = torch.float32 if self.esize == 4 else torch.float16     # N(0,1) bit patterns; bf16 reads them as finite too
        return (torch.empty(self.total // self.esize, device=dev, dtype=t).normal_(),
                torch.empty(self.total // self.esize, device=dev, dtype=t).normal_())


def compare(lib, lay, n_sets, launches, warmup, dev, base_work, base_rec):
    sets = [lay.pair(dev) for _ in range(n_sets)]
    s = _lib.stream_handle(None)
    total = warmup + launches
    ev = {k: events(total) for k in ("baseline_call", "param_call", "timed_call", "param_pass")}
    torch.cuda.synchronize()
    j = 0
    for i in range(total):
        # neither always follows the other; "timed": the new entry once more with the dispatch's own events,
        # apart from the compared call, since a launch that records events is itself slower to start
        for name in (("baseline", "param", "timed") if i % 2 == 0 else ("param", "baseline", "timed")):
            p, q = sets[j % n_sets]
            j += 1
            a, b = ev[name + "_call"][i]
            a.record()
            if name != "baseline":
                p0, p1 = ev["param_pass"][i] if name == "timed" else (None, None)
                rc = lib.dpwa_measure_param_distance(lay.table.data_ptr(), lay.count, p.data_ptr(), q.data_ptr(), lay.total,
                                                     lay.work.data_ptr(), lay.rec.data_ptr(), s,
                                                     p0.cuda_event if p0 else None, p1.cuda_event if p1 else None)
            elif lay.as_mixed:
                rc = lib.dpwa_measure_distance_mixed(ctypes.byref(lay.segment), p.data_ptr(), q.data_ptr(),
                                                     base_work.data_ptr(), base_rec.data_ptr(), s)
            else:
                rc = lib.dpwa_measure_distance(lay.code, p.data_ptr(), q.data_ptr(), lay.total // lay.esize,
                                               base_work.data_ptr(), base_rec.data_ptr(), s)
            b.record()
            if rc:
                raise _lib.DpwaError("dpwa_measure_(param_)distance", rc, lib.dpwa_last_error().decode())
    torch.cuda.synchronize()
    return {name: [1e3 * a.elapsed_time(b) for a, b in pairs[warmup:]] for name, pairs in ev.items()}


def finish_times(lib, lay, launches, warmup):
    s = _lib.stream_handle(None)
    ev = events(warmup + launches)
    torch.cuda.synchronize()
    for a, b in ev:
        rc = lib.dpwa_param_distance_finish(lay.table.data_ptr(), lay.count, lay.work.data_ptr(), lay.rec.data_ptr(), None, s,
                                            a.cuda_event, b.cuda_event)
        if rc:
            raise _lib.DpwaError("dpwa_param_distance_finish", rc, lib.dpwa_last_error().decode())
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in ev[warmup:]]


def adapter_rounds(rounds, repeats, dev):
    """The adapter's round (update_send + update_wait, write-through default) on ResNet-18's tensors,
    the adapters taking turns in blocks of `rounds`: wall time per round."""
    tmp = tempfile.mkdtemp(prefix="dpwa_pdist_")
    kinds = {"whole_model": dict(track_distance=True),
             "per_parameter_every_1": dict(track_distance="per_parameter", distance_every=1),
             "per_parameter_every_100": dict(track_distance="per_parameter", distance_every=100)}
    ads = {}
    for k, (name, kw) in enumerate(kinds.items()):
        cfg = os.path.join(tmp, "a%d.yaml" % k)
        bench.write_config(cfg, ["a1"], "constant", self_peer=True, base_port=45950 + 10 * k)
        ads[name] = DpwaPyTorchAdapter(resnet18().to(dev), "a1", cfg, seed=3000, group=LocalGroup(), **kw)
    out = {name: [] for name in ads}
    for ad in ads.values():
        for _ in range(50):
            ad.update_send(1.0)
            ad.update_wait(1.0)
    torch.cuda.synchronize()
    names = list(ads)
    for rep in range(repeats):
        for name in names[rep % len(names):] + names[:rep % len(names)]:
            ad = ads[name]
            t0 = time.perf_counter()
            for _ in range(rounds):
                ad.update_send(1.0)
                ad.update_wait(1.0)
            torch.cuda.synchronize()
            out[name].append(round(1e6 * (time.perf_counter() - t0) / rounds, 3))
    for ad in ads.values():
        ad.connection.close()
    res = {"model": "ResNet-18 tensors, 11,173,962 float32", "rounds_per_block": rounds, "blocks": repeats}
    for name, walls in out.items():
        res[name] = {"wall_us": walls, "wall_us_median": statistics.median(walls)}
    for name in names[1:]:
        res[name]["over_whole_model"] = round(res[name]["wall_us_median"] / res["whole_model"]["wall_us_median"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="param_distance_cost.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("param_distance_cost.py needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    nbytes = ctypes.c_int64()
    _lib.call("dpwa_distance_workspace", ctypes.byref(nbytes))
    base_work = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
    base_rec = torch.zeros(32, dtype=torch.uint8, device=dev)
    out = {"what": "dpwa_measure_param_distance against dpwa_measure_distance(_mixed) on the same buffers, interleaved "
                   "launch by launch; *_call: an event pair around the entry (pass + finishing step); param_pass / "
                   "finish: the dispatch's own events",
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "launches": args.launches,
           "repeats": args.repeats, "layouts": {}}
    for name, code, esize, sizes in layouts():
        lay = Layout(name, code, esize, sizes, dev)
        cold_sets = -(-3 * CACHE // (2 * lay.total)) + 1
        entry = {"tensors": lay.count, "payload_bytes": lay.total, "bytes_read_per_launch": 2 * lay.total,
                 "table_bytes": lay.sizes.table_bytes, "workspace_bytes": lay.sizes.workspace_bytes,
                 "record_bytes": lay.sizes.record_bytes, "max_rows": lay.sizes.max_rows, "cold_sets": cold_sets}
        for mode, n_sets in (("warm", 1), ("cold", cold_sets)):
            reps = []
            for _ in range(args.repeats):
                us = compare(lib, lay, n_sets, args.launches, args.warmup, dev, base_work, base_rec)
                r = {k: stats(v) for k, v in us.items()}
                b, p = r["baseline_call"], r["param_call"]
                r["param_over_baseline_median"] = round(p["median_us"] / b["median_us"], 4)
                r["param_median_above_baseline_p90"] = p["median_us"] > b["p90_us"]
                reps.append(r)
                torch.cuda.empty_cache()
            entry[mode] = {"repeats": reps,
                           "param_over_baseline_median": statistics.median(r["param_over_baseline_median"] for r in reps)}
        entry["finish"] = [stats(finish_times(lib, lay, args.launches, args.warmup)) for _ in range(args.repeats)]
        out["layouts"][name] = entry
        del lay
        torch.cuda.empty_cache()
    out["adapter_round_resnet18"] = adapter_rounds(300, 2 * args.repeats, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    brief = {name: {mode: e[mode]["param_over_baseline_median"] for mode in ("warm", "cold")}
             for name, e in out["layouts"].items()}
    print(json.dumps({"param_over_baseline_median": brief,
                      "finish_median_us": {n: [r["median_us"] for r in e["finish"]] for n, e in out["layouts"].items()},
                      "adapter_round_resnet18": {k: v["wall_us_median"] for k, v in out["adapter_round_resnet18"].items()
                                                 if isinstance(v, dict)}}))


if __name__ == "__main__":
    main()
