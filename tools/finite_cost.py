"""What skipping non-finite peers costs (skip_nonfinite_peer; kernels.hip "non-finite peer check").

  pass    dpwa_check_finite alone, timed by its own dispatch events (hipExtLaunchKernelGGL), at
          11,173,962 float32 and 2^26 bfloat16, warm (one buffer) and cold (buffers rotated so that
          three cache sizes of other bytes pass between two uses), three repeats of --launches
          launches after --warmup.  Interleaved launch by launch with a baseline of the same launch
          shape: dpwa_stream_mix with one source and one destination -- it refuses a launch with no
          destination, so the baseline reads the bytes once AND writes as many, twice the pass's
          traffic; the pass's own GB/s is reported beside it.
  policy  the pass followed by the fused average (dpwa_average) on the same peer snapshot, both timed
          by their dispatch events, with the pass's loads default against `nt` (DPWA_FINITE_LOADS, read
          once per process: fresh child processes taking turns), at 11,173,962 float32 (the round's
          buffers fit the Infinity Cache) and 100,000,000 float32 (they do not).
  round   the adapter's round (tools/host_round.py's loop: update_send + update_wait, write-through
          default) with the switch on against off, the two adapters taking turns in blocks of 300
          rounds, at 11,173,962 float32.

    python tools/finite_cost.py [--launches K] [--warmup W] [--repeats R] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
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
from tools.distance_cost import CACHE, SIZES, events, stats  # noqa: E402

POLICY_SIZES = [11_173_962, 100_000_000]


def check(lib, name, rc):
    if rc:
        raise _lib.DpwaError(name, rc, lib.dpwa_last_error().decode())


def pass_alone(lib, code, tdtype, n, n_sets, launches, warmup, dev):
    """One repeat: the pass and the one-read-one-write stream, interleaved, over `n_sets` rotated buffers."""
    esize = torch.empty((), dtype=tdtype).element_size()
    nbytes = n * esize // 16 * 16
    raw = torch.float32 if esize == 4 else torch.float16
    peers = [torch.empty(n, device=dev, dtype=raw).normal_() for _ in range(n_sets)]
    dsts = [torch.empty(n, device=dev, dtype=raw) for _ in range(n_sets)]
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    s = _lib.stream_handle(None)
    total = warmup + launches
    ev = {"pass": events(total), "stream_1r1w": events(total)}
    torch.cuda.synchronize()
    j = 0
    for i in range(total):
        for name in (("pass", "stream_1r1w") if i % 2 == 0 else ("stream_1r1w", "pass")):
            k = j % n_sets
            j += 1
            a, b = ev[name][i]
            if name == "pass":
                check(lib, "dpwa_check_finite", lib.dpwa_check_finite(code, peers[k].data_ptr(), n, word.data_ptr(), i + 1, s,
                                                                       a.cuda_event, b.cuda_event))
            else:
                src, dst = (ctypes.c_void_p * 1)(peers[k].data_ptr()), (ctypes.c_void_p * 1)(dsts[k].data_ptr())
                check(lib, "dpwa_stream_mix", lib.dpwa_stream_mix(dst, 1, src, 1, nbytes, s, a.cuda_event, b.cuda_event))
    torch.cuda.synchronize()
    assert int(word.item()) == 0, "N(0,1) data vetoed"
    return {name: [1e3 * a.elapsed_time(b) for a, b in pairs[warmup:]] for name, pairs in ev.items()}


def policy_child(n, launches, warmup):
    """Child process (DPWA_FINITE_LOADS set by the parent): the pass, then the plain fused average of
    the same snapshot; one buffer set below the cache-fit threshold (warm, as a gossip loop), rotated
    sets above it.  Prints the per-launch microseconds of both."""
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    set_bytes = 2 * 4 * n
    n_sets = 1 if 3 * 4 * n <= (160 << 20) else -(-3 * CACHE // set_bytes) + 1
    hdr = _lib.SLOT_PAYLOAD_OFFSET // 4
    params = [torch.empty(n, device=dev).normal_() for _ in range(n_sets)]
    slots = [torch.zeros(hdr + n, device=dev) for _ in range(n_sets)]
    for t in slots:
        t[hdr:].normal_()
    clock, coef = torch.zeros(2, device=dev, dtype=torch.float64), torch.zeros(4, device=dev, dtype=torch.float64)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    s = _lib.stream_handle(None)
    total = warmup + launches
    ev = {"pass": events(total), "average": events(total)}
    torch.cuda.synchronize()
    for i in range(total):
        k = i % n_sets
        (a0, a1), (b0, b1) = ev["pass"][i], ev["average"][i]
        check(lib, "dpwa_check_finite", lib.dpwa_check_finite(_lib.F32, slots[k].data_ptr() + _lib.SLOT_PAYLOAD_OFFSET, n,
                                                               word.data_ptr(), i + 1, s, a0.cuda_event, a1.cuda_event))
        check(lib, "dpwa_average", lib.dpwa_average(_lib.F32, params[k].data_ptr(), slots[k].data_ptr(), n, ctypes.byref(cfg),
                                                    clock.data_ptr(), 1.0, coef.data_ptr(), None, s, b0.cuda_event,
                                                    b1.cuda_event))
    torch.cuda.synchronize()
    us = {name: [1e3 * a.elapsed_time(b) for a, b in pairs[warmup:]] for name, pairs in ev.items()}
    us["both"] = [x + y for x, y in zip(us["pass"], us["average"])]
    print(json.dumps({name: stats(v) for name, v in us.items()}))


def policy_ab(n, launches, warmup, repeats):
    out = {"default": [], "nt": []}
    for rep in range(repeats):
        for loads in (("default", "nt") if rep % 2 == 0 else ("nt", "default")):
            env = dict(os.environ, DPWA_FINITE_LOADS=loads)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--launches", str(launches),
                                  "--warmup", str(warmup)], env=env, capture_output=True, text=True, timeout=600)
            if res.returncode:
                raise SystemExit("policy child failed (%d): %s" % (res.returncode, res.stderr[-2000:]))
            out[loads].append(json.loads(res.stdout.strip().splitlines()[-1]))
            print("policy %d %s: %s" % (n, loads, out[loads][-1]["both"]), file=sys.stderr, flush=True)
    med = {k: statistics.median(r["both"]["median_us"] for r in v) for k, v in out.items()}
    return {"numel": n, "runs": out, "both_median_us": med, "nt_over_default": round(med["nt"] / med["default"], 4)}


def adapter_rounds(numel, rounds, repeats, dev):
    """The adapter's round with the switch off and on, taking turns in blocks of `rounds`."""
    tmp = tempfile.mkdtemp(prefix="dpwa_finite_")
    ads = {}
    for k, name in enumerate(("off", "on")):
        cfg = os.path.join(tmp, "a%d.yaml" % k)
        bench.write_config(cfg, ["a1"], "constant", self_peer=True, base_port=45700 + 10 * k)
        net = torch.nn.Module()
        net.register_parameter("w", torch.nn.Parameter(torch.randn(numel, device=dev)))
        ads[name] = DpwaPyTorchAdapter(net, "a1", cfg, seed=3000, group=LocalGroup(), skip_nonfinite_peer=name == "on")
    out = {name: {"issue_us": [], "wall_us": []} for name in ads}
    for ad in ads.values():
        for _ in range(50):
            ad.update_send(1.0)
            ad.update_wait(1.0)
    torch.cuda.synchronize()
    for rep in range(repeats):
        for name in (("off", "on") if rep % 2 == 0 else ("on", "off")):
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
    skips = {name: ad.nonfinite_skips for name, ad in ads.items()}
    for ad in ads.values():
        ad.connection.close()
    res = {"numel": numel, "rounds_per_block": rounds, "blocks": repeats, "skips": skips}
    for name, d in out.items():
        res[name] = dict(d, issue_us_median=statistics.median(d["issue_us"]), wall_us_median=statistics.median(d["wall_us"]))
    res["on_over_off_wall"] = round(res["on"]["wall_us_median"] / res["off"]["wall_us_median"], 4)
    res["on_over_off_issue"] = round(res["on"]["issue_us_median"] / res["off"]["issue_us_median"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="finite_cost.json")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finite_cost.py needs a GPU")
    if args.child:
        return policy_child(args.child, args.launches, args.warmup)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    out = {"what": "dpwa_check_finite alone against a one-read-one-write stream of the same launch shape; the pass's "
                   "load policy under the pass + average; the adapter's round with skip_nonfinite_peer on against off",
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "launches": args.launches,
           "repeats": args.repeats, "pass": {}}
    for name, code, tdtype, n in SIZES:
        esize = torch.empty((), dtype=tdtype).element_size()
        cold_sets = -(-3 * CACHE // (2 * esize * n)) + 1
        entry = {"numel": n, "bytes_read": esize * n, "cold_sets": cold_sets}
        for mode, n_sets in (("warm", 1), ("cold", cold_sets)):
            reps = []
            for _ in range(args.repeats):
                us = pass_alone(lib, code, tdtype, n, n_sets, args.launches, args.warmup, dev)
                r = {k: stats(v) for k, v in us.items()}
                r["pass_gb_per_s"] = round(esize * n / r["pass"]["median_us"] / 1e3, 1)
                r["pass_over_stream_median"] = round(r["pass"]["median_us"] / r["stream_1r1w"]["median_us"], 4)
                reps.append(r)
                torch.cuda.empty_cache()
            entry[mode] = {"repeats": reps, "pass_median_us": statistics.median(r["pass"]["median_us"] for r in reps),
                           "pass_gb_per_s": statistics.median(r["pass_gb_per_s"] for r in reps),
                           "pass_over_stream_median": statistics.median(r["pass_over_stream_median"] for r in reps)}
        out["pass"][name] = entry
    out["policy"] = {str(n): policy_ab(n, args.launches, args.warmup, 2 * args.repeats) for n in POLICY_SIZES}
    out["adapter_round_f32"] = adapter_rounds(SIZES[0][3], 300, 2 * args.repeats, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"pass_median_us": {k: {m: e[m]["pass_median_us"] for m in ("warm", "cold")} for k, e in out["pass"].items()},
                      "pass_gb_per_s": {k: {m: e[m]["pass_gb_per_s"] for m in ("warm", "cold")} for k, e in out["pass"].items()},
                      "nt_over_default": {k: v["nt_over_default"] for k, v in out["policy"].items()},
                      "round_on_over_off_wall": out["adapter_round_f32"]["on_over_off_wall"]}))


if __name__ == "__main__":
    main()
