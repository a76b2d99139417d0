"""The write-through fused average (dpwa_average with a snapshot payload) for DPWA_F16 against
DPWA_BF16 on the same buffers, interleaved in one process: the two kernels move the same bytes
(2 reads + 2 writes of 2 bytes per element) and differ only in how they convert (v_cvt_f32_f16 /
v_cvt_pk_f16_f32 against shifts / v_cvt_pk_bf16_f32).  Each launch is timed by the events the
ABI records around the dispatch itself (hipExtLaunchKernelGGL).

The yardstick is the bf16 kernel of the same run: the JSON holds every launch's time, the medians
and the spread of both.  The launches run back to back over one set of buffers (parameters, peer
slot, next snapshot: 3 x 2 bytes x numel); at the default 2^26 elements that is 384 MiB against a
256 MiB Infinity Cache, so every launch finds part of its operands there: the times are neither
cold nor in-loop ones (the rate they imply is above the HBM ceiling) and only compare the two
dtypes, which meet the same cache state alternately (tools/cold_sweep.py rotates buffer sets for
cold times).

    python tools/f16_vs_bf16.py [--numel N] [--launches K] [--warmup W] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=int, default=1 << 26)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="f16_vs_bf16.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("f16_vs_bf16.py needs a GPU")
    dev = torch.device("cuda", 0)
    n = args.numel
    hdr = _lib.SLOT_PAYLOAD_OFFSET // 2
    # fp16 N(0, 1) bit patterns: finite (tiny) values read as bf16 too
    param = torch.empty(n, device=dev, dtype=torch.float16).normal_()
    slot = torch.zeros(hdr + n, device=dev, dtype=torch.float16)
    slot[hdr:].normal_()
    snap = torch.empty(hdr + n, device=dev, dtype=torch.float16)[hdr:]
    clock = torch.zeros(2, device=dev, dtype=torch.float64)
    coef = torch.zeros(4, device=dev, dtype=torch.float64)
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    lib = _lib.load()
    s = _lib.stream_handle(None)
    dtypes = [("f16", _lib.F16), ("bf16", _lib.BF16)]
    total = args.warmup + args.launches
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(total)]
          for name, _ in dtypes}
    for pairs in ev.values():
        for a, b in pairs:       # create the events (the dispatch then records into them)
            a.record()
            b.record()

    def run(name, code, i):
        a, b = ev[name][i]
        rc = lib.dpwa_average(code, param.data_ptr(), slot.data_ptr(), n, ctypes.byref(cfg), clock.data_ptr(), 1.0,
                              coef.data_ptr(), snap.data_ptr(), s, a.cuda_event, b.cuda_event)
        if rc:
            raise _lib.DpwaError("dpwa_average", rc, lib.dpwa_last_error().decode())

    torch.cuda.synchronize()
    for i in range(total):
        order = dtypes if i % 2 == 0 else dtypes[::-1]     # neither dtype always follows the other
        for name, code in order:
            run(name, code, i)
    torch.cuda.synchronize()
    nbytes = 4 * 2 * n
    out = {"what": "dpwa_average write-through, DPWA_F16 vs DPWA_BF16, same buffers, interleaved",
           "device": torch.cuda.get_device_name(0), "numel": n, "bytes_per_launch": nbytes,
           "working_set_bytes": 3 * 2 * n, "warmup": args.warmup, "launches": args.launches, "dtypes": {}}
    for name, _ in dtypes:
        us = [1e3 * a.elapsed_time(b) for a, b in ev[name][args.warmup:]]
        srt = sorted(us)
        med = statistics.median(us)
        out["dtypes"][name] = {
            "us": [round(x, 2) for x in us], "median_us": round(med, 2), "min_us": round(srt[0], 2),
            "max_us": round(srt[-1], 2), "p10_us": round(srt[len(srt) // 10], 2),
            "p90_us": round(srt[(9 * len(srt)) // 10], 2), "median_gb_per_s": round(nbytes / med / 1e3, 1)}
    f16, bf16 = out["dtypes"]["f16"], out["dtypes"]["bf16"]
    out["f16_over_bf16_median"] = round(f16["median_us"] / bf16["median_us"], 4)
    out["f16_median_within_bf16_p10_p90"] = bf16["p10_us"] <= f16["median_us"] <= bf16["p90_us"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "dtypes"}
                     | {name: {k: v for k, v in d.items() if k != "us"} for name, d in out["dtypes"].items()}))


if __name__ == "__main__":
    main()
