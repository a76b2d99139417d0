"""What packed snapshots cost on the device: dpwa_pack and a local dpwa_unpack against
dpwa_stream_mix(nr=1, nw=1) over the payload's bytes on the same buffers, interleaved launch by launch in
one process, each launch timed by the events the ABI records around the dispatch itself.  The mix moves
2*n*s bytes where pack and unpack move about 1.27*n*s (float32) or 1.52*n*s (bfloat16), so each median
should not exceed the mix's p90 of the same repeat ("within_mix_p90").  No link is measured: the image and
the payload are both in this GPU's memory.

    python tools/pack_cost.py [--launches K] [--warmup W] [--repeats R] [--out FILE]
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
from tools.distance_cost import SIZES, events, stats  # noqa: E402

FORMS = ("mix", "pack", "unpack")


def compare(lib, code, tdtype, n, launches, warmup, max_blocks, dev):
    """One repeat: `launches` timed launches of each form, interleaved."""
    esize = torch.empty((), dtype=tdtype).element_size()
    host = torch.float32 if esize == 4 else torch.float16
    payload = torch.empty(n, device=dev, dtype=host).normal_()
    back = torch.empty(n, device=dev, dtype=host)
    size = ctypes.c_int64()
    _lib.call("dpwa_pack_bytes", code, n, ctypes.byref(size))
    image = torch.zeros(size.value, dtype=torch.uint8, device=dev)
    src, dst = (ctypes.c_void_p * 1)(payload.data_ptr()), (ctypes.c_void_p * 1)(back.data_ptr())
    nbytes = n * esize // 16 * 16
    s = _lib.stream_handle(None)
    total = warmup + launches
    ev = {f: events(total) for f in FORMS}
    torch.cuda.synchronize()
    for i in range(total):
        k = i % len(FORMS)
        for form in FORMS[k:] + FORMS[:k]:          # no form always follows the same other one
            a0, a1 = ev[form][i]
            if form == "mix":
                rc = lib.dpwa_stream_mix(dst, 1, src, 1, nbytes, s, a0.cuda_event, a1.cuda_event)
            elif form == "pack":
                rc = lib.dpwa_pack(code, payload.data_ptr(), n, image.data_ptr(), s, a0.cuda_event, a1.cuda_event)
            else:
                rc = lib.dpwa_unpack(code, image.data_ptr(), n, back.data_ptr(), max_blocks, s, a0.cuda_event,
                                     a1.cuda_event)
            if rc:
                raise _lib.DpwaError(form, rc, lib.dpwa_last_error().decode())
    torch.cuda.synchronize()
    return {f: [1e3 * a.elapsed_time(b) for a, b in pairs[warmup:]] for f, pairs in ev.items()}, size.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-blocks", type=int, default=1 << 20, help="of dpwa_unpack (uncapped: the kernel alone)")
    ap.add_argument("--out", default="pack_cost.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pack_cost.py needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    out = {"what": "dpwa_pack and a local dpwa_unpack against dpwa_stream_mix(nr=1, nw=1) over the payload's bytes on "
                   "the same buffers, interleaved launch by launch; dispatch begin/end events; no link is measured",
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "launches": args.launches,
           "repeats": args.repeats, "unpack_max_blocks": args.max_blocks, "sizes": {}}
    for name, code, tdtype, n in SIZES:
        reps = []
        for _ in range(args.repeats):
            us, image_bytes = compare(lib, code, tdtype, n, args.launches, args.warmup, args.max_blocks, dev)
            r = {k: stats(v) for k, v in us.items()}
            for f in FORMS[1:]:
                r[f + "_within_mix_p90"] = r[f]["median_us"] <= r["mix"]["p90_us"]
            reps.append(r)
            torch.cuda.empty_cache()
        esize = torch.empty((), dtype=tdtype).element_size()
        out["sizes"][name] = {"numel": n, "payload_bytes": n * esize, "image_bytes": image_bytes, "repeats": reps}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({nm: [{f: r[f]["median_us"] for f in FORMS} | {"mix_p90_us": r["mix"]["p90_us"]}
                           for r in e["repeats"]] for nm, e in out["sizes"].items()}))


if __name__ == "__main__":
    main()
