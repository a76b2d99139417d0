"""What packed snapshots cost on the device: dpwa_pack and a local dpwa_unpack against
dpwa_stream_mix(nr=1, nw=1) over the payload's bytes on the same buffers, interleaved launch by launch in
one process, each launch timed by the events the ABI records around the dispatch itself.  The mix moves
2*n*s bytes where pack and unpack move about 1.27*n*s (float32) or 1.52*n*s (bfloat16), so each median
should not exceed the mix's p90 of the same repeat ("within_mix_p90").  No link is measured: the image and
the payload are both in this GPU's memory.

    python tools/pack_cost.py [--launches K] [--warmup W] [--repeats R] [--out FILE]

--avg measures the average straight from the image instead (profiles/pack_avg_cost.json), the same way, all
write-through: "pair" dpwa_unpack + dpwa_average back to back, from the first dispatch's begin to the second's end
(the two launches dpwa_average_packed replaces); "fused" dpwa_average_packed; "mix" dpwa_stream_mix(nr=2, nw=2), the
nearest mix its arguments express -- it reads 2 n s where the fused kernel reads (1 + 1/s + 1/64) n s, so it
over-counts reads; "avg" the plain dpwa_average, whose peer is contiguous.  Every buffer is local and, at these
sizes, Infinity-Cache warm from the launch before.

--emit measures the write-through average that packs its snapshot (profiles/pack_emit_cost.json), for both peer
sources ("payload": a contiguous peer, "image": a packed one) and both cold (a 1-GiB fill between the timed forms)
and cache-warm: "pair" dpwa_average / dpwa_average_packed + dpwa_pack of the snapshot, from the first dispatch's
begin to the second's end (the two launches dpwa_average_pack replaces); "fused" dpwa_average_pack; "avg" the plain
write-through average alone; "pack_if" dpwa_pack_if on a miss (what a guarded publish still launches).

--sr measures what stochastic rounding costs (profiles/pack_sr_cost.json): dpwa_pack_stochastic against dpwa_pack
and dpwa_average_pack_stochastic against dpwa_average_pack, for both peer sources, cache-warm, the four interleaved
launch by launch on the same buffers.
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


AVG_FORMS = ("pair", "fused", "mix", "avg")


def compare_avg(lib, code, tdtype, n, launches, warmup, max_blocks, dev):
    """One repeat of the --avg forms, interleaved; constant factor 0.5 on the same parameters throughout."""
    esize = torch.empty((), dtype=tdtype).element_size()
    off = _lib.SLOT_PAYLOAD_OFFSET // esize
    param, snap = torch.empty(n, device=dev, dtype=tdtype).normal_(), torch.empty(n, device=dev, dtype=tdtype)
    slot = torch.zeros(off + n, device=dev, dtype=tdtype)          # a zero header (clock 0), then the peer's payload
    slot[off:].normal_()
    size = ctypes.c_int64()
    _lib.call("dpwa_pack_bytes", code, n, ctypes.byref(size))
    image = torch.zeros(size.value, dtype=torch.uint8, device=dev)
    s = _lib.stream_handle(None)
    _lib.call("dpwa_pack", code, slot[off:].data_ptr(), n, image.data_ptr(), s, None, None)
    clock = torch.zeros(2, dtype=torch.float64, device=dev)
    coef = torch.zeros(32, dtype=torch.uint8, device=dev)
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    tail = (ctypes.byref(cfg), clock.data_ptr(), 1.0, coef.data_ptr(), snap.data_ptr(), s)
    src = (ctypes.c_void_p * 2)(param.data_ptr(), slot[off:].data_ptr())
    dst = (ctypes.c_void_p * 2)(param.data_ptr(), snap.data_ptr())
    nbytes = n * esize // 16 * 16
    total = warmup + launches
    ev = {f: events(total) for f in AVG_FORMS}
    mid = events(total)
    torch.cuda.synchronize()
    for i in range(total):
        k = i % len(AVG_FORMS)
        for form in AVG_FORMS[k:] + AVG_FORMS[:k]:
            a0, a1 = (e.cuda_event for e in ev[form][i])
            if form == "pair":
                m0, m1 = (e.cuda_event for e in mid[i])
                rc = lib.dpwa_unpack(code, image.data_ptr(), n, slot[off:].data_ptr(), max_blocks, s, a0, m0) or \
                    lib.dpwa_average(code, param.data_ptr(), slot.data_ptr(), n, *tail, m1, a1)
            elif form == "fused":
                rc = lib.dpwa_average_packed(code, param.data_ptr(), slot.data_ptr(), image.data_ptr(), n, *tail, a0, a1)
            elif form == "mix":
                rc = lib.dpwa_stream_mix(dst, 2, src, 2, nbytes, s, a0, a1)
            else:
                rc = lib.dpwa_average(code, param.data_ptr(), slot.data_ptr(), n, *tail, a0, a1)
            if rc:
                raise _lib.DpwaError(form, rc, lib.dpwa_last_error().decode())
    torch.cuda.synchronize()
    return {f: [1e3 * a.elapsed_time(b) for a, b in pairs[warmup:]] for f, pairs in ev.items()}, size.value


def main_avg(args, lib, dev):
    out = {"what": "the average straight from a packed image, write-through: pair = dpwa_unpack + dpwa_average from the "
                   "first begin to the second end, fused = dpwa_average_packed, mix = dpwa_stream_mix(nr=2, nw=2) "
                   "(over-counts the fused kernel's reads), avg = dpwa_average from a contiguous peer; interleaved "
                   "launch by launch on the same buffers, all local and Infinity-Cache warm; no link is measured",
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "launches": args.launches,
           "repeats": args.repeats, "unpack_max_blocks": args.max_blocks,
           "DPWA_PACKED_SCALES": os.environ.get("DPWA_PACKED_SCALES", ""), "sizes": {}}
    for name, code, tdtype, n in SIZES:
        reps = []
        for _ in range(args.repeats):
            us, image_bytes = compare_avg(lib, code, tdtype, n, args.launches, args.warmup, args.max_blocks, dev)
            r = {k: stats(v) for k, v in us.items()}
            for f in AVG_FORMS[:1] + AVG_FORMS[2:]:
                r["fused_over_" + f] = round(r["fused"]["median_us"] / r[f]["median_us"], 3)
            reps.append(r)
            torch.cuda.empty_cache()
        out["sizes"][name] = {"numel": n, "image_bytes": image_bytes, "repeats": reps}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({nm: [{f: r[f]["median_us"] for f in AVG_FORMS} for r in e["repeats"]]
                      for nm, e in out["sizes"].items()}))


EMIT_FORMS = ("pair", "fused", "avg", "pack_if")


def compare_emit(lib, code, tdtype, n, launches, warmup, dev, source, cold):
    """One repeat of the --emit forms, interleaved; constant factor 0.5 on the same parameters throughout."""
    esize = torch.empty((), dtype=tdtype).element_size()
    off = _lib.SLOT_PAYLOAD_OFFSET // esize
    param, snap = torch.empty(n, device=dev, dtype=tdtype).normal_(), torch.empty(n, device=dev, dtype=tdtype)
    slot = torch.zeros(off + n, device=dev, dtype=tdtype)          # a zero header (clock 0), then the peer's payload
    slot[off:].normal_()
    size = ctypes.c_int64()
    _lib.call("dpwa_pack_bytes", code, n, ctypes.byref(size))
    peer_image, out_image = (torch.zeros(size.value, dtype=torch.uint8, device=dev) for _ in range(2))
    s = _lib.stream_handle(None)
    _lib.call("dpwa_pack", code, slot[off:].data_ptr(), n, peer_image.data_ptr(), s, None, None)
    clock = torch.zeros(2, dtype=torch.float64, device=dev)
    coef = torch.zeros(32, dtype=torch.uint8, device=dev)
    dirty = torch.zeros(1, dtype=torch.int32, device=dev)          # never this publish's generation: a miss
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    tail = (ctypes.byref(cfg), clock.data_ptr(), 1.0, coef.data_ptr(), snap.data_ptr())
    scrub = torch.empty(1 << 28, dtype=torch.float32, device=dev) if cold else None
    payload, image = slot[off:].data_ptr(), peer_image.data_ptr()

    def average(a0, a1):
        if source == "payload":
            return lib.dpwa_average(code, param.data_ptr(), slot.data_ptr(), n, *tail, s, a0, a1)
        return lib.dpwa_average_packed(code, param.data_ptr(), slot.data_ptr(), image, n, *tail, s, a0, a1)

    total = warmup + launches
    ev = {f: events(total) for f in EMIT_FORMS}
    mid = events(total)
    torch.cuda.synchronize()
    for i in range(total):
        k = i % len(EMIT_FORMS)
        for form in EMIT_FORMS[k:] + EMIT_FORMS[:k]:
            if cold:
                scrub.fill_(float(i))
            a0, a1 = (e.cuda_event for e in ev[form][i])
            if form == "pair":
                m0, m1 = (e.cuda_event for e in mid[i])
                rc = average(a0, m0) or lib.dpwa_pack(code, snap.data_ptr(), n, out_image.data_ptr(), s, m1, a1)
            elif form == "fused":
                rc = lib.dpwa_average_pack(code, param.data_ptr(), slot.data_ptr(), payload if source == "payload" else None,
                                           None if source == "payload" else image, n, *tail, out_image.data_ptr(), s, a0, a1)
            elif form == "avg":
                rc = average(a0, a1)
            else:
                rc = lib.dpwa_pack_if(code, snap.data_ptr(), n, out_image.data_ptr(), dirty.data_ptr(), 1, s, a0, a1)
            if rc:
                raise _lib.DpwaError(form, rc, lib.dpwa_last_error().decode())
    torch.cuda.synchronize()
    return {f: [1e3 * a.elapsed_time(b) for a, b in pairs[warmup:]] for f, pairs in ev.items()}


def main_emit(args, lib, dev):
    out = {"what": "the write-through average that packs its snapshot: pair = dpwa_average (source payload) or "
                   "dpwa_average_packed (source image) + dpwa_pack of the snapshot, from the first begin to the second "
                   "end; fused = dpwa_average_pack; avg = that average alone; pack_if = dpwa_pack_if on a miss; "
                   "interleaved launch by launch on the same local buffers, warm (Infinity-Cache warm from the launch "
                   "before) and cold (a 1-GiB fill before every timed form); no link is measured",
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "launches": args.launches,
           "repeats": args.repeats, "sizes": {}}
    for name, code, tdtype, n in SIZES:
        entry = {"numel": n}
        for source in ("payload", "image"):
            for cold in (False, True):
                reps = []
                for _ in range(args.repeats):
                    us = compare_emit(lib, code, tdtype, n, args.launches, args.warmup, dev, source, cold)
                    reps.append({k: stats(v) for k, v in us.items()})
                    torch.cuda.empty_cache()
                pair = [r["pair"]["median_us"] for r in reps]
                entry["%s_%s" % (source, "cold" if cold else "warm")] = {
                    "repeats": reps, "pair_median_spread_us": round(max(pair) - min(pair), 3)}
        out["sizes"][name] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({nm: {k: [{f: r[f]["median_us"] for f in EMIT_FORMS} for r in v["repeats"]]
                           for k, v in e.items() if k != "numel"} for nm, e in out["sizes"].items()}))


SR_FORMS = ("pack", "pack_sr", "emit", "emit_sr")


def compare_sr(lib, code, tdtype, n, launches, warmup, dev, source):
    """One repeat of the --sr forms, interleaved; compare_emit's buffers, the stochastic nonce changing every launch."""
    esize = torch.empty((), dtype=tdtype).element_size()
    off = _lib.SLOT_PAYLOAD_OFFSET // esize
    param, snap = torch.empty(n, device=dev, dtype=tdtype).normal_(), torch.empty(n, device=dev, dtype=tdtype)
    slot = torch.zeros(off + n, device=dev, dtype=tdtype)
    slot[off:].normal_()
    size = ctypes.c_int64()
    _lib.call("dpwa_pack_bytes", code, n, ctypes.byref(size))
    peer_image, out_image = (torch.zeros(size.value, dtype=torch.uint8, device=dev) for _ in range(2))
    s = _lib.stream_handle(None)
    _lib.call("dpwa_pack", code, slot[off:].data_ptr(), n, peer_image.data_ptr(), s, None, None)
    clock = torch.zeros(2, dtype=torch.float64, device=dev)
    coef = torch.zeros(32, dtype=torch.uint8, device=dev)
    cfg = _lib.Interp(_lib.INTERP_CONSTANT, 0, 0.5, 0.0)
    peer = (slot[off:].data_ptr(), None) if source == "payload" else (None, peer_image.data_ptr())
    emit = (code, param.data_ptr(), slot.data_ptr(), *peer, n, ctypes.byref(cfg), clock.data_ptr(), 1.0, coef.data_ptr(),
            snap.data_ptr(), out_image.data_ptr(), s)
    total = warmup + launches
    ev = {f: events(total) for f in SR_FORMS}
    torch.cuda.synchronize()
    for i in range(total):
        k = i % len(SR_FORMS)
        for form in SR_FORMS[k:] + SR_FORMS[:k]:
            a0, a1 = (e.cuda_event for e in ev[form][i])
            nonce = 0x9E3779B97F4A7C15 * (i + 1) % 2 ** 64
            if form == "pack":
                rc = lib.dpwa_pack(code, snap.data_ptr(), n, out_image.data_ptr(), s, a0, a1)
            elif form == "pack_sr":
                rc = lib.dpwa_pack_stochastic(code, snap.data_ptr(), n, out_image.data_ptr(), nonce, s, a0, a1)
            elif form == "emit":
                rc = lib.dpwa_average_pack(*emit, a0, a1)
            else:
                rc = lib.dpwa_average_pack_stochastic(*emit, a0, a1, nonce)
            if rc:
                raise _lib.DpwaError(form, rc, lib.dpwa_last_error().decode())
    torch.cuda.synchronize()
    return {f: [1e3 * a.elapsed_time(b) for a, b in pairs[warmup:]] for f, pairs in ev.items()}


def main_sr(args, lib, dev):
    out = {"what": "stochastic rounding against nearest: pack = dpwa_pack, pack_sr = dpwa_pack_stochastic, emit = "
                   "dpwa_average_pack, emit_sr = dpwa_average_pack_stochastic (write-through, peer from a payload or "
                   "from an image); interleaved launch by launch on the same local buffers, Infinity-Cache warm from "
                   "the launch before; dispatch begin/end events; no link is measured",
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "launches": args.launches,
           "repeats": args.repeats, "sizes": {}}
    for name, code, tdtype, n in SIZES:
        entry = {"numel": n}
        for source in ("payload", "image"):
            reps = []
            for _ in range(args.repeats):
                r = {k: stats(v) for k, v in compare_sr(lib, code, tdtype, n, args.launches, args.warmup, dev, source).items()}
                for f in ("pack", "emit"):
                    r[f + "_sr_over_" + f] = round(r[f + "_sr"]["median_us"] / r[f]["median_us"], 3)
                reps.append(r)
                torch.cuda.empty_cache()
            entry["peer_" + source] = reps
        out["sizes"][name] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({nm: {k: [{f: r[f]["median_us"] for f in SR_FORMS} for r in v] for k, v in e.items() if k != "numel"}
                      for nm, e in out["sizes"].items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-blocks", type=int, default=1 << 20, help="of dpwa_unpack (uncapped: the kernel alone)")
    ap.add_argument("--out", default="pack_cost.json")
    ap.add_argument("--avg", action="store_true", help="measure dpwa_average_packed against what it replaces")
    ap.add_argument("--emit", action="store_true", help="measure dpwa_average_pack against what it replaces")
    ap.add_argument("--sr", action="store_true", help="measure the stochastically rounding entries against the nearest")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pack_cost.py needs a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    if args.sr:
        return main_sr(args, lib, dev)
    if args.avg:
        return main_avg(args, lib, dev)
    if args.emit:
        return main_emit(args, lib, dev)
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
