#!/usr/bin/env python3
"""Up to which size the cache-fit policy of the averaging kernel wins bench.py's headline: plain
`bench.py --gpus 1 --numel N` at every size, with DPWA_CACHE_FIT_BYTES=0 (never fit: the product
policy) and a huge DPWA_CACHE_FIT_BYTES (always fit) taking turns, each run a process of its own.
Prints one JSON line per run and a summary per size (the values of either setting, their medians, the
ratio).  kCacheFitBytes (dpwa_amd/csrc/policy.hpp) goes below 3 x the bytes of the first size at which
fit no longer wins.

    python tools/fit_threshold.py [--sizes 5600000,11173962,...] [--passes 2] [--out FILE] [-- bench arguments]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = "5600000,11173962,16800000,22300000,33500000,44700000"
SETTINGS = (("product", "0"), ("fit", str(1 << 60)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=SIZES)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("rest", nargs=argparse.REMAINDER)
    args = ap.parse_args()
    extra = [a for a in args.rest if a != "--"]
    rows, summary = [], []
    for numel in (int(s) for s in args.sizes.split(",")):
        for p in range(args.passes):
            for name, value in (SETTINGS if p % 2 == 0 else SETTINGS[::-1]):
                cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--numel", str(numel)] + extra
                out = subprocess.run(cmd, env=dict(os.environ, DPWA_CACHE_FIT_BYTES=value), cwd=ROOT,
                                     stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
                if out.returncode != 0:
                    print(json.dumps({"numel": numel, "setting": name, "error": out.stderr[-800:]}), flush=True)
                    return 1
                d = json.loads(out.stdout.strip().splitlines()[-1])
                row = {"numel": numel, "bytes_x3": 3 * 4 * numel, "pass": p, "setting": name, "value": d["value"],
                       "ms_per_step": d["ms_per_step"]}
                rows.append(row)
                print(json.dumps(row), flush=True)
        mine = {name: [r["value"] for r in rows if r["numel"] == numel and r["setting"] == name] for name, _ in SETTINGS}
        med = {name: statistics.median(v) for name, v in mine.items()}
        summary.append({"numel": numel, "bytes_x3": 3 * 4 * numel, "product": mine["product"], "fit": mine["fit"],
                        "fit_over_product_median": round(med["fit"] / med["product"], 4),
                        "fit_wins": min(mine["fit"]) > max(mine["product"])})
        print(json.dumps({"summary": summary[-1]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"what": "plain bench.py --gpus 1 --numel N (float32), DPWA_CACHE_FIT_BYTES=0 against a huge one, "
                               "alternately; fit_wins: every fit run above every product run of that size",
                       "rows": rows, "summary": summary}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
