#!/usr/bin/env python3
"""Malvar-He-Cutler kernel (include/mibayer.h, MIBAYER_FLAG_MHC) against the bilinear kernels in HBM: the same
device-resident batch converted by an MHC context and by a bilinear one, timed alternately in one process with HIP
events on each context's stream (mibayer_time_device).

  python tools/mhc_bench.py [OUT.json]     three arms, MHC and bilinear each; prints the fraction of 8 TB/s
  python tools/mhc_bench.py trace          a few launches of every arm, for rocprofv3 --kernel-trace --stats

Arms: 4K x 64 8-bit -> BGRx (1 B read + 4 B written per pixel), 4K x 16 12-bit LE -> ARGB64 (2 + 8 B), and one 4K
8-bit frame per launch (launch-latency-bound; the bilinear side runs its one-frame plan)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160
PEAK = 8.0e12                   # MI355X HBM3E, bytes/s
# (name, frames per launch, output format, deep keywords, bytes per pixel)
ARMS = (("8bit->BGRx x64", 64, "BGRx", {}, 5),
        ("12le->ARGB64 x16", 16, "ARGB64", {"bits": 12}, 10),
        ("8bit->BGRx x1", 1, "BGRx", {}, 5))
ROUNDS = 5


def main():
    import __graft_entry__ as entry
    pkg = entry.load_package()
    if pkg.device_count() < 1:
        sys.exit("no HIP device")
    trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
    rng = np.random.default_rng(5)
    result = {"geometry": "%dx%d" % (W, H), "peak_bytes_per_s": PEAK, "rounds": ROUNDS, "arms": []}
    for name, n, fmt, deep, bpp in ARMS:
        if deep:
            frame = rng.integers(0, 1 << 16, (H, W)).astype("<u2")     # junk above bit 12: masked by the kernel
        else:
            frame = rng.integers(0, 256, (H, W), dtype=np.uint8)
        ctxs = {m: pkg.Context(W, H, "bggr", fmt, device=0, method=m, **deep) for m in ("bilinear", "mhc")}
        bufs = {}
        try:
            for m, ctx in ctxs.items():
                d_src = ctx.device_alloc(n * ctx.src_bytes)
                d_dst = ctx.device_alloc(n * ctx.dst_bytes)
                bufs[m] = (d_src, d_dst)
                for f in range(n):
                    ctx.to_device(d_src + f * ctx.src_bytes, frame)
            if trace:
                for m, ctx in ctxs.items():
                    for _ in range(20):
                        ctx.process_device(*bufs[m], n)
                    ctx.sync()
                continue
            for m, ctx in ctxs.items():
                t0 = time.time()
                while time.time() - t0 < 0.2:           # clocks up, caches and TLBs warm
                    ctx.process_device(*bufs[m], n)
                    ctx.sync()
            runs = {m: [] for m in ctxs}
            for _ in range(ROUNDS):                     # alternating: both kernels see the same clocks and neighbours
                for m, ctx in ctxs.items():
                    runs[m].append(ctx.time_device(*bufs[m], n, warmup=3, reps=30 if n > 1 else 200))
            names = {m: ctx.variant_name for m, ctx in ctxs.items()}
        finally:
            for m, ctx in ctxs.items():
                for d in bufs.get(m, ()):
                    ctx.device_free(d)
                ctx.close()
        arm = {"arm": name, "frames_per_launch": n, "bytes_per_pixel": bpp}
        for m in ("mhc", "bilinear"):
            ms = float(np.median(runs[m]))
            bw = bpp * W * H * n / (ms * 1e-3)
            arm[m] = {"kernel": names[m], "ms_per_launch_median": round(ms, 4),
                      "ms_per_launch_runs": [round(r, 4) for r in runs[m]],
                      "fraction_of_8TBps": round(bw / PEAK, 4), "gpix_per_s": round(W * H * n / (ms * 1e-3) / 1e9, 1)}
            print("%-17s %-8s %2d B/px  %.4f ms / launch  %.0f GB/s  %.1f %% of 8 TB/s" % (
                name, m, bpp, ms, bw / 1e9, 100 * bw / PEAK))
        arm["mhc_over_bilinear_time"] = round(arm["mhc"]["ms_per_launch_median"]
                                              / arm["bilinear"]["ms_per_launch_median"], 3)
        result["arms"].append(arm)
    if not trace:
        line = json.dumps(result)
        print(line)
        if len(sys.argv) > 1:
            with open(sys.argv[1], "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
