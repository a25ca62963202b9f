#!/usr/bin/env python3
"""Mosaic zone statistics (include/mibayer.h, group `stats`) in HBM: mibayer_stats_device over a device-resident batch,
alternating with the plain demosaic launch of the same context on the same source buffers.  The statistics kernel only
reads (1 or 2 B/px), so its yardsticks are the read-only traffic bound W x H x bytes against the 8 TB/s peak, and the
demosaic launch, which moves 5 or 10 B/px over the same mosaic.

  python tools/stats_bench.py [OUT.json]

Arms: 4K x 64 8-bit and 4K x 16 12-bit LE, each with 1 x 1 and 32 x 32 zones.  Both launches are timed the same way:
`REPS` launches back to back on the context's stream, one mibayer_sync, wall clock / REPS (a statistics call is a
memset of the zones plus the kernel, and has no event-timed entry point); the median of ROUNDS alternating rounds."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160
PEAK = 8.0e12                   # MI355X HBM3E, bytes/s
# (name, frames per launch, output format, deep keywords, mosaic bytes per pixel, demosaic bytes per pixel)
ARMS = (("8bit x64", 64, "BGRx", {}, 1, 5),
        ("12le x16", 16, "ARGB64", {"bits": 12}, 2, 10))
GRIDS = ((1, 1), (32, 32))
ROUNDS = 5
REPS = 40


def timed(ctx, launch):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(REPS):
        launch()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / REPS


def main():
    import __graft_entry__ as entry
    pkg = entry.load_package()
    if pkg.device_count() < 1:
        sys.exit("no HIP device")
    rng = np.random.default_rng(5)
    result = {"geometry": "%dx%d" % (W, H), "peak_bytes_per_s": PEAK, "rounds": ROUNDS, "launches_per_round": REPS,
              "timing": "wall clock over back-to-back launches and one sync", "arms": []}
    for name, n, fmt, deep, src_bpp, dem_bpp in ARMS:
        depth = deep.get("bits", 8)
        vmax = (1 << depth) - 1
        lo, hi = 1, vmax - (vmax >> 4)
        if deep:
            frame = rng.integers(0, 1 << 16, (H, W)).astype("<u2")     # junk above bit 12: masked by the kernel
        else:
            frame = rng.integers(0, 256, (H, W), dtype=np.uint8)
        with pkg.Context(W, H, "bggr", fmt, device=0, **deep) as ctx:
            d_src = ctx.device_alloc(n * ctx.src_bytes)
            d_dst = ctx.device_alloc(n * ctx.dst_bytes)
            d_stats = ctx.device_alloc(n * 32 * 32 * 64)
            try:
                for f in range(n):
                    ctx.to_device(d_src + f * ctx.src_bytes, frame)
                launches = {"demosaic": lambda: ctx.process_device(d_src, d_dst, n)}
                for zx, zy in GRIDS:
                    launches["stats %dx%d" % (zx, zy)] = (
                        lambda zx=zx, zy=zy: ctx.stats_device(d_src, d_stats, zx, zy, lo, hi, n))
                t0 = time.time()
                while time.time() - t0 < 0.3:           # clocks up, caches and TLBs warm
                    for launch in launches.values():
                        launch()
                    ctx.sync()
                runs = {k: [] for k in launches}
                for _ in range(ROUNDS):                 # alternating: every kernel sees the same clocks and neighbours
                    for k, launch in launches.items():
                        runs[k].append(timed(ctx, launch))
            finally:
                for p in (d_src, d_dst, d_stats):
                    ctx.device_free(p)
        arm = {"arm": name, "frames_per_launch": n, "lo": lo, "hi": hi}
        for k, r in runs.items():
            bpp = dem_bpp if k == "demosaic" else src_bpp
            ms = float(np.median(r))
            bw = bpp * W * H * n / (ms * 1e-3)
            arm[k] = {"bytes_per_pixel": bpp, "ms_per_launch_median": round(ms, 4),
                      "ms_per_launch_runs": [round(x, 4) for x in r], "fraction_of_8TBps": round(bw / PEAK, 4)}
            print("%-9s %-12s %2d B/px  %.4f ms / launch  %.0f GB/s  %.1f %% of 8 TB/s" % (
                name, k, bpp, ms, bw / 1e9, 100 * bw / PEAK))
        for zx, zy in GRIDS:
            k = "stats %dx%d" % (zx, zy)
            arm[k]["time_over_demosaic"] = round(arm[k]["ms_per_launch_median"] / arm["demosaic"]["ms_per_launch_median"], 3)
        result["arms"].append(arm)
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
