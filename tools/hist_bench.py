#!/usr/bin/env python3
"""Mosaic histogram (include/mibayer.h, group `hist`) in HBM: mibayer_hist_device over a device-resident batch,
alternating in one process, on the same source buffers, with the statistics launch (1 x 1 and 32 x 32 zones) and the
plain demosaic launch of the same context.  The histogram kernel only reads (1 or 2 B/px), so its yardsticks are the
read-only traffic bound W x H x bytes against the 8 TB/s peak, the statistics kernel in the same run, and -- the kernel
spends its time in LDS atomics, whose cost depends on how many lanes of a wave share a bin -- the ratio of its time on
a constant frame to its time on a random one.

  python tools/hist_bench.py [OUT.json]

Arms: 4K x 64 8-bit and 4K x 16 12-bit LE, each over three contents: random, smooth plus noise (a ramp with +-4 of
noise: neighbours share bins often), constant (every sample in one bin).  Every launch is timed the same way: `REPS`
launches back to back on the context's stream, one mibayer_sync, wall clock / REPS (a histogram call is a memset plus
the kernel, and has no event-timed entry point); the median of ROUNDS alternating rounds after a warm-up."""
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
CONTENTS = ("random", "smooth", "constant")
GRIDS = ((1, 1), (32, 32))
ROUNDS = 5
REPS = 20


def content(rng, kind, depth):
    """one (H, W) frame of samples below 2^depth"""
    top = 1 << depth
    if kind == "random":
        return rng.integers(0, top, (H, W))
    if kind == "constant":
        return np.full((H, W), (3 * top) // 4)
    ramp = (np.arange(W)[None, :] * (top - 1) // (W - 1) + np.arange(H)[:, None] * (top // 16) // H) % top
    return np.clip(ramp + rng.integers(-4 * (top >> 8), 4 * (top >> 8) + 1, (H, W)), 0, top - 1)


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
        with pkg.Context(W, H, "bggr", fmt, device=0, **deep) as ctx:
            d_src = ctx.device_alloc(n * ctx.src_bytes)
            d_dst = ctx.device_alloc(n * ctx.dst_bytes)
            d_stats = ctx.device_alloc(n * 32 * 32 * 64)
            d_hist = ctx.device_alloc(n * 4096)
            try:
                for kind in CONTENTS:
                    frame = content(rng, kind, depth).astype("<u2" if deep else np.uint8)
                    for f in range(n):
                        ctx.to_device(d_src + f * ctx.src_bytes, frame)
                    launches = {"hist": lambda: ctx.hist_device(d_src, d_hist, (0, 0, 0, 0), n),
                                "demosaic": lambda: ctx.process_device(d_src, d_dst, n)}
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
                    # the figures are worth something only if the counts are right
                    got = ctx.from_device(d_hist, 4096).view(np.uint32).reshape(4, 256)
                    want = np.stack([np.bincount((frame[s >> 1::2, s & 1::2].astype(np.int64) >> (depth - 8)).reshape(-1),
                                                 minlength=256) for s in range(4)])
                    assert np.array_equal(got, want), (name, kind)
                    arm = {"arm": name, "content": kind, "frames_per_launch": n}
                    for k, r in runs.items():
                        bpp = dem_bpp if k == "demosaic" else src_bpp
                        ms = float(np.median(r))
                        bw = bpp * W * H * n / (ms * 1e-3)
                        arm[k] = {"bytes_per_pixel": bpp, "ms_per_launch_median": round(ms, 4),
                                  "ms_per_launch_runs": [round(x, 4) for x in r], "fraction_of_8TBps": round(bw / PEAK, 4)}
                        print("%-9s %-9s %-12s %2d B/px  %.4f ms / launch  %.0f GB/s  %.1f %% of 8 TB/s" % (
                            name, kind, k, bpp, ms, bw / 1e9, 100 * bw / PEAK), flush=True)
                    for k in ("stats 1x1", "stats 32x32", "demosaic"):
                        arm["hist"]["time_over_" + k.replace(" ", "_")] = round(
                            arm["hist"]["ms_per_launch_median"] / arm[k]["ms_per_launch_median"], 3)
                    result["arms"].append(arm)
            finally:
                for p in (d_src, d_dst, d_stats, d_hist):
                    ctx.device_free(p)
        per = {a["content"]: a["hist"]["ms_per_launch_median"] for a in result["arms"] if a["arm"] == name}
        result.setdefault("constant_over_random", {})[name] = round(per["constant"] / per["random"], 3)
    # one frame per launch, 8-bit: the grid the host path gets
    with pkg.Context(W, H, "bggr", "BGRx", device=0) as ctx:
        d_src, d_hist = ctx.device_alloc(ctx.src_bytes), ctx.device_alloc(4096)
        try:
            ctx.to_device(d_src, rng.integers(0, 256, (H, W), dtype=np.uint8))
            one = lambda: ctx.hist_device(d_src, d_hist)  # noqa: E731
            for _ in range(200):
                one()
            r = [timed(ctx, one) for _ in range(ROUNDS)]
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_hist)
    result["one_frame_8bit_random_ms_per_launch"] = {"median": round(float(np.median(r)), 4), "runs": [round(x, 4) for x in r]}
    print("one 4K frame per launch: %.4f ms (memset + kernel, back to back)" % float(np.median(r)))
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
