#!/usr/bin/env python3
"""Lens shading correction (include/mibayer.h, group `shading`) in HBM: mibayer_shade_device over a device-resident
batch, in place and out of place, alternating in one process with the plain demosaic launch of the same context over
the same mosaics.  The pass reads and writes the mosaic (1 or 2 B/px each way), so its yardsticks are the read + write
traffic bound against the 8 TB/s peak and the demosaic launch next to it; then the host path's frame rate with and
without a table.

  python tools/shading_bench.py [OUT.json]

Arms: 4K x 64 8-bit and 4K x 16 12-bit LE, cells of 32 x 32.  Every launch is timed the same way: `REPS` launches back
to back on the context's stream, one mibayer_sync, wall clock / REPS; the median of ROUNDS alternating rounds after a
warm-up.  (In place the mosaic is shaded again and again: the values drift to the clamps, the traffic is the same.)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 3840, 2160
KX = KY = 5
PEAK = 8.0e12                   # MI355X HBM3E, bytes/s
# (name, frames per launch, output format, deep keywords, mosaic bytes per pixel, demosaic bytes per pixel)
ARMS = (("8bit x64", 64, "BGRx", {}, 1, 5),
        ("12le x16", 16, "ARGB64", {"bits": 12}, 2, 10))
ROUNDS = 5
REPS = 20
HOST_FRAMES = 200


def table_for(pkg):
    """a plausible table: gain 1 at the centre rising to 3 in the corners, a little colour shading per site"""
    nx, ny = pkg.shading_nodes(W, H, KX, KY)
    j, i = np.mgrid[0:ny, 0:nx]
    r2 = ((i * 32 - W / 2) ** 2 + (j * 32 - H / 2) ** 2) / float((W / 2) ** 2 + (H / 2) ** 2)
    return np.stack([np.rint(4096 * (1 + (2.0 + 0.1 * s) * r2)) for s in range(4)]).astype(np.uint16)


def timed(ctx, launch):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(REPS):
        launch()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / REPS


def host_fps(ctx, src, dst, frames=HOST_FRAMES):
    """frames per second through mibayer_submit / mibayer_wait from pageable numpy buffers, two in flight"""
    for _ in range(10):
        ctx.process_host(src, dst[0])
    t0 = time.perf_counter()
    queued = 0
    for f in range(frames):
        if queued == 2:
            ctx.wait()
            queued -= 1
        ctx.submit(src, dst[f & 1], tag=f + 1)
        queued += 1
    while queued:
        ctx.wait()
        queued -= 1
    return frames / (time.perf_counter() - t0)


def main():
    import __graft_entry__ as entry
    import shading_model as shm
    pkg = entry.load_package()
    if pkg.device_count() < 1:
        sys.exit("no HIP device")
    rng = np.random.default_rng(5)
    table = table_for(pkg)
    result = {"geometry": "%dx%d" % (W, H), "cells": "%dx%d" % (1 << KX, 1 << KY), "peak_bytes_per_s": PEAK,
              "rounds": ROUNDS, "launches_per_round": REPS, "timing": "wall clock over back-to-back launches and one sync",
              "arms": []}
    for name, n, fmt, deep, src_bpp, dem_bpp in ARMS:
        depth = deep.get("bits", 8)
        black = (1 << depth) // 16
        with pkg.Context(W, H, "bggr", fmt, device=0, **deep) as ctx:
            ctx.set_shading(pkg.Shading(KX, KY, table, (black,) * 4))
            d_src = ctx.device_alloc(n * ctx.src_bytes)
            d_out = ctx.device_alloc(n * ctx.src_bytes)
            d_dst = ctx.device_alloc(n * ctx.dst_bytes)
            try:
                frame = rng.integers(0, 1 << depth, (H, W)).astype("<u2" if deep else np.uint8)
                for f in range(n):
                    ctx.to_device(d_src + f * ctx.src_bytes, frame)
                # the figures are worth something only if the samples are right: one frame against the model
                ctx.shade_device(d_src, d_out, 1)
                ctx.sync()
                got = ctx.from_device(d_out, ctx.src_bytes)
                want = shm.shade_raw(frame, table, KX, KY, (black,) * 4, W, H, ctx.src_stride, deep.get("bits", 0))
                assert np.array_equal(got, want), name
                launches = {"shade out of place": lambda: ctx.shade_device(d_src, d_out, n),
                            "shade in place": lambda: ctx.shade_device(d_out, None, n),
                            "demosaic": lambda: ctx.process_device(d_src, d_dst, n)}
                t0 = time.time()
                while time.time() - t0 < 0.3:           # clocks up, caches and TLBs warm
                    for launch in launches.values():
                        launch()
                    ctx.sync()
                runs = {k: [] for k in launches}
                for _ in range(ROUNDS):                 # alternating: every kernel sees the same clocks and neighbours
                    for k, launch in launches.items():
                        runs[k].append(timed(ctx, launch))
                arm = {"arm": name, "frames_per_launch": n}
                for k, r in runs.items():
                    bpp = dem_bpp if k == "demosaic" else 2 * src_bpp
                    ms = float(np.median(r))
                    bw = bpp * W * H * n / (ms * 1e-3)
                    arm[k] = {"bytes_per_pixel": bpp, "ms_per_launch_median": round(ms, 4),
                              "ms_per_launch_runs": [round(x, 4) for x in r], "fraction_of_8TBps": round(bw / PEAK, 4)}
                    print("%-9s %-19s %2d B/px  %.4f ms / launch  %.0f GB/s  %.1f %% of 8 TB/s" % (
                        name, k, bpp, ms, bw / 1e9, 100 * bw / PEAK), flush=True)
                for k in ("shade out of place", "shade in place"):
                    arm[k]["time_over_demosaic"] = round(arm[k]["ms_per_launch_median"] / arm["demosaic"]["ms_per_launch_median"], 3)
                result["arms"].append(arm)
            finally:
                for p in (d_src, d_out, d_dst):
                    ctx.device_free(p)
    # the host path, 8-bit 4K, two frames in flight: with and without a table, alternating
    with pkg.Context(W, H, "bggr", "BGRx", inflight=2, device=0) as ctx:
        src = rng.integers(0, 256, (H, W), dtype=np.uint8).reshape(-1)
        dst = [np.zeros((H, 4 * W), np.uint8) for _ in range(2)]
        sh = pkg.Shading(KX, KY, table, (16,) * 4)
        fps = {"without": [], "with": []}
        for _ in range(3):
            ctx.set_shading(None)
            fps["without"].append(host_fps(ctx, src, dst))
            ctx.set_shading(sh)
            fps["with"].append(host_fps(ctx, src, dst))
    result["host_path_8bit_fps"] = {k: {"median": round(float(np.median(v)), 1), "runs": [round(x, 1) for x in v]}
                                    for k, v in fps.items()}
    print("host path, 4K 8-bit, pageable buffers, 2 in flight: %.1f fps without, %.1f fps with a table" % (
        float(np.median(fps["without"])), float(np.median(fps["with"]))))
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
