#!/usr/bin/env python3
"""Defective pixel correction (include/mibayer.h, group `dpc`) in HBM: mibayer_dpc_device over a device-resident batch,
alternating in one process with the lens shading pass (out of place) and the plain demosaic launch of the same context
over the same mosaics.  The pass reads the mosaic once and writes it once (1 or 2 B/px each way), so its yardsticks are
that traffic bound against the 8 TB/s peak and the shading pass next to it; then the host path's frame rate with the
correction on and off.

  python tools/dpc_bench.py [OUT.json]

Arms: 4K x 64 8-bit and 4K x 16 12-bit LE; thresholds of 1/16 of the range on a noisy ramp with 0.1 % stuck samples
(a few hundred per frame also in the list).  Every launch is timed the same way: `REPS` launches back to back on the
context's stream, one mibayer_sync, wall clock / REPS; the median of ROUNDS alternating rounds after a warm-up.  The
first frame of every arm is compared with the model (tests/dpc_model.py) before anything is timed."""
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


def scene(rng, depth):
    """a ramp with sensor noise, per-site levels and one sample in a thousand stuck at 0 or max; the first 300 stuck
    samples are the list"""
    vmax = (1 << depth) - 1
    y, x = np.mgrid[0:H, 0:W]
    S = vmax // 8 + (x * (vmax // 2)) // W + (y * (vmax // 8)) // H + (vmax // 32) * (2 * (y & 1) + (x & 1))
    S = np.clip(S + rng.normal(0, vmax / 256.0, S.shape).astype(np.int64), 0, vmax)
    stuck = rng.random(S.shape) < 1e-3
    S[stuck] = rng.choice([0, vmax], int(stuck.sum()))
    return S, np.argwhere(stuck)[:300, ::-1].astype(np.uint32)


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
    import dpc_model as dm
    pkg = entry.load_package()
    if pkg.device_count() < 1:
        sys.exit("no HIP device")
    rng = np.random.default_rng(5)
    nx, ny = pkg.shading_nodes(W, H, KX, KY)
    table = np.full((4, ny, nx), 5000, np.uint16)
    result = {"geometry": "%dx%d" % (W, H), "peak_bytes_per_s": PEAK, "rounds": ROUNDS, "launches_per_round": REPS,
              "timing": "wall clock over back-to-back launches and one sync", "arms": []}
    for name, n, fmt, deep, src_bpp, dem_bpp in ARMS:
        depth = deep.get("bits", 8)
        t = (1 << depth) // 16
        with pkg.Context(W, H, "bggr", fmt, device=0, **deep) as ctx:
            S, lst = scene(rng, depth)
            ctx.set_dpc(pkg.Dpc(t, t, lst))
            ctx.set_shading(pkg.Shading(KX, KY, table, (t,) * 4))
            d_src = ctx.device_alloc(n * ctx.src_bytes)
            d_out = ctx.device_alloc(n * ctx.src_bytes)
            d_dst = ctx.device_alloc(n * ctx.dst_bytes)
            try:
                frame = S.astype("<u2" if deep else np.uint8)
                for f in range(n):
                    ctx.to_device(d_src + f * ctx.src_bytes, frame)
                # the figures are worth something only if the samples are right: one frame against the model
                ctx.dpc_device(d_src, d_out, 1)
                ctx.sync()
                got = ctx.from_device(d_out, ctx.src_bytes)
                raw = frame.view(np.uint8).reshape(-1)
                want = dm.correct_raw(raw, raw, W, H, ctx.src_stride, deep.get("bits", 0), False, t, t, lst)
                assert np.array_equal(got, want), name
                changed = int((dm.correct(S, t, t, lst) != S).sum())
                launches = {"dpc": lambda: ctx.dpc_device(d_src, d_out, n),
                            "shade out of place": lambda: ctx.shade_device(d_src, d_out, n),
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
                arm = {"arm": name, "frames_per_launch": n, "samples_corrected_per_frame": changed}
                for k, r in runs.items():
                    bpp = dem_bpp if k == "demosaic" else 2 * src_bpp
                    ms = float(np.median(r))
                    bw = bpp * W * H * n / (ms * 1e-3)
                    arm[k] = {"bytes_per_pixel": bpp, "ms_per_launch_median": round(ms, 4),
                              "ms_per_launch_runs": [round(x, 4) for x in r], "fraction_of_8TBps": round(bw / PEAK, 4)}
                    print("%-9s %-19s %2d B/px  %.4f ms / launch  %.0f GB/s  %.1f %% of 8 TB/s" % (
                        name, k, bpp, ms, bw / 1e9, 100 * bw / PEAK), flush=True)
                for other in ("shade out of place", "demosaic"):
                    arm["dpc"]["time_over_" + other.split()[0]] = round(
                        arm["dpc"]["ms_per_launch_median"] / arm[other]["ms_per_launch_median"], 3)
                result["arms"].append(arm)
            finally:
                for p in (d_src, d_out, d_dst):
                    ctx.device_free(p)
    # the host path, 8-bit 4K, two frames in flight: correction off and on, alternating
    with pkg.Context(W, H, "bggr", "BGRx", inflight=2, device=0) as ctx:
        S, lst = scene(rng, 8)
        src = S.astype(np.uint8).reshape(-1)
        dst = [np.zeros((H, 4 * W), np.uint8) for _ in range(2)]
        fps = {"off": [], "on": []}
        for _ in range(3):
            ctx.set_dpc(None)
            fps["off"].append(host_fps(ctx, src, dst))
            ctx.set_dpc(pkg.Dpc(16, 16, lst))
            fps["on"].append(host_fps(ctx, src, dst))
    result["host_path_8bit_fps"] = {k: {"median": round(float(np.median(v)), 1), "runs": [round(x, 1) for x in v]}
                                    for k, v in fps.items()}
    print("host path, 4K 8-bit, pageable buffers, 2 in flight: %.1f fps with the correction off, %.1f fps with it on" % (
        float(np.median(fps["off"])), float(np.median(fps["on"]))))
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
