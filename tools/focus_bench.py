#!/usr/bin/env python3
"""Mosaic focus statistics (include/mibayer.h, group `focus`) in HBM: mibayer_focus_device over a device-resident batch,
alternating in one process, on the same source buffers, with the statistics launch (1 x 1 zones), the defect pass and
the plain demosaic launch of the same context.  The focus kernel only reads (1 or 2 B/px), so its yardsticks are the
read-only traffic bound W x H x bytes against the 8 TB/s peak, and the statistics kernel and the defect pass over the
same mosaics: it reads what they read, plus four halo rows per segment of 64.

  python tools/focus_bench.py [OUT.json]
  python tools/focus_bench.py --host LIBMIBAYER.so     one process, the host path only, over the library given: one JSON line

Arms: 4K x 64 8-bit and 4K x 16 12-bit LE of random samples; focus at 1 x 1 and 32 x 32 zones with a threshold of a
quarter of the range.  Every launch is timed the same way: `REPS` launches back to back on the context's stream, one
mibayer_sync, wall clock / REPS (a focus call is a memset plus the kernel); the median of ROUNDS alternating rounds after
a warm-up.  The zones of the first frame of each focus arm are compared with the model (tests/focus_model.py) in the
run.  --host: 4K 8-bit -> BGRx frames/s, two in flight, with focus off, then -- where the library has it -- on; run it in
alternating fresh processes over two libraries to compare them."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 3840, 2160
PEAK = 8.0e12                   # MI355X HBM3E, bytes/s
# (name, frames per launch, output format, deep keywords, mosaic bytes per pixel, demosaic bytes per pixel)
ARMS = (("8bit x64", 64, "BGRx", {}, 1, 5),
        ("12le x16", 16, "ARGB64", {"bits": 12}, 2, 10))
GRIDS = ((1, 1), (32, 32))
ROUNDS = 5
REPS = 20
HOST_FRAMES = 200


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


def host_path(pkg, rng, rounds):
    """4K 8-bit -> BGRx, two frames in flight: focus off and (where the library has it) on at 32 x 32, alternating"""
    has_focus = hasattr(pkg.lib(), "mibayer_set_focus")
    with pkg.Context(W, H, "bggr", "BGRx", inflight=2, device=0) as ctx:
        src = rng.integers(0, 256, (H, W), dtype=np.uint8).reshape(-1)
        dst = [np.zeros((H, 4 * W), np.uint8) for _ in range(2)]
        fps = {"off": [], "on": []}
        for _ in range(rounds):
            if has_focus:
                ctx.set_focus(0, 0)
            fps["off"].append(host_fps(ctx, src, dst))
            if has_focus:
                ctx.set_focus(32, 32, 64)
                fps["on"].append(host_fps(ctx, src, dst))
    return {k: {"median": round(float(np.median(v)), 1), "runs": [round(x, 1) for x in v]} for k, v in fps.items() if v}


def main():
    import __graft_entry__ as entry
    import focus_model as fm
    pkg = entry.load_package()
    if len(sys.argv) > 2 and sys.argv[1] == "--host":
        pkg.LIB_PATH = os.path.abspath(sys.argv[2])     # lib() is lazy: nothing has been loaded yet
        import ctypes
        probe = ctypes.CDLL(pkg.LIB_PATH)
        for name in [n for n in pkg.ABI if not hasattr(probe, n)]:
            del pkg.ABI[name]           # a library from before the group: the harness binds what it has
        print(json.dumps({"lib": sys.argv[2], "host_path_8bit_fps": host_path(pkg, np.random.default_rng(5), 2)}))
        return
    if pkg.device_count() < 1:
        sys.exit("no HIP device")
    rng = np.random.default_rng(5)
    result = {"geometry": "%dx%d" % (W, H), "peak_bytes_per_s": PEAK, "rounds": ROUNDS, "launches_per_round": REPS,
              "timing": "wall clock over back-to-back launches and one sync", "arms": []}
    for name, n, fmt, deep, src_bpp, dem_bpp in ARMS:
        depth = deep.get("bits", 8)
        vmax = (1 << depth) - 1
        thr = vmax // 4
        with pkg.Context(W, H, "bggr", fmt, device=0, **deep) as ctx:
            ctx.set_dpc(pkg.Dpc(vmax // 16, vmax // 16, None))
            d_src = ctx.device_alloc(n * ctx.src_bytes)
            d_out = ctx.device_alloc(n * ctx.src_bytes)
            d_dst = ctx.device_alloc(n * ctx.dst_bytes)
            d_stats = ctx.device_alloc(n * 64)
            d_focus = ctx.device_alloc(n * 32 * 32 * 96)
            try:
                S = rng.integers(0, vmax + 1, (H, W))
                frame = S.astype("<u2" if deep else np.uint8)
                for f in range(n):
                    ctx.to_device(d_src + f * ctx.src_bytes, frame)
                launches = {"stats 1x1": lambda: ctx.stats_device(d_src, d_stats, 1, 1, 1, vmax - 1, n),
                            "dpc": lambda: ctx.dpc_device(d_src, d_out, n),
                            "demosaic": lambda: ctx.process_device(d_src, d_dst, n)}
                for zx, zy in GRIDS:
                    launches["focus %dx%d" % (zx, zy)] = (
                        lambda zx=zx, zy=zy: ctx.focus_device(d_src, d_focus, zx, zy, thr, n))
                # the figures are worth something only if the zones are right: the first frame of each focus arm
                for zx, zy in GRIDS:
                    launches["focus %dx%d" % (zx, zy)]()
                    ctx.sync()
                    got = ctx.from_device(d_focus, zx * zy * 96).view(fm.FOCUS_DTYPE).reshape(zy, zx)
                    assert got.tobytes() == fm.zone_focus(S, zx, zy, thr, vmax).tobytes(), (name, zx, zy)
                t0 = time.time()
                while time.time() - t0 < 0.3:           # clocks up, caches and TLBs warm
                    for launch in launches.values():
                        launch()
                    ctx.sync()
                runs = {k: [] for k in launches}
                for _ in range(ROUNDS):                 # alternating: every kernel sees the same clocks and neighbours
                    for k, launch in launches.items():
                        runs[k].append(timed(ctx, launch))
                arm = {"arm": name, "frames_per_launch": n, "threshold": thr}
                for k, r in runs.items():
                    bpp = dem_bpp if k == "demosaic" else 2 * src_bpp if k == "dpc" else src_bpp
                    ms = float(np.median(r))
                    bw = bpp * W * H * n / (ms * 1e-3)
                    arm[k] = {"bytes_per_pixel": bpp, "ms_per_launch_median": round(ms, 4),
                              "ms_per_launch_runs": [round(x, 4) for x in r], "fraction_of_8TBps": round(bw / PEAK, 4)}
                    print("%-9s %-12s %2d B/px  %.4f ms / launch  %.0f GB/s  %.1f %% of 8 TB/s" % (
                        name, k, bpp, ms, bw / 1e9, 100 * bw / PEAK), flush=True)
                for grid in ("focus 1x1", "focus 32x32"):
                    for other in ("stats 1x1", "dpc", "demosaic"):
                        arm[grid]["time_over_" + other.replace(" ", "_")] = round(
                            arm[grid]["ms_per_launch_median"] / arm[other]["ms_per_launch_median"], 3)
                result["arms"].append(arm)
            finally:
                for p in (d_src, d_out, d_dst, d_stats, d_focus):
                    ctx.device_free(p)
    result["host_path_8bit_fps"] = host_path(pkg, rng, 3)
    fps = result["host_path_8bit_fps"]
    print("host path, 4K 8-bit, pageable buffers, 2 in flight: %.1f fps with focus off, %.1f fps with it on (32 x 32)" % (
        fps["off"]["median"], fps["on"]["median"]))
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
