#!/usr/bin/env python3
"""Noise reduction (include/mibayer.h, group `nr`) in HBM: mibayer_nr_device over a device-resident batch, alternating
in one process with the defect pass and the lens shading pass (out of place) over the same mosaics.  The pass reads the
mosaic once and writes it once (1 or 2 B/px each way), so its yardsticks are that traffic bound against the 8 TB/s peak
and the two other mosaic passes next to it; then the host path's frame rate with the curve off and on.

  python tools/nr_bench.py [OUT.json]
  python tools/nr_bench.py --host LIBMIBAYER.so     one process, the host path only, over the library given: one JSON line

Arms: 4K x 64 8-bit and 4K x 16 12-bit LE; the noisy ramp of tests/nr_cases.py (uniform noise of +-A on a ramp with a
per-site offset, a constant curve of about 2 A / 3).  Every launch is timed the same way: `REPS` launches back to back on
the context's stream, one mibayer_sync, wall clock / REPS; the median of ROUNDS alternating rounds after a warm-up.  The
first and the last 256 rows of the first frame of every arm are compared with the model (tests/nr_model.py) before
anything is timed.  --host: frames/s with the curve off, then -- where the library has one -- on; run it in alternating
fresh processes over two libraries to compare them."""
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
# (name, frames per launch, output format, deep keywords, mosaic bytes per pixel)
ARMS = (("8bit x64", 64, "BGRx", {}, 1),
        ("12le x16", 16, "ARGB64", {"bits": 12}, 2))
ROUNDS = 5
REPS = 20
HOST_FRAMES = 200
CHECK_ROWS = 256


def scene(rng, depth):
    """the frame of tests/nr_cases.py at 4K: a diagonal ramp, a per-site offset, uniform noise of +-A"""
    import nr_cases as nc
    vmax = (1 << depth) - 1
    amp, t = nc.NOISE[depth]
    y, x = np.mgrid[0:H, 0:W]
    S = vmax // 4 + (x + 2 * y) * (vmax // 4) // (W + 2 * H) + (vmax // 16) * (2 * (y & 1) + (x & 1))
    return S + rng.integers(-amp, amp + 1, S.shape), [t] * 17


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
    """4K 8-bit -> BGRx, two frames in flight: curve off and (where the library has one) on, alternating"""
    has_nr = hasattr(pkg.lib(), "mibayer_set_nr")
    with pkg.Context(W, H, "bggr", "BGRx", inflight=2, device=0) as ctx:
        S, curve = scene(rng, 8)
        src = S.astype(np.uint8).reshape(-1)
        dst = [np.zeros((H, 4 * W), np.uint8) for _ in range(2)]
        fps = {"off": [], "on": []}
        for _ in range(rounds):
            if has_nr:
                ctx.set_nr(None)
            fps["off"].append(host_fps(ctx, src, dst))
            if has_nr:
                ctx.set_nr(pkg.Nr(curve))
                fps["on"].append(host_fps(ctx, src, dst))
    return {k: {"median": round(float(np.median(v)), 1), "runs": [round(x, 1) for x in v]} for k, v in fps.items() if v}


def main():
    import __graft_entry__ as entry
    import nr_model as nm
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
    nx, ny = pkg.shading_nodes(W, H, KX, KY)
    table = np.full((4, ny, nx), 5000, np.uint16)
    result = {"geometry": "%dx%d" % (W, H), "peak_bytes_per_s": PEAK, "rounds": ROUNDS, "launches_per_round": REPS,
              "timing": "wall clock over back-to-back launches and one sync", "arms": []}
    for name, n, fmt, deep, src_bpp in ARMS:
        depth = deep.get("bits", 8)
        with pkg.Context(W, H, "bggr", fmt, device=0, **deep) as ctx:
            S, curve = scene(rng, depth)
            t = (1 << depth) // 16
            ctx.set_nr(pkg.Nr(curve))
            ctx.set_dpc(pkg.Dpc(t, t, None))
            ctx.set_shading(pkg.Shading(KX, KY, table, (t,) * 4))
            d_src = ctx.device_alloc(n * ctx.src_bytes)
            d_out = ctx.device_alloc(n * ctx.src_bytes)
            try:
                frame = S.astype("<u2" if deep else np.uint8)
                for f in range(n):
                    ctx.to_device(d_src + f * ctx.src_bytes, frame)
                # the figures are worth something only if the samples are right: the first and the last rows of one
                # frame against the model (the rows a crop of CHECK_ROWS + 8 rows decides)
                ctx.nr_device(d_src, d_out, 1)
                ctx.sync()
                got = ctx.from_device(d_out, ctx.src_bytes).view("<u2" if deep else np.uint8).reshape(H, W)
                top = nm.denoise(S[:CHECK_ROWS + 8], curve, depth)[:CHECK_ROWS]
                bottom = nm.denoise(S[-CHECK_ROWS - 8:], curve, depth)[-CHECK_ROWS:]
                assert np.array_equal(got[:CHECK_ROWS], top) and np.array_equal(got[-CHECK_ROWS:], bottom), name
                changed = float((top != S[:CHECK_ROWS]).mean())
                share = float(nm.included(S[:CHECK_ROWS + 8], curve, depth)[:, :CHECK_ROWS].mean())
                launches = {"nr": lambda: ctx.nr_device(d_src, d_out, n),
                            "dpc": lambda: ctx.dpc_device(d_src, d_out, n),
                            "shade out of place": lambda: ctx.shade_device(d_src, d_out, n)}
                t0 = time.time()
                while time.time() - t0 < 0.3:           # clocks up, caches and TLBs warm
                    for launch in launches.values():
                        launch()
                    ctx.sync()
                runs = {k: [] for k in launches}
                for _ in range(ROUNDS):                 # alternating: every kernel sees the same clocks and neighbours
                    for k, launch in launches.items():
                        runs[k].append(timed(ctx, launch))
                arm = {"arm": name, "frames_per_launch": n, "share_of_samples_changed": round(changed, 4),
                       "share_of_neighbours_included": round(share, 4)}
                for k, r in runs.items():
                    bpp = 2 * src_bpp
                    ms = float(np.median(r))
                    bw = bpp * W * H * n / (ms * 1e-3)
                    arm[k] = {"bytes_per_pixel": bpp, "ms_per_launch_median": round(ms, 4),
                              "ms_per_launch_runs": [round(x, 4) for x in r], "fraction_of_8TBps": round(bw / PEAK, 4)}
                    print("%-9s %-19s %2d B/px  %.4f ms / launch  %.0f GB/s  %.1f %% of 8 TB/s" % (
                        name, k, bpp, ms, bw / 1e9, 100 * bw / PEAK), flush=True)
                for other in ("dpc", "shade out of place"):
                    arm["nr"]["time_over_" + other.split()[0]] = round(
                        arm["nr"]["ms_per_launch_median"] / arm[other]["ms_per_launch_median"], 3)
                result["arms"].append(arm)
            finally:
                for p in (d_src, d_out):
                    ctx.device_free(p)
    result["host_path_8bit_fps"] = host_path(pkg, rng, 3)
    fps = result["host_path_8bit_fps"]
    print("host path, 4K 8-bit, pageable buffers, 2 in flight: %.1f fps with the curve off, %.1f fps with it on" % (
        fps["off"]["median"], fps["on"]["median"]))
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
