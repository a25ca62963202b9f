#!/usr/bin/env python3
"""Half-size demosaic (include/mibayer.h, group `half`) in HBM: mibayer_process_device of a HALF context over a
device-resident batch, alternating in one process, on the same source buffers, with the full-resolution bilinear launch
of the same cfg without the flag.  The kernel is pointwise: its bound is the bytes it must move -- the mosaic read once
plus the quarter-size frame written once -- against the 8 TB/s peak; the full-resolution launch is measured against its
own bytes the same way.

  python tools/half_bench.py [OUT.json]

Arms: 4K x 64 8-bit and 4K x 16 12-bit LE of random samples, each to BGRx, ARGB64, RGB and GBR planes.  Every launch is
timed the same way: `REPS` launches back to back on the context's stream, one mibayer_sync, wall clock / REPS; the median
of ROUNDS alternating rounds after a warm-up.  The first frame of every arm, half and full, is compared with the models
(tests/half_model.py; tests/rgb24_model.py, tests/planar_model.py, tests/highbit_model.py) before anything is timed.
Then the host path: 4K 8-bit -> BGRx frames/s from pageable buffers, two in flight, a half and a full context in
alternating rounds."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 3840, 2160
OW, OH = W // 2, H // 2
PEAK = 8.0e12                   # MI355X HBM3E, bytes/s
# (name, frames per launch, deep keywords, mosaic bytes per sample)
SAMPLES = (("8bit x64", 64, {}, 1), ("12le x16", 16, {"bits": 12}, 2))
# (output format, bytes written per output pixel)
OUTPUTS = (("BGRx", 4), ("ARGB64", 8), ("RGB", 3), ("GBR", 3))
ROUNDS = 5
REPS = 20
HOST_FRAMES = 200
HOST_ROUNDS = 3


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


def host_path(pkg, rng):
    """4K 8-bit -> BGRx, two frames in flight: a full-resolution and a half-size context, alternating"""
    src = rng.integers(0, 256, (H, W), dtype=np.uint8).reshape(-1)
    fps = {"full": [], "half": []}
    with pkg.Context(W, H, "bggr", "BGRx", inflight=2, device=0) as full, \
            pkg.Context(W, H, "bggr", "BGRx", inflight=2, method="half", device=0) as half:
        dst = {"full": [np.zeros((H, 4 * W), np.uint8) for _ in range(2)],
               "half": [np.zeros((OH, 4 * OW), np.uint8) for _ in range(2)]}
        for _ in range(HOST_ROUNDS):
            fps["full"].append(host_fps(full, src, dst["full"]))
            fps["half"].append(host_fps(half, src, dst["half"]))
    out = {k: {"median": round(float(np.median(v)), 1), "runs": [round(x, 1) for x in v]} for k, v in fps.items()}
    out["half_over_full"] = round(out["half"]["median"] / out["full"]["median"], 3)
    return out


def full_model(frame, fmt, bits):
    """the full-resolution frame of the existing models, (rows, row bytes)"""
    import highbit_model as hm
    import planar_model as pm
    import rgb24_model as rm
    if fmt in pm.FORMATS:
        return pm.bayer2rgb_planar(frame, W, H, "bggr", fmt, bits=bits).reshape(3 * H, -1)
    if fmt in rm.FOUR_BYTE:
        return rm.bayer2rgb_rgb24(frame, W, H, "bggr", fmt, bits=bits)
    if fmt.endswith("64") or bits:
        return hm.bayer2rgb_highbit(frame, W, H, "bggr", fmt, bits or 8, fmt.endswith("64"))
    return rm.four_byte(frame, W, H, "bggr", "RGB" if fmt == "RGBx" else "BGR", bits)


def main():
    import __graft_entry__ as entry
    import half_model as hf
    pkg = entry.load_package()
    if pkg.device_count() < 1:
        sys.exit("no HIP device")
    rng = np.random.default_rng(5)
    result = {"geometry": "%dx%d -> %dx%d" % (W, H, OW, OH), "peak_bytes_per_s": PEAK, "rounds": ROUNDS,
              "launches_per_round": REPS, "timing": "wall clock over back-to-back launches and one sync", "arms": []}
    for name, n, deep, src_bps in SAMPLES:
        bits = deep.get("bits", 0)
        vmax = (1 << (bits or 8)) - 1
        frame = rng.integers(0, vmax + 1, (H, W)).astype("<u2" if bits else np.uint8)
        frame_bytes = np.ascontiguousarray(frame).view(np.uint8).reshape(H, -1)
        for fmt, px in OUTPUTS:
            with pkg.Context(W, H, "bggr", fmt, device=0, method="half", **deep) as half, \
                    pkg.Context(W, H, "bggr", fmt, device=0, **deep) as full:
                d_src = half.device_alloc(n * half.src_bytes)
                d_half = half.device_alloc(n * half.dst_bytes)
                d_full = full.device_alloc(n * full.dst_bytes)
                try:
                    for f in range(n):
                        half.to_device(d_src + f * half.src_bytes, frame_bytes)
                    launches = {"half": (half, lambda: half.process_device(d_src, d_half, n)),
                                "full": (full, lambda: full.process_device(d_src, d_full, n))}
                    # the figures are worth something only if the frames are right: the first frame of each arm
                    for ctx, launch in launches.values():
                        launch()
                        ctx.sync()
                    got = half.from_device(d_half, half.dst_bytes).reshape(half.dst_rows, half.dst_stride)
                    assert np.array_equal(got, hf.frame(frame_bytes, W, H, "bggr", fmt, bits=bits)), (name, fmt, "half")
                    got = full.from_device(d_full, full.dst_bytes).reshape(full.dst_rows, full.dst_stride)
                    assert np.array_equal(got, full_model(frame_bytes, fmt, bits)), (name, fmt, "full")
                    t0 = time.time()
                    while time.time() - t0 < 0.3:       # clocks up, caches and TLBs warm
                        for ctx, launch in launches.values():
                            launch()
                            ctx.sync()
                    runs = {k: [] for k in launches}
                    for _ in range(ROUNDS):             # alternating: both kernels see the same clocks and neighbours
                        for k, (ctx, launch) in launches.items():
                            runs[k].append(timed(ctx, launch))
                    arm = {"arm": name, "output": fmt, "frames_per_launch": n,
                           "kernels": {"half": half.variant_name, "full": full.variant_name}}
                    for k, r in runs.items():
                        pixels = OW * OH if k == "half" else W * H
                        moved = (src_bps * W * H + px * pixels) * n
                        ms = float(np.median(r))
                        bw = moved / (ms * 1e-3)
                        arm[k] = {"bytes_per_launch": moved, "ms_per_launch_median": round(ms, 4),
                                  "ms_per_launch_runs": [round(x, 4) for x in r], "fraction_of_8TBps": round(bw / PEAK, 4)}
                        print("%-9s %-7s %-5s %.4f ms / launch  %.0f GB/s  %.1f %% of 8 TB/s" % (
                            name, fmt, k, ms, bw / 1e9, 100 * bw / PEAK), flush=True)
                    arm["half_over_full_time"] = round(arm["half"]["ms_per_launch_median"]
                                                       / arm["full"]["ms_per_launch_median"], 3)
                    result["arms"].append(arm)
                finally:
                    half.device_free(d_src)
                    half.device_free(d_half)
                    full.device_free(d_full)
    result["host_path_8bit_bgrx_fps"] = host_path(pkg, rng)
    fps = result["host_path_8bit_bgrx_fps"]
    print("host path, 4K 8-bit -> BGRx, pageable buffers, 2 in flight: %.1f fps full, %.1f fps half (x %.2f)" % (
        fps["full"]["median"], fps["half"]["median"], fps["half_over_full"]))
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
