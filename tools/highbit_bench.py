#!/usr/bin/env python3
"""Deep-sample kernel (include/mibayer.h, MIBAYER_FLAG_SRC_BITS) in HBM: mibayer_process_device over a 16-frame 4K
batch, device-resident, timed with HIP events on the context's stream (mibayer_time_device).

  python tools/highbit_bench.py [OUT.json]     12-bit LE -> ARGB64 (2 B read + 8 B written per pixel) and
                                               12-bit LE -> BGRx (2 + 4 B); prints the fraction of 8 TB/s
  python tools/highbit_bench.py trace          a few launches of both arms, for rocprofv3 --kernel-trace --stats

The input is random 12-bit samples with junk in the 4 bits above them (the kernel masks them)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N = 3840, 2160, 16
PEAK = 8.0e12                   # MI355X HBM3E, bytes/s
ARMS = (("12le->ARGB64", "ARGB64", 10), ("12le->BGRx", "BGRx", 6))


def main():
    import __graft_entry__ as entry
    pkg = entry.load_package()
    if pkg.device_count() < 1:
        sys.exit("no HIP device")
    trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
    rng = np.random.default_rng(12)
    frame = rng.integers(0, 1 << 16, (H, W)).astype("<u2")
    result = {"geometry": "%dx%d" % (W, H), "frames_per_launch": N, "peak_bytes_per_s": PEAK, "arms": []}
    for name, fmt, bpp in ARMS:
        with pkg.Context(W, H, "bggr", fmt, bits=12, device=0) as ctx:
            d_src = ctx.device_alloc(N * ctx.src_bytes)
            d_dst = ctx.device_alloc(N * ctx.dst_bytes)
            try:
                for f in range(N):
                    ctx.to_device(d_src + f * ctx.src_bytes, frame)
                if trace:
                    for _ in range(20):
                        ctx.process_device(d_src, d_dst, N)
                    ctx.sync()
                    continue
                t0 = time.time()
                while time.time() - t0 < 0.2:           # clocks up, caches and TLBs warm
                    ctx.process_device(d_src, d_dst, N)
                    ctx.sync()
                runs = [ctx.time_device(d_src, d_dst, N, warmup=3, reps=30) for _ in range(5)]
            finally:
                ctx.device_free(d_src)
                ctx.device_free(d_dst)
        ms = float(np.median(runs))
        bw = bpp * W * H * N / (ms * 1e-3)
        arm = {"arm": name, "bytes_per_pixel": bpp, "ms_per_launch_median": round(ms, 4),
               "ms_per_launch_runs": [round(r, 4) for r in runs], "bytes_per_s": round(bw / 1e9, 1) * 1e9,
               "fraction_of_8TBps": round(bw / PEAK, 4), "gpix_per_s": round(W * H * N / (ms * 1e-3) / 1e9, 1)}
        result["arms"].append(arm)
        print("%-14s %2d B/px  %.3f ms / 16 frames  %.0f GB/s  %.1f %% of 8 TB/s" % (
            name, bpp, ms, bw / 1e9, 100 * bw / PEAK))
    if not trace:
        line = json.dumps(result)
        print(line)
        if len(sys.argv) > 1:
            with open(sys.argv[1], "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
