#!/usr/bin/env python3
"""Fused colour stage (include/mibayer.h, MIBAYER_FLAG_COLOUR) against the plain kernels in HBM: the same
device-resident batch converted by a colour context (matrix + sRGB curve, and the identity stage with no curve) and by
the plain context of the same method -- the MHC and deep / production kernels, unchanged by the colour stage -- timed
alternately in one process with HIP events on each context's stream (mibayer_time_device).  The stage adds no memory
traffic, so the yardstick is the plain MHC kernel at the same formats.

  python tools/colour_bench.py [OUT.json]     two arms x two methods x {plain, colour off, colour on}
  python tools/colour_bench.py trace          a few launches of everything, for rocprofv3 --kernel-trace --stats

Arms: 4K x 64 8-bit -> BGRx (1 B read + 4 B written per pixel) and 4K x 16 12-bit LE -> ARGB64 (2 + 8 B).
"colour off" is a colour context holding the identity without a curve: the colour kernel's own cost, its bytes equal
the plain context's."""
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
        ("12le->ARGB64 x16", 16, "ARGB64", {"bits": 12}, 10))
METHODS = ("bilinear", "mhc")
ROUNDS = 5
CCM = (1.62, -0.48, -0.14, -0.21, 1.43, -0.22, 0.03, -0.55, 1.52)


def main():
    import __graft_entry__ as entry
    pkg = entry.load_package()
    if pkg.device_count() < 1:
        sys.exit("no HIP device")
    trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
    rng = np.random.default_rng(5)
    result = {"geometry": "%dx%d" % (W, H), "peak_bytes_per_s": PEAK, "rounds": ROUNDS,
              "colour_on": "black level 1/16 of the range, gains (1.9, 1, 1.6) x CCM, sRGB curve", "arms": []}
    for name, n, fmt, deep, bpp in ARMS:
        depth = deep.get("bits", 8)
        if deep:
            frame = rng.integers(0, 1 << 16, (H, W)).astype("<u2")     # junk above bit 12: masked by the kernel
        else:
            frame = rng.integers(0, 256, (H, W), dtype=np.uint8)
        on = pkg.Colour.make(black=(1 << depth) // 16, gains=(1.9, 1.0, 1.6), ccm=CCM, curve=pkg.TONE_SRGB)
        ctxs = {}
        for m in METHODS:
            ctxs[m, "plain"] = pkg.Context(W, H, "bggr", fmt, device=0, method=m, **deep)
            ctxs[m, "colour_off"] = pkg.Context(W, H, "bggr", fmt, device=0, method=m, colour=True, **deep)
            ctxs[m, "colour_on"] = pkg.Context(W, H, "bggr", fmt, device=0, method=m, colour=on, **deep)
        any_ctx = ctxs["mhc", "plain"]
        d_src = any_ctx.device_alloc(n * any_ctx.src_bytes)
        d_dst = any_ctx.device_alloc(n * any_ctx.dst_bytes)
        try:
            for f in range(n):
                any_ctx.to_device(d_src + f * any_ctx.src_bytes, frame)
            if trace:
                for ctx in ctxs.values():
                    for _ in range(20):
                        ctx.process_device(d_src, d_dst, n)
                    ctx.sync()
                continue
            for ctx in ctxs.values():
                t0 = time.time()
                while time.time() - t0 < 0.2:           # clocks up, caches and TLBs warm
                    ctx.process_device(d_src, d_dst, n)
                    ctx.sync()
            runs = {k: [] for k in ctxs}
            for _ in range(ROUNDS):                     # alternating: every kernel sees the same clocks and neighbours
                for k, ctx in ctxs.items():
                    runs[k].append(ctx.time_device(d_src, d_dst, n, warmup=3, reps=30))
            names = {k: ctx.variant_name for k, ctx in ctxs.items()}
        finally:
            any_ctx.device_free(d_src)
            any_ctx.device_free(d_dst)
            for ctx in ctxs.values():
                ctx.close()
        arm = {"arm": name, "frames_per_launch": n, "bytes_per_pixel": bpp}
        for m in METHODS:
            arm[m] = {}
            for what in ("plain", "colour_off", "colour_on"):
                ms = float(np.median(runs[m, what]))
                bw = bpp * W * H * n / (ms * 1e-3)
                arm[m][what] = {"kernel": names[m, what], "ms_per_launch_median": round(ms, 4),
                                "ms_per_launch_runs": [round(r, 4) for r in runs[m, what]],
                                "fraction_of_8TBps": round(bw / PEAK, 4),
                                "gpix_per_s": round(W * H * n / (ms * 1e-3) / 1e9, 1)}
                print("%-17s %-8s %-10s %2d B/px  %.4f ms / launch  %.0f GB/s  %.1f %% of 8 TB/s" % (
                    name, m, what, bpp, ms, bw / 1e9, 100 * bw / PEAK))
        mhc_ms = arm["mhc"]["plain"]["ms_per_launch_median"]
        arm["colour_on_over_plain_mhc_time"] = {m: round(arm[m]["colour_on"]["ms_per_launch_median"] / mhc_ms, 3)
                                                for m in METHODS}
        arm["colour_off_over_plain_mhc_time"] = {m: round(arm[m]["colour_off"]["ms_per_launch_median"] / mhc_ms, 3)
                                                 for m in METHODS}
        result["arms"].append(arm)
    if not trace:
        line = json.dumps(result)
        print(line)
        if len(sys.argv) > 1:
            with open(sys.argv[1], "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
