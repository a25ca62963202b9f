#!/usr/bin/env python3
"""Packed 24-bit output (include/mibayer.h, MIBAYER_FLAG_DST_24BIT) against its 4-byte twin, in HBM:
mibayer_process_device over a 64-frame 4K batch, device-resident, timed with HIP events on the context's stream
(mibayer_time_device).  All arms run in ONE process on ONE pair of buffers and alternate, round after round, so that a
drift of the clocks or a neighbour on the host hits every arm alike.

  python tools/rgb24_bench.py [OUT.json]

The pairs (4-byte twin first; algorithmic bytes per pixel read + written):
  8-bit bilinear -> BGRx (1 + 4, the production plan: the yardstick)   -> BGR (1 + 3, the strip kernel)
  12-bit LE      -> BGRx (2 + 4)                                        -> BGR (2 + 3)
  MHC 8-bit      -> BGRx (1 + 4)                                        -> BGR (1 + 3)
  colour, 8-bit  -> BGRx (1 + 4)                                        -> BGR (1 + 3)
For every arm: ms per launch, Tpix/s and the share of 8 TB/s at its own bytes per pixel; for every pair the 24-bit :
4-byte time ratio (below 1: the 24-bit arm is faster in pixels per second)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, N = 3840, 2160, 64
PEAK = 8.0e12                   # MI355X HBM3E, bytes/s
ROUNDS, WARMUP, REPS = 5, 3, 10
CCM = (1.62, -0.48, -0.14, -0.21, 1.43, -0.22, 0.03, -0.55, 1.52)
# (pair, keywords of Context besides the format, bytes read per pixel)
PAIRS = (
    ("8-bit bilinear", {}, 1),
    ("12-bit LE", dict(bits=12), 2),
    ("MHC 8-bit", dict(method="mhc"), 1),
    ("colour 8-bit", dict(colour=True), 1),
)


def main():
    import __graft_entry__ as entry
    pkg = entry.load_package()
    if pkg.device_count() < 1:
        sys.exit("no HIP device")
    rng = np.random.default_rng(24)
    frame16 = rng.integers(0, 1 << 16, (H, W)).astype("<u2")     # 12 bits + junk above them (the kernel masks it)
    frame8 = rng.integers(0, 256, (H, W)).astype(np.uint8)
    col = pkg.Colour.make(black=16, gains=(1.9, 1.0, 1.6), ccm=CCM, curve=pkg.TONE_SRGB)
    arms = []
    for pair, kw, src_px in PAIRS:
        for fmt, dst_px in (("BGRx", 4), ("BGR", 3)):
            kw2 = dict(kw)
            if kw2.get("colour"):
                kw2["colour"] = col
            ctx = pkg.Context(W, H, "bggr", fmt, device=0, **kw2)
            arms.append({"pair": pair, "fmt": fmt, "ctx": ctx, "bpp": src_px + dst_px, "src16": src_px == 2, "runs": []})
    first = arms[0]["ctx"]
    d_src = first.device_alloc(N * 2 * W * H)
    d_dst = first.device_alloc(N * 4 * W * H)
    try:
        loaded = None
        for r in range(ROUNDS + 1):                     # round 0 warms every arm up and is not kept
            for a in arms:
                ctx = a["ctx"]
                if loaded != a["src16"]:
                    for f in range(N):
                        ctx.to_device(d_src + f * ctx.src_bytes, frame16 if a["src16"] else frame8)
                    loaded = a["src16"]
                if r == 0:
                    t0 = time.time()
                    while time.time() - t0 < 0.2:       # clocks up, code objects loaded, TLBs warm
                        ctx.process_device(d_src, d_dst, N)
                        ctx.sync()
                    continue
                a["runs"].append(ctx.time_device(d_src, d_dst, N, warmup=WARMUP, reps=REPS))
    finally:
        first.device_free(d_src)
        first.device_free(d_dst)
    result = {"geometry": "%dx%d" % (W, H), "frames_per_launch": N, "peak_bytes_per_s": PEAK, "rounds": ROUNDS,
              "reps_per_round": REPS, "arms": [], "pairs": []}
    for a in arms:
        ms = float(np.median(a["runs"]))
        px_s = W * H * N / (ms * 1e-3)
        a["ms"] = ms
        result["arms"].append({
            "arm": "%s -> %s" % (a["pair"], a["fmt"]), "kernel": a["ctx"].variant_name, "bytes_per_pixel": a["bpp"],
            "ms_per_launch_median": round(ms, 4), "ms_per_launch_runs": [round(x, 4) for x in a["runs"]],
            "tpix_per_s": round(px_s / 1e12, 4), "fraction_of_8TBps": round(a["bpp"] * px_s / PEAK, 4)})
        print("%-24s %-24s %d B/px  %.3f ms / %d frames  %.3f Tpix/s  %.1f %% of 8 TB/s" % (
            result["arms"][-1]["arm"], a["ctx"].variant_name, a["bpp"], ms, N, px_s / 1e12, 100 * a["bpp"] * px_s / PEAK))
        a["ctx"].close()
    for four, three in zip(arms[0::2], arms[1::2]):
        ratio = three["ms"] / four["ms"]
        result["pairs"].append({"pair": four["pair"], "time_24bit_over_4byte": round(ratio, 4)})
        print("%-16s 24-bit : 4-byte time = %.3f" % (four["pair"], ratio))
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
