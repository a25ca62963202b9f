#!/usr/bin/env python3
"""Planar 8-bit output (include/mibayer.h, MIBAYER_FLAG_DST_PLANAR) against its packed 24-bit twin and its 4-byte twin,
in HBM: mibayer_process_device over a device-resident 4K batch (64 frames of an 8-bit mosaic, 16 of a 12-bit one), timed
with HIP events on the context's stream (mibayer_time_device).  All arms run in ONE process on ONE pair of buffers and
alternate, round after round, so that a drift of the clocks or a neighbour on the host hits every arm alike.

  python tools/planar_bench.py [OUT.json]

The triples (algorithmic bytes per pixel read + written):
  8-bit bilinear -> RGBx (1 + 4, the production plan)   -> RGB (1 + 3)   -> RGBP (1 + 3)
  12-bit LE      -> RGBx (2 + 4)                        -> RGB (2 + 3)   -> RGBP (2 + 3)
  MHC 8-bit      -> RGBx (1 + 4)                        -> RGB (1 + 3)   -> RGBP (1 + 3)
  colour, 8-bit  -> RGBx (1 + 4)                        -> RGB (1 + 3)   -> RGBP (1 + 3)
For every arm: ms per launch, Tpix/s and the share of 8 TB/s at its own bytes per pixel; for every triple the time
ratios planar : 24-bit and planar : 4-byte (below 1: the planar arm is faster in pixels per second).

The second pass that planar output removes, as a yardstick: the 4-byte arm's launch plus a torch de-interleave of the
same frames, rgbx.view(N, H, W, 4)[..., :3].permute(0, 3, 1, 2).contiguous(), timed with events in the same process."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160
PEAK = 8.0e12                   # MI355X HBM3E, bytes/s
ROUNDS, WARMUP, REPS = 5, 3, 10
CCM = (1.62, -0.48, -0.14, -0.21, 1.43, -0.22, 0.03, -0.55, 1.52)
# (triple, keywords of Context besides the format, bytes read per pixel, frames per launch)
TRIPLES = (
    ("8-bit bilinear", {}, 1, 64),
    ("12-bit LE", dict(bits=12), 2, 16),
    ("MHC 8-bit", dict(method="mhc"), 1, 64),
    ("colour 8-bit", dict(colour=True), 1, 64),
)
FORMATS = (("RGBx", 4), ("RGB", 3), ("RGBP", 3))


def main():
    import torch                # first, as bench.py does: the process then runs on torch's bundled HIP runtime
    import __graft_entry__ as entry
    pkg = entry.load_package()
    if pkg.device_count() < 1:
        sys.exit("no HIP device")
    rng = np.random.default_rng(24)
    frame16 = rng.integers(0, 1 << 16, (H, W)).astype("<u2")     # 12 bits + junk above them (the kernel masks it)
    frame8 = rng.integers(0, 256, (H, W)).astype(np.uint8)
    col = pkg.Colour.make(black=16, gains=(1.9, 1.0, 1.6), ccm=CCM, curve=pkg.TONE_SRGB)
    arms = []
    for triple, kw, src_px, n in TRIPLES:
        for fmt, dst_px in FORMATS:
            kw2 = dict(kw)
            if kw2.get("colour"):
                kw2["colour"] = col
            ctx = pkg.Context(W, H, "bggr", fmt, device=0, **kw2)
            arms.append({"triple": triple, "fmt": fmt, "ctx": ctx, "bpp": src_px + dst_px, "src16": src_px == 2, "n": n,
                         "runs": []})
    nmax = max(t[3] for t in TRIPLES)
    src = torch.empty(nmax * W * H, dtype=torch.uint8, device="cuda:0")            # 64 8-bit frames, or 16 of 2 B/px
    dst = torch.empty(nmax * 4 * W * H, dtype=torch.uint8, device="cuda:0")
    d_src, d_dst = src.data_ptr(), dst.data_ptr()
    torch.cuda.synchronize()
    second_pass = []
    loaded = None
    for r in range(ROUNDS + 1):                     # round 0 warms every arm up and is not kept
        for a in arms:
            ctx, n = a["ctx"], a["n"]
            if loaded != a["src16"]:
                for f in range(n):
                    ctx.to_device(d_src + f * ctx.src_bytes, frame16 if a["src16"] else frame8)
                loaded = a["src16"]
            if r == 0:
                t0 = time.time()
                while time.time() - t0 < 0.2:       # clocks up, code objects loaded, TLBs warm
                    ctx.process_device(d_src, d_dst, n)
                    ctx.sync()
                continue
            a["runs"].append(ctx.time_device(d_src, d_dst, n, warmup=WARMUP, reps=REPS))
        # the second pass over the 4-byte frames of the first triple (what is in dst does not matter to its time)
        n = TRIPLES[0][3]
        rgbx = dst[:n * 4 * W * H].view(n, H, W, 4)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(WARMUP):
            chw = rgbx[..., :3].permute(0, 3, 1, 2).contiguous()
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(REPS):
            chw = rgbx[..., :3].permute(0, 3, 1, 2).contiguous()
        ev1.record()
        torch.cuda.synchronize()
        del chw
        if r > 0:
            second_pass.append(ev0.elapsed_time(ev1) / REPS)
    result = {"geometry": "%dx%d" % (W, H), "peak_bytes_per_s": PEAK, "rounds": ROUNDS, "reps_per_round": REPS,
              "arms": [], "triples": []}
    for a in arms:
        ms = float(np.median(a["runs"]))
        px_s = W * H * a["n"] / (ms * 1e-3)
        a["ms"] = ms
        result["arms"].append({
            "arm": "%s -> %s" % (a["triple"], a["fmt"]), "kernel": a["ctx"].variant_name, "frames_per_launch": a["n"],
            "bytes_per_pixel": a["bpp"], "ms_per_launch_median": round(ms, 4),
            "ms_per_launch_runs": [round(x, 4) for x in a["runs"]],
            "tpix_per_s": round(px_s / 1e12, 4), "fraction_of_8TBps": round(a["bpp"] * px_s / PEAK, 4)})
        print("%-24s %-24s %d B/px  %.3f ms / %d frames  %.3f Tpix/s  %.1f %% of 8 TB/s" % (
            result["arms"][-1]["arm"], a["ctx"].variant_name, a["bpp"], ms, a["n"], px_s / 1e12,
            100 * a["bpp"] * px_s / PEAK))
        a["ctx"].close()
    for four, three, planar in zip(arms[0::3], arms[1::3], arms[2::3]):
        result["triples"].append({"triple": four["triple"],
                                  "time_planar_over_24bit": round(planar["ms"] / three["ms"], 4),
                                  "time_planar_over_4byte": round(planar["ms"] / four["ms"], 4)})
        print("%-16s planar : 24-bit time = %.3f   planar : 4-byte time = %.3f" % (
            four["triple"], planar["ms"] / three["ms"], planar["ms"] / four["ms"]))
    pass_ms = float(np.median(second_pass))
    four, planar = arms[0], arms[2]
    result["second_pass"] = {
        "what": "torch: rgbx.view(N, H, W, 4)[..., :3].permute(0, 3, 1, 2).contiguous() over the %d frames of "
                "'%s -> RGBx'" % (four["n"], four["triple"]),
        "ms_median": round(pass_ms, 4), "ms_runs": [round(x, 4) for x in second_pass],
        "ms_4byte_arm_plus_second_pass": round(four["ms"] + pass_ms, 4),
        "time_planar_over_4byte_plus_second_pass": round(planar["ms"] / (four["ms"] + pass_ms), 4)}
    print("second pass (torch de-interleave of %d frames): %.3f ms; 4-byte arm + second pass %.3f ms; "
          "planar : that = %.3f" % (four["n"], pass_ms, four["ms"] + pass_ms, planar["ms"] / (four["ms"] + pass_ms)))
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
