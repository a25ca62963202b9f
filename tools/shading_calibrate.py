#!/usr/bin/env python3
"""Lens shading calibration (include/mibayer.h, group `shading`): a raw flat-field frame -> the zone statistics of the
mosaic (mibayer_stats_device) -> a gain table (mibayer_stats_shading) -> the MISH file bayer2rgb shading-file= reads.

  python tools/shading_calibrate.py FLAT.raw WIDTHxHEIGHT OUT.mish [--bits N] [--big-endian] [--stride BYTES]
         [--black B | --black B0,B1,B2,B3] [--cells KX,KY] [--zones ZX,ZY] [--max-gain G] [--device D]

FLAT.raw holds one frame (more are ignored): rows of --stride bytes (default: the width rounded up to 4, or two bytes per
sample with --bits 10/12/14/16).  The black level is per CFA site s = 2 (y & 1) + (x & 1).  Clipped samples (the top
1/64 of the range) are left out of the zone means.  Defaults: cells of 32 x 32 (--cells 5,5), as many zones as fit (up to
64 x 64), max gain 7.99.

The file, little-endian: "MISH", u32 version = 1, kx, ky, nx, ny, black[4] (all u32), then the 4 * ny * nx u16 table."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_mish(path, kx, ky, table, black):
    """the file's one writer in the product tree; element_load_shading (gst/gstmibayerelement.c) is its reader, and
    tests/test_shading_abi.py holds this writer and the test model's to the same bytes"""
    _, ny, nx = table.shape
    with open(path, "wb") as f:
        f.write(b"MISH" + np.array([1, kx, ky, nx, ny] + list(black), "<u4").tobytes() + table.astype("<u2").tobytes())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("flat")
    ap.add_argument("size")
    ap.add_argument("out")
    ap.add_argument("--bits", type=int, default=0)
    ap.add_argument("--big-endian", action="store_true")
    ap.add_argument("--stride", type=int, default=0)
    ap.add_argument("--black", default="0")
    ap.add_argument("--cells", default="5,5")
    ap.add_argument("--zones", default="")
    ap.add_argument("--max-gain", type=float, default=7.99)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import __graft_entry__ as entry
    pkg = entry.load_package()
    if pkg.device_count() < 1:
        sys.exit("no HIP device")
    w, h = (int(v) for v in a.size.lower().split("x"))
    kx, ky = (int(v) for v in a.cells.split(","))
    black = [int(v) for v in a.black.split(",")]
    black = black * 4 if len(black) == 1 else black
    assert len(black) == 4, "--black takes one value or four"
    zx, zy = (int(v) for v in a.zones.split(",")) if a.zones else (min(64, w // 2), min(64, h // 2))
    depth = a.bits or 8
    vmax = (1 << depth) - 1
    nx, ny = pkg.shading_nodes(w, h, kx, ky)
    # the Bayer order plays no part: statistics and gains are per CFA SITE (row and column parity), whatever its colour
    with pkg.Context(w, h, "bggr", "RGBx", src_stride=a.stride, bits=a.bits, src_big_endian=a.big_endian,
                     device=a.device) as ctx:
        frame = np.fromfile(a.flat, np.uint8, ctx.src_bytes)
        if frame.size < ctx.src_bytes:
            sys.exit("%s holds %d bytes, a frame is %d" % (a.flat, frame.size, ctx.src_bytes))
        d_src, d_stats = ctx.device_alloc(ctx.src_bytes), ctx.device_alloc(zx * zy * 64)
        try:
            ctx.to_device(d_src, frame)
            ctx.stats_device(d_src, d_stats, zx, zy, 0, vmax - (vmax >> 6))
            ctx.sync()
            zones = ctx.from_device(d_stats, zx * zy * 64).view(pkg.STATS_DTYPE).reshape(zy, zx)
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_stats)
    clipped = int(zones["clipped"].sum())
    ok, table = pkg.stats_shading(zones, w, h, black, kx, ky, a.max_gain)
    if not ok:
        sys.exit("no table: a CFA site has no unclipped samples, or its mean is not above the black level")
    write_mish(a.out, kx, ky, table, black)
    print("%s: %dx%d, cells %dx%d, %d x %d nodes, %d x %d zones, %d clipped samples left out" % (
        a.out, w, h, 1 << kx, 1 << ky, nx, ny, zx, zy, clipped))
    for s in range(4):
        print("  site %d: gain %.3f .. %.3f" % (s, table[s].min() / 4096.0, table[s].max() / 4096.0))


if __name__ == "__main__":
    main()
