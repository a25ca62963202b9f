#!/usr/bin/env python3
"""A fixed sequence of launches through every arm of the launch layer (csrc/mibayer_abi.hip: FrameSet, plan_launch,
launch_frames), for comparing two builds of the library: the ordered list of (kernel, grid, workgroup) must be the same.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/launch_trace.py      the launches
  python tools/launch_trace.py --list DIR/.../t_kernel_trace.csv                                 the ordered list

Runs on the lab build (the rgb2bayer tile kernel, MIBAYER_R2B_FLAT=0, exists there only); MIBAYER_LIB_PATH names
another lab build.  Every step is printed with the (tile, band, grid) mibayer_launch_geometry reports for it and ends
with a sync, so the order of the trace is the order of the steps.  The frames hold whatever the allocation held."""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ordered_list(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        grid = "x".join(r.get(k, "1") for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z")) \
            if "Grid_Size_X" in r else r["Grid_Size"]
        wg = "x".join(r.get(k, "1") for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z")) \
            if "Workgroup_Size_X" in r else r["Workgroup_Size"]
        print("%s\tgrid %s\tworkgroup %s" % (r["Kernel_Name"], grid, wg))


if len(sys.argv) > 2 and sys.argv[1] == "--list":
    ordered_list(sys.argv[2])
    sys.exit(0)

import numpy as np  # noqa: E402

import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package(lab="MIBAYER_LIB_PATH" not in os.environ)
assert pkg.lib().mibayer_is_lab_build() == 1, "tools/launch_trace.py needs a lab build (make lab)"
NAMES = pkg.variant_names()


class Frames:
    """n separately allocated source / destination frames and one contiguous batch of them"""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.srcs = [ctx.device_alloc(ctx.src_bytes) for _ in range(n)]
        self.dsts = [ctx.device_alloc(ctx.dst_bytes + 64) for _ in range(n)]
        self.src, self.dst = ctx.device_alloc(n * ctx.src_bytes), ctx.device_alloc(n * ctx.dst_bytes)

    def free(self):
        for p in self.srcs + self.dsts + [self.src, self.dst]:
            self.ctx.device_free(p)


def step(label, ctx, fn, geometry_of=None):
    geo = ""
    if geometry_of is not None:
        g = ctx.launch_geometry(geometry_of)
        geo = "  [tile %dx%d band %d grid %d]" % (g["tile_w"], g["tile_h"], g["band"], g["grid_blocks"])
    print("%s%s" % (label, geo), flush=True)
    fn()
    ctx.sync()


def strided_and_lists(tag, ctx, dst_off=0):
    """batches of 1 and 64, lists of 5 and 21 (two launches: 16 + 5); dst_off: the list's destinations that far in"""
    fr = Frames(ctx, 64)
    try:
        step("%s: strided batch of 1" % tag, ctx, lambda: ctx.process_device(fr.src, fr.dst, 1), 1)
        step("%s: strided batch of 64" % tag, ctx, lambda: ctx.process_device(fr.src, fr.dst, 64), 64)
        for n in (5, 21):
            step("%s: list of %d" % (tag, n), ctx, lambda: ctx.process_device_list(
                fr.srcs[:n], [d + dst_off for d in fr.dsts[:n]]), min(n, 16))
    finally:
        fr.free()


def tile_arms():
    # fast: 1920x1080 at the default strides; generic: 642 px; aligned: 642 px under set_plan (.., 128), whose list has
    # destinations at 8 mod 16
    with pkg.Context(1920, 1080, "rggb", "BGRx", device=0) as ctx:
        strided_and_lists("tile fast 1920x1080", ctx)
    with pkg.Context(642, 480, "grbg", "RGBx", device=0) as ctx:
        strided_and_lists("tile generic 642x480", ctx)
        ctx.set_plan(NAMES.index("lds_2x4_r4_dpp_nt"), 1, 128)
        strided_and_lists("tile aligned128 642x480", ctx, dst_off=8)
        ctx.set_plan(NAMES.index("lds_2x4_r4_dpp_nt"), 0, 64)
        strided_and_lists("tile aligned64 642x480", ctx, dst_off=8)


def host_frames():
    w, h = 3840, 2160                   # large enough for the banded path
    src = np.zeros((h, w), np.uint8)
    with pkg.Context(w, h, "bggr", "BGRx", device=0) as ctx:
        step("host path: banded frame, 4K", ctx, lambda: ctx.process_host(src), 1)
    with pkg.Context(w, h, "bggr", "BGRx", dst_stride=4 * w + 64, device=0) as ctx:
        step("host path: banded frame, padded destination rows", ctx, lambda: ctx.process_host(src), 1)
    for label, flags in (("compute-queue graph", pkg.FLAG_HIPGRAPH),
                         ("whole-frame graph", pkg.FLAG_HIPGRAPH | pkg.FLAG_HIPGRAPH_CHAIN)):
        with pkg.Context(w, h, "bggr", "BGRx", flags=flags, device=0) as ctx:
            step("host path: %s, two frames" % label, ctx, lambda: (ctx.process_host(src), ctx.process_host(src)), 1)
    with pkg.Context(640, 480, "bggr", "BGRx", device=0) as ctx:
        step("host path: plain frame, 640x480", ctx, lambda: ctx.process_host(np.zeros((480, 640), np.uint8)), 1)


def strip_contexts():
    w, h = 1282, 722
    for tag, kw in (("strip plain 12-bit to ARGB64", dict(fmt="ARGB64", bits=12)),
                    ("strip MHC 8-bit to BGRx", dict(fmt="BGRx", method="mhc")),
                    ("strip colour 10-bit MHC to RGB", dict(fmt="RGB", bits=10, method="mhc", colour=True)),
                    ("strip planar 8-bit to GBR", dict(fmt="GBR"))):
        with pkg.Context(w, h, "gbrg", device=0, **kw) as ctx:
            fr = Frames(ctx, 21)
            try:
                step("%s: strided batch of 1" % tag, ctx, lambda: ctx.process_device(fr.src, fr.dst, 1))
                step("%s: strided batch of 21" % tag, ctx, lambda: ctx.process_device(fr.src, fr.dst, 21))
                step("%s: list of 5" % tag, ctx, lambda: ctx.process_device_list(fr.srcs[:5], fr.dsts[:5]))
                step("%s: list of 21" % tag, ctx, lambda: ctx.process_device_list(fr.srcs, fr.dsts))
                step("%s: host frame" % tag, ctx, lambda: ctx.process_host(np.zeros(ctx.src_bytes, np.uint8)))
            finally:
                fr.free()
    with pkg.Context(3840, 2160, "gbrg", "ARGB64", bits=12, device=0) as ctx:
        step("strip plain 12-bit: banded host frame, 4K", ctx,
             lambda: ctx.process_host(np.zeros(ctx.src_bytes, np.uint8)))


def inverse_contexts():
    for tag, env in (("rgb2bayer flat kernel", None), ("rgb2bayer tile kernel (MIBAYER_R2B_FLAT=0)", "0")):
        if env is None:
            os.environ.pop("MIBAYER_R2B_FLAT", None)
        else:
            os.environ["MIBAYER_R2B_FLAT"] = env
        for w, h in ((1920, 1080), (642, 480)):
            with pkg.Context(w, h, "rggb", (1, 2, 3), flags=pkg.FLAG_RGB2BAYER, device=0) as ctx:
                fr = Frames(ctx, 21)
                try:
                    t = "%s %dx%d" % (tag, w, h)
                    step("%s: strided batch of 1" % t, ctx, lambda: ctx.process_device(fr.src, fr.dst, 1))
                    step("%s: strided batch of 21" % t, ctx, lambda: ctx.process_device(fr.src, fr.dst, 21))
                    step("%s: list of 5" % t, ctx, lambda: ctx.process_device_list(fr.srcs[:5], fr.dsts[:5]))
                    step("%s: list of 21" % t, ctx, lambda: ctx.process_device_list(fr.srcs, fr.dsts))
                    step("%s: list of 5, destinations at 4 mod 8" % t, ctx, lambda: ctx.process_device_list(
                        fr.srcs[:5], [d + 4 for d in fr.dsts[:5]]))
                    step("%s: host frame" % t, ctx, lambda: ctx.process_host(np.zeros(ctx.src_bytes, np.uint8)))
                finally:
                    fr.free()
    os.environ.pop("MIBAYER_R2B_FLAT", None)
    with pkg.Context(3840, 2160, "rggb", (1, 2, 3), flags=pkg.FLAG_RGB2BAYER, device=0) as ctx:
        step("rgb2bayer: banded host frame, 4K", ctx, lambda: ctx.process_host(np.zeros(ctx.src_bytes, np.uint8)))


def measurements():
    with pkg.Context(1922, 1082, "grbg", "BGRx", bits=12, device=0) as ctx:
        d_src, d_out = ctx.device_alloc(3 * ctx.src_bytes), ctx.device_alloc(3 * 8 * 8 * 64 + 3 * 4096)
        try:
            step("statistics: 3 frames, 8x8 zones", ctx, lambda: ctx.stats_device(d_src, d_out, 8, 8, 16, 4000, 3))
            step("histogram: 3 frames, a window", ctx, lambda: ctx.hist_device(d_src, d_out, (2, 1, 1000, 700), 3))
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_out)
        ctx.set_stats(4, 4, 0, 4095)
        ctx.set_hist(True)
        step("host frame with statistics and a histogram", ctx,
             lambda: ctx.process_host(np.zeros(ctx.src_bytes, np.uint8)))


tile_arms()
host_frames()
strip_contexts()
inverse_contexts()
measurements()
print("done")
