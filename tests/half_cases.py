"""TEST INFRASTRUCTURE: the case table of the half-size demosaic's GPU tests (tests/test_gpu_half.py).  No GPU and no
library here: tests/test_half_cases.py asserts, from this table alone, which seam every case reaches, and that the
constants are the kernel's (csrc/mibayer_internal.h).

bayer2rgb_half_kernel: a lane owns LANE_PIXELS output pixels, a wave a strip of WAVE_PIXELS output pixels x ROWS output
rows, a workgroup four waves in launch order -- side by side (GROUP_PIXELS) where the row is that long.  The last lane
of a row holds 1 .. 4 pixels; whether the row ends in a wave that is full (one wide load per row) or not (dword by
dword) is a path of its own, and so are the pieces of the 8-byte pixel store, which depend on the last lane's place in
its quad of lanes: together OW % 16."""
import collections

LANE_PIXELS = 4                 # kHalfLanePixels
WAVE_PIXELS = 256               # kHalfWavePixels
GROUP_PIXELS = 1024             # kHalfGroupPixels
ROWS = 4                        # kHalfRows: output rows per wave (and per workgroup)
MAX_LIST = 16                   # kMaxList

ORDERS = ("bggr", "gbrg", "grbg", "rggb")
# output families: (name of the layout, bytes of a pixel in a row)
LAYOUT8 = ("RGBx", "BGRx", "xRGB", "xBGR")
LAYOUT16 = ("ARGB64",)          # little- and big-endian: Family.dbe
LAYOUT24 = ("RGB", "BGR")
PLANAR = ("GBR", "RGBP", "BGRP")

Family = collections.namedtuple("Family", "fmt px dbe")
FAMILIES = (tuple(Family(f, 4, False) for f in LAYOUT8) + (Family("ARGB64", 8, False), Family("ARGB64", 8, True))
            + tuple(Family(f, 3, False) for f in LAYOUT24) + tuple(Family(f, 1, False) for f in PLANAR))

# sample formats: (bits, big-endian); bits = 0 is the 8-bit mosaic
SAMPLES = ((0, False), (10, False), (10, True), (12, False), (12, True), (16, False), (16, True))

# lane, wave and workgroup extent - 1, 0, + 1, and the smallest rows: 1, 2, 3 pixels in the only lane
OUT_WIDTHS = (2, 3, LANE_PIXELS, LANE_PIXELS + 1, 2 * LANE_PIXELS - 1, 2 * LANE_PIXELS, 2 * LANE_PIXELS + 1,
              WAVE_PIXELS - 1, WAVE_PIXELS, WAVE_PIXELS + 1, GROUP_PIXELS - 1, GROUP_PIXELS, GROUP_PIXELS + 1)
# mosaic heights: the smallest three, and one short of / exactly / one and two over a workgroup's 2 ROWS source rows
HEIGHTS = (3, 4, 5, 2 * ROWS - 1, 2 * ROWS, 2 * ROWS + 1, 2 * ROWS + 2)
SWEEP_HEIGHT = 2 * ROWS + 3     # the height of the width sweep: two chunks, the second short, the last row dropped
SWEEP_OUT_WIDTHS = (WAVE_PIXELS + 1, 7)         # the widths of the height sweep

Case = collections.namedtuple("Case", "w h order family bits sbe")


def width_of(ow):
    return 2 * ow


def out_size(w, h):
    return w // 2, h >> 1


def row_end(ow):
    """where an output row ends: the wave and lane that hold its last pixels, how many (1 .. 4), whether that wave is
    full (every lane 4 pixels) and the last lane's place in its quad"""
    g = (ow + LANE_PIXELS - 1) // LANE_PIXELS - 1
    return {"wave": g // 64, "lane": g % 64, "n": ow - LANE_PIXELS * g, "wave_full": ow % WAVE_PIXELS == 0,
            "quad_lane": g % 4}


def chunks(h):
    """(chunks of ROWS output rows, output rows of the last one, whether a source row is dropped)"""
    oh = h >> 1
    n = (oh + ROWS - 1) // ROWS
    return n, oh - ROWS * (n - 1), bool(h & 1)


def sizes():
    return [(width_of(ow), SWEEP_HEIGHT) for ow in OUT_WIDTHS] + [(width_of(ow), h) for ow in SWEEP_OUT_WIDTHS
                                                                   for h in HEIGHTS]


def cases(family, first=0):
    """every size for one output family, from an 8-bit mosaic AND from a deep one: the Bayer order and the deep sample
    format rotate with the index at periods 4 and 6"""
    deep = SAMPLES[1:]
    out = []
    for i, (w, h) in enumerate(sizes()):
        out.append(Case(w, h, ORDERS[(first + i) % 4], family, *SAMPLES[0]))
        out.append(Case(w, h, ORDERS[(first + i + 1) % 4], family, *deep[(first + i) % len(deep)]))
    return out


def dst_row_bytes(family, ow):
    return family.px * ow


def default_dst_stride(family, ow):
    return (family.px * ow + 3) & ~3


def padded_dst_stride(family, ow):
    """the default stride + 8: a multiple of 8 wherever the default is (16-bit channels need one)"""
    return default_dst_stride(family, ow) + 8


def tail_stores(family, n):
    """the byte sizes of the stores a last lane of n pixels issues per row (per plane when planar): exactly px * n"""
    if family.px == 8:
        return [16] * (n // 2) + [8] * (n % 2)
    if family.px == 4:
        return {4: [16], 3: [8, 4], 2: [8], 1: [4]}[n]
    if family.px == 3:
        return {4: [12], 3: [8, 1], 2: [4, 2], 1: [2, 1]}[n]
    return {4: [4], 3: [2, 1], 2: [2], 1: [1]}[n]
