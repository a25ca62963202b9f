"""TEST INFRASTRUCTURE: the case tables of the tile-kernel tests (tests/test_gpu_tile_geometry.py).  No GPU here:
tests/test_tile_cases.py asserts, from these tables alone, that the widths, heights, pitches and plans reach the
branches they are meant to reach.

The 8-bit tile kernels (csrc/mibayer_kernels.hip: bayer2rgb_lds_kernel, fast and GENERIC arm, and
bayer2rgb_lds_aligned_kernel): a workgroup converts a tile of tile_w x tile_h pixels, WX x WY waves of 256 pixels x
4 rows; a lane owns 4 pixels.  The tile is staged in 16-byte chunks (TW / 16 per row) plus one halo dword on either
side; in the GENERIC arm the chunk that straddles ROUND_UP_4 (width) is read dword by dword (`avail` = 4, 8, 12).
Lane 0 and lane 63 of a wave take their outer neighbour from LDS -- the next wave's dword, or the halo at a tile seam.
The aligned arm shifts the lane map of every output row by s = ((-row address) mod 128) / 4 pixels, one of 16 even values."""
import collections

import strip_cases as sc
from strip_cases import ORDERS, LAYOUT8, last_group, plane_frames, pattern_frames    # noqa: F401  (shared, not copied)

# -- the kernels' geometry (kVariants, LDS_VARIANT_AL / LDS_VARIANT in csrc/mibayer_kernels.hip) ---------------------

WAVE_PX = 256                   # 64 lanes x 4 pixels
ROWS_PER_WAVE = 4               # RPW of every production shape
CHUNK = 16                      # bytes of one staging load
ALIGN = 128                     # the one flavour of the aligned arm the product build has
NUM_XCD = 8                     # kNumXcd (csrc/mibayer_internal.h: block_to_tile)
MAX_LIST = sc.MAX_LIST          # kMaxList

Shape = collections.namedtuple("Shape", "stem tile_w tile_h")
SHAPES = (Shape("lds_4x2_r4_dpp", 1024, 8), Shape("lds_2x4_r4_dpp", 512, 16), Shape("lds_1x8_r4_dpp", 256, 32))
STORES = ("_nt", "", "_hy")     # streaming, plain (write-back), hybrid
NT_NAMES = tuple(s.stem + "_nt" for s in SHAPES)
PLAIN_NAMES = tuple(s.stem for s in SHAPES)
HY_NAMES = tuple(s.stem + "_hy" for s in SHAPES)
PRODUCTION_NAMES = NT_NAMES + PLAIN_NAMES + HY_NAMES    # ids 1 .. 9, looked up by name (pkg.variant_names())
ARM128_NAMES = NT_NAMES + PLAIN_NAMES                   # LDS_VARIANT_AL: the names that have a 128-byte arm

# the eight 4-byte layouts of the element's src template (FORMATS of the ctypes harness)
ALL_FORMATS = LAYOUT8 + ("RGBA", "BGRA", "ARGB", "ABGR")


def shape_of(name):
    return next(s for s in SHAPES if name.startswith(s.stem))


def variant_id(pkg, name):
    return pkg.variant_names().index(name)


# -- tables ----------------------------------------------------------------------------------------------------------

# every even residue mod 16 inside one wave; around each tile width TW: TW-2, TW, TW+2, TW+4, TW+6, TW+10; 1040: the
# fast path with a second tile of 16 px; 2050: three tiles of 1024 and a tail
WIDTHS = (20, 22, 24, 26, 28, 30, 32, 34,
          254, 256, 258, 260, 262, 266,
          510, 512, 514, 516, 518, 522,
          1022, 1024, 1026, 1028, 1030, 1034,
          1040, 2050)
SWEEP_HEIGHT = 35               # every shape: more than one tile row, the last one 3 rows high
HEIGHTS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12,
           15, 16, 17, 18, 19, 20,
           31, 32, 33, 34, 35, 36,
           63, 64, 65, 67)
HEIGHT_WIDTHS = (262, 1028)     # 262: two tiles per row for 256x32 only; 1028: a tile seam for every shape

# (w, h, extra destination pitch, destination offset inside the allocation, frames, frame pitch extra): run under
# set_plan (id, band, 128).  The offset and every pitch are multiples of 8; the allocation is 0 mod 128.
ALIGNED_CASES = (
    # every one of the 16 shifts: pitch = 8 x odd (mod 128) walks through all of them in 16 rows
    (258, 35, 0, 0, 4, 8),      # width % 4 == 2; pitch 1032 = 8 mod 128; the phase moves from frame to frame
    (260, 19, 8, 0, 1, 0),      # width % 4 == 0 needs a pitch (or offset) of 8 mod 16: 1048 = 24 mod 128
    (512, 17, 8, 0, 1, 0),      # ... and a row at shift 0 whose last wave ends exactly at the width
    (1028, 17, 0, 8, 2, 8),     # pitch 16 mod 128: offset 8 gives the odd multiples of 8, the second frame the rest
    # narrower than the largest head (30 px): a pitch of 0 mod 128 at offset 0 would be on the grid
    (4, 6, 8, 8, 2, 8),
    (6, 7, 0, 8, 3, 8),
    (14, 40, 0, 0, 1, 0),
    (30, 17, 16, 0, 2, 8),      # 120 + 8 = 128 would be on the grid: + 16
    (32, 18, 8, 0, 1, 0),
    (34, 6, 0, 24, 1, 0),
    # wave_x + 256 below / equal to / above the width: 256 + s and 512 + s, and the seam widths of WIDTHS
    (254, 18, 0, 0, 1, 0),
    (256, 17, 8, 0, 1, 0),
    (262, 17, 0, 0, 2, 8),
    (266, 5, 24, 56, 1, 0),
    (270, 16, 0, 8, 1, 0),
    (286, 16, 0, 0, 1, 0),      # 256 + 30: the largest shift
    (288, 6, 0, 8, 1, 0),       # pitch 1152 = 0 mod 128, on the grid but for the offset: a constant shift of 30
    (510, 17, 0, 0, 1, 0),
    (514, 17, 0, 0, 2, 8),
    (516, 16, 8, 0, 1, 0),
    (518, 16, 0, 0, 1, 0),
    (522, 16, 0, 0, 1, 0),
    (542, 16, 0, 0, 1, 0),      # 512 + 30
    (1022, 17, 0, 0, 1, 0),
    (1024, 9, 8, 8, 2, 8),
    (1026, 17, 0, 0, 2, 8),
    (1030, 33, 0, 120, 2, 8),
    (1034, 16, 0, 0, 1, 0),
    (1040, 9, 8, 0, 1, 0),
    (1290, 8, 104, 72, 1, 0),
    (2050, 12, 40, 16, 1, 0),
)
ALIGNED_BANDS = (0, 1, -1)      # rotate with the case index

# (w, h, frames, variant name, band): the tile-row count is no multiple of 8 x band, so trailing blocks idle, and a band
# (band >= 2) holds tile rows of two frames; with band 1 one XCD walks tile rows of two frames
PLAN_CASES = (
    (1028, 19, 3, "lds_4x2_r4_dpp_nt", 1),
    (1028, 19, 3, "lds_2x4_r4_dpp_nt", 3),
    (1028, 35, 5, "lds_1x8_r4_dpp_nt", 1),
    (262, 35, 5, "lds_4x2_r4_dpp", 3),
    (1028, 19, 3, "lds_2x4_r4_dpp", 0),
    (262, 35, 5, "lds_1x8_r4_dpp", 3),
    (1028, 19, 3, "lds_4x2_r4_dpp_hy", -1),
    (262, 35, 5, "lds_2x4_r4_dpp_hy", -1),
    (262, 67, 3, "lds_1x8_r4_dpp_hy", -1),
    (262, 35, 5, "lds_1x8_r4_dpp_nt", 0),
    (262, 35, 5, "lds_2x4_r4_dpp_nt", 1),
    (1028, 19, 3, "lds_4x2_r4_dpp", 0),
)

# the value extremes: (w, h) of the fast and of the generic geometry; the third run is the generic one under the
# 128-byte arm with EXTREME_ALIGNED_PAD more bytes per destination row
EXTREME_FAST = (272, 18)
EXTREME_GENERIC = (266, 18)
EXTREME_ALIGNED_PAD = 8


def weakest_widths(shape):
    """the widths converted from the weakest base pointers: the seam of the shape, and the widths every arm would take
    its fast path at"""
    tw = shape.tile_w
    return tuple(sorted({tw - 2, tw, tw + 2, tw + 4, tw + 6, tw + 10, 32, 256, 512, 1024}))


# -- cases -----------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "w h order layout")


def rotate(i, w, h):
    """case i: the Bayer order and the layout rotate with the index at different periods (4 and 8; 32 cases in a row see
    all 32 pairs)"""
    return Case(w, h, ORDERS[i % 4], ALL_FORMATS[(i // 4 + i) % 8])


def width_cases(k=0):
    """every width at SWEEP_HEIGHT; k: the variant's index, so that the variants do not all see the same pairs"""
    return [rotate(i + 5 * k, w, SWEEP_HEIGHT) for i, w in enumerate(WIDTHS)]


def fast_width_cases(k=0):
    """the widths of the sweep the fast arm takes (0 mod 16), once more: converted with unpadded strides"""
    return [rotate(i + 5 * k + 2, w, SWEEP_HEIGHT) for i, w in enumerate(WIDTHS) if w % 16 == 0]


def height_cases(k=0):
    sizes = [(w, h) for w in HEIGHT_WIDTHS for h in HEIGHTS]
    return [rotate(i + 3 * k, w, h) for i, (w, h) in enumerate(sizes)]


def src_stride_of(w):
    return ((w + 3) & ~3) + 12          # rows dword-aligned, not 8-byte-aligned


def fast_width(w):
    """the next width the fast arm takes; 1028 -> 1040 and 262 -> 272 keep the tiles per row of every shape"""
    return (w + 15) & ~15


# -- what a launch runs ----------------------------------------------------------------------------------------------

# src_mod / dst_mod: the base pointers mod 128 (device allocations are 0 mod 128; asserted where it matters);
# align / has_arm: the plan's store alignment and whether the variant has that arm; as_list: a list launch over the
# frames at base + f * frame bytes
Launch = collections.namedtuple("Launch", "w src_stride dst_stride src_mod dst_mod nframes src_fb dst_fb align has_arm "
                                          "as_list")


def make_launch(w, h, src_stride=None, dst_stride=None, src_mod=0, dst_mod=0, nframes=1, dst_gap=0, align=0,
                has_arm=True, as_list=False):
    src_stride = src_stride or (w + 3) & ~3
    dst_stride = dst_stride or 4 * w
    return Launch(w, src_stride, dst_stride, src_mod, dst_mod, nframes, src_stride * h, dst_stride * h + dst_gap, align,
                  has_arm, as_list)


def sweep_launch(case, weakest=False, padded=True):
    """the launches of the width sweep (and, weakest, of the weakest-base-pointer test); padded: source stride
    ROUND_UP_4 (w) + 12 and destination stride 4 w + 24, else the defaults"""
    off = 4 if weakest else 0
    if not padded:
        return make_launch(case.w, case.h, src_mod=off, dst_mod=off)
    return make_launch(case.w, case.h, src_stride_of(case.w), 4 * case.w + 24, off, off)


def height_launch(case, align):
    return make_launch(case.w, case.h, src_stride_of(case.w), 4 * case.w + 8, align=align)


def aligned_launch(row, as_list=False):
    w, h, pad, off, n, gap = row
    return make_launch(w, h, src_stride_of(w), 4 * w + pad, 0, off % 128, n, gap, ALIGN, True, as_list)


def expected_arm(L):
    """"fast" | "generic" | "aligned128": the arm a launch runs.  This RESTATES the rule of plan_launch
    (csrc/mibayer_abi.hip: the block that computes `fast`, `rows8`, `on_grid`) for the pointers the GPU tests use; the
    ABI cannot report which arm ran, so it is not an observation."""
    srcs = [(L.src_mod + f * L.src_fb) for f in range(L.nframes)]
    dsts = [(L.dst_mod + f * L.dst_fb) for f in range(L.nframes)]
    if L.as_list:               # the caller looked at every frame pointer; frame pitches do not apply
        ptr16 = all(p % 16 == 0 for p in srcs + dsts)
        dst8 = all(p % 8 == 0 for p in dsts)
        on_grid = False
    else:
        ptr16 = L.src_mod % 16 == 0 and L.dst_mod % 16 == 0 and (
            L.nframes == 1 or (L.src_fb % 16 == 0 and L.dst_fb % 16 == 0))
        dst8 = L.dst_mod % 8 == 0 and (L.nframes == 1 or L.dst_fb % 8 == 0)
        on_grid = L.dst_stride % ALIGN == 0 and L.dst_mod % ALIGN == 0 and (L.nframes == 1 or L.dst_fb % ALIGN == 0)
    fast = L.w % 16 == 0 and L.src_stride % 16 == 0 and L.dst_stride % 16 == 0 and ptr16
    if fast:
        return "fast"
    if L.align == ALIGN and L.has_arm and L.dst_stride % 8 == 0 and dst8 and not on_grid:
        return "aligned128"
    return "generic"


def row_addresses(row, base_mod_128=0):
    """(frame, row, address mod 128) of every output row of an ALIGNED_CASES entry"""
    w, h, pad, off, n, gap = row
    stride = 4 * w + pad
    return [(f, j, (base_mod_128 + off + f * (stride * h + gap) + j * stride) % ALIGN)
            for f in range(n) for j in range(h)]


def shift_of(address):
    """s of bayer2rgb_lds_aligned_kernel: pixels in front of the row's first 128-byte boundary"""
    return ((-address) % ALIGN) // 4


def row_shifts(row, base_mod_128=0):
    """the set of per-row shifts of an ALIGNED_CASES entry"""
    return {shift_of(a) for _, _, a in row_addresses(row, base_mod_128)}


def wave_position(wave_x0, width):
    """where a wave lies in its row by the unshifted lane map: "first" (column 0), "last" (it holds column width - 1) or
    "middle"; None: right of the frame (the padding of the last tile)"""
    if wave_x0 >= width:
        return None
    if wave_x0 == 0:
        return "first"
    return "last" if wave_x0 + WAVE_PX >= width else "middle"


def edge_wave_sides(row, base_mod_128=0):
    """{(position, side)} over every row and wave of an ALIGNED_CASES entry whose wave_x = wave_x0 + s is > 0: side is
    "below" / "equal" / "above" for wave_x + 256 <, ==, > width.  The kernel takes its edge-free path exactly for
    "below".  ("last", "below") cannot occur: wave_x0 + 256 >= width there.)"""
    w = row[0]
    out = set()
    for s in row_shifts(row, base_mod_128):
        for wave_x0 in range(0, w, WAVE_PX):
            wave_x = wave_x0 + s
            if wave_x > 0:
                end = wave_x + WAVE_PX
                out.add((wave_position(wave_x0, w), "below" if end < w else "equal" if end == w else "above"))
    return out


# -- staging, halo, rows ---------------------------------------------------------------------------------------------

def wlimit4(w):
    return (w + 3) & ~3


def tail_chunk(w, tile_w):
    """the last chunk of a row that holds readable bytes: (tile, chunk index inside the tile, avail); avail = 16 stands
    for every full chunk (>= 16 takes the 16-byte load)"""
    last = (wlimit4(w) - 1) // CHUNK * CHUNK            # column of that chunk
    return last // tile_w, (last % tile_w) // CHUNK, min(wlimit4(w) - last, 16)


def right_halo_readable(w, tile_w, tile=0):
    """the halo loop's `col < wlimit4` for the dword right of a tile"""
    return (tile + 1) * tile_w < wlimit4(w)


def tile_position(w, tile_w):
    """last_group () in the terms of a tile shape: the tile, the wave inside it and the lane of the last group"""
    g = last_group(w)
    per_tile = tile_w // WAVE_PX
    return {"tile": g["wave"] // per_tile, "wave": g["wave"] % per_tile, "lane": g["lane"], "full": g["full"]}


def dn_last(h):
    """the source row that stands in for row h (fill_params: height >= 4 ? height - 4 : 1)"""
    return h - 4 if h >= 4 else 1


def wave_nrows(h, tile_h):
    """`nrows` of every wave of the last tile row: rows of the wave inside the frame (<= 0: none; a march is 4 rows)"""
    ty = (h - 1) // tile_h
    return [h - (ty * tile_h + r0) for r0 in range(0, tile_h, ROWS_PER_WAVE)]


# -- block orders ----------------------------------------------------------------------------------------------------

def plan_geometry(w, h, frames, name, band):
    """(tiles_x, tile_rows, effective band, grid blocks): fill_params and grid_blocks_for (csrc/mibayer_internal.h),
    restated; the GPU test compares it with mibayer_launch_geometry"""
    shape = shape_of(name)
    tiles_x = -(-w // shape.tile_w)
    tile_rows = frames * -(-h // shape.tile_h)
    if band < 0:
        band = -(-tile_rows // NUM_XCD)
    if band <= 0:
        return tiles_x, tile_rows, band, tile_rows * tiles_x
    group = NUM_XCD * band
    return tiles_x, tile_rows, band, -(-tile_rows // group) * group * tiles_x
