"""TEST INFRASTRUCTURE: the case tables of the rgb2bayer geometry tests (tests/test_gpu_r2b_geometry.py), the frame
builder they share and a mirror of the LAUNCH DECISIONS of the inverse direction.  No GPU and no library here:
tests/test_r2b_cases.py asserts, from these tables and the mirror alone, that the shapes reach the seams they are meant
to reach.  The mirror is not a second model of the conversion: oracle/bayer2rgb_np.rgb2bayer stays the only one.

rgb2bayer_flat_kernel (csrc/mibayer_kernels.hip): the batch (or every frame of a list) is one sequence of ITEMS of 4
pixels = 16 bytes in, one dword out; a row has out_dwords = ROUND_UP_4 (width) / 4 of them, the last one PARTIAL when
width % 4 != 0.  A thread keeps K GROUPS of PX / 4 adjacent items in flight, group k of thread t of block b starting at
item (b * 256 K + k * 256 + t) * PX / 4.  rgb2bayer_kernel (the tile kernel): a block is R rows x 256 dwords, tile rows
run through the whole batch, and a lane finds (frame, y) of its k-th row by walking frames from (frame, y) of the tile
row's first row.  launch_flat / launch_rgb2bayer / launch_rgb2bayer_list and the c->inverse arm of launch_frames
(csrc/mibayer_abi.hip) decide vec16, dst8, px and the grid."""
import collections
import itertools

import numpy as np

from oracle import bayer2rgb_np

WAVE_ITEMS = 64                 # a wave covers 64 consecutive items per group
BLOCK_THREADS = 256             # __launch_bounds__ (256), both kernels
Shape = collections.namedtuple("Shape", "K PX LD")
PRODUCTION = Shape(2, 4, 1)     # r2b_flat_k, r2b_flat_px, r2b_flat_ld of mibayer_ctx; R2B_FLAT (2, 4, 1)
LAB_SHAPES = tuple(Shape(k, px, ld) for k in (1, 2, 3, 4, 8) for px in (4, 8) for ld in (0, 1))    # flat_kernel_for
TILE_ROWS = (2, 4, 8, 16)       # R2B_ROWS of the R2B_LAUNCH table; the product build carries 2
TILE_DWORDS = 256               # xd = tile.tx * 256 + threadIdx.x: 1024 pixels
MAX_LIST = 16                   # kMaxList
BAND_UNIT = 16                  # kInverseBandUnit
BAND_MIN_BYTES = 16 << 20       # choose_host_bands: smaller frames are not banded

ORDERS = ("bggr", "gbrg", "grbg", "rggb")
TRIPLES = tuple(itertools.permutations(range(4), 3))    # every (r_off, g_off, b_off) validate () accepts

# one launch's frames: strides and pitches 0 = the defaults; *_off = the base pointer's residue mod 16 (a batch), or one
# residue per frame (a list)
Geometry = collections.namedtuple("Geometry", "w h n src_stride dst_stride src_pitch dst_pitch src_off dst_off")
Launch = collections.namedtuple("Launch", "vec16 dst8 px fallback per_block items blocks")
Tile = collections.namedtuple("Tile", "tiles_x tile_rows walk last_tile_dwords")


def geometry(w, h, n=1, src_stride=0, dst_stride=0, src_pitch=0, dst_pitch=0, src_off=0, dst_off=0):
    return Geometry(w, h, n, src_stride, dst_stride, src_pitch, dst_pitch, src_off, dst_off)


def shape_id(shape):
    return "K%d_PX%d_LD%d" % shape


def round_up_4(w):
    return (w + 3) & ~3


def out_dwords(w):
    return round_up_4(w) // 4


def resolved(g):
    """g with the defaults of validate () and Context.process_device filled in"""
    ss = g.src_stride or 4 * g.w
    ds = g.dst_stride or round_up_4(g.w)
    return g._replace(src_stride=ss, dst_stride=ds, src_pitch=g.src_pitch or ss * g.h, dst_pitch=g.dst_pitch or ds * g.h)


def _residues(off, n):
    return [off] * n if np.ndim(off) == 0 else list(off)


# -- the mirror ---------------------------------------------------------------------------------------------------------

def vec16_terms(g, is_list=False):
    """(width, stride, pointer or pitch): the three predicates of `vec16` in launch_frames; FrameSet::on_grid for the
    third -- the pitch of a single frame does not count"""
    g = resolved(g)
    if is_list:
        grid = all(r % 16 == 0 for r in _residues(g.src_off, g.n))
    else:
        grid = g.src_off % 16 == 0 and (g.n == 1 or g.src_pitch % 16 == 0)
    return g.w % 4 == 0, g.src_stride % 16 == 0, grid


def dst8(g, is_list=False):
    """launch_rgb2bayer: the pitch and the base pointer (of one frame too); a list: FrameSet::dsts8, every pointer"""
    g = resolved(g)
    if is_list:
        return all(r % 8 == 0 for r in _residues(g.dst_off, g.n))
    return g.dst_pitch % 8 == 0 and g.dst_off % 8 == 0


def launch(shape, g, is_list=False):
    """launch_flat: what a launch of the flat kernel over g runs as.  items / blocks: of the batch, or of one frame of a
    list (every frame takes a whole number of blocks)"""
    r = resolved(g)
    vec16 = all(vec16_terms(g, is_list))
    d8 = dst8(g, is_list)
    od = out_dwords(g.w)
    fallback = ()
    if shape.PX == 8:
        fallback = tuple(name for name, hit in (("odd_dwords", od & 1), ("dst_stride", r.dst_stride & 7),
                                                ("dst8", not d8), ("vec16", not vec16)) if hit)
    px = 8 if shape.PX == 8 and not fallback else 4
    per_block = BLOCK_THREADS * shape.K * (px // 4)
    items = g.h * od * (1 if is_list else g.n)
    return Launch(vec16, d8, px, fallback, per_block, items, -(-items // per_block))


def list_goes_frame_by_frame(flat_k, w, h):
    """launch_frames: the tile kernel has no frame table, nor has a frame beyond the 32-bit item index"""
    return flat_k <= 0 or h * out_dwords(w) > 0x7fffffff


def list_chunks(n):
    """mibayer_process_device_list: launches of at most kMaxList frames"""
    return [min(MAX_LIST, n - f0) for f0 in range(0, n, MAX_LIST)]


def item_position(item, w, h, is_list=False):
    """(frame, y, xd, partial) of an item; in a list launch items count inside the block's own frame"""
    row, xd = divmod(item, out_dwords(w))
    f, y = (0, row) if is_list else divmod(row, h)
    return f, y, xd, 4 * xd + 3 >= w


def group_items(shape, g, block, thread, is_list=False):
    """the items of the K groups of one thread, those below item_end"""
    L = launch(shape, g, is_list)
    ipg = L.px // 4
    first = (block * BLOCK_THREADS * shape.K + thread) * ipg
    return [[i for i in range(first + k * BLOCK_THREADS * ipg, first + k * BLOCK_THREADS * ipg + ipg) if i < L.items]
            for k in range(shape.K)]


def block_frames(shape, g, block):
    """the frames a block of a batch launch has items in"""
    L = launch(shape, g)
    lo, hi = block * L.per_block, min((block + 1) * L.per_block, L.items)
    return sorted({item_position(i, g.w, g.h)[0] for i in (lo, hi - 1)} | {
        f for f in range(g.n) if lo <= f * g.h * out_dwords(g.w) < hi})


def tile(R, w, h, n):
    """launch_rgb2bayer's tile kernel: tiles per row, tile rows of the batch, the largest number of steps the frame
    walk `while (y >= p.height)` takes, the dwords of the last tile of a row"""
    od = out_dwords(w)
    total = n * h
    walk = max(((t * R) % h + k) // h for t in range(-(-total // R)) for k in range(R) if t * R + k < total)
    return Tile(-(-od // TILE_DWORDS), -(-total // R), walk, od - (-(-od // TILE_DWORDS) - 1) * TILE_DWORDS)


def host_bands(want, src_bytes, h):
    """choose_host_bands for the inverse direction: how many bands of BAND_UNIT-row units a frame is cut into"""
    if want < 2 or src_bytes < BAND_MIN_BYTES:
        return 1
    units = -(-h // BAND_UNIT)
    while want > 1:
        per = -(-units // want)
        nb = -(-units // per)
        if nb == want and per * BAND_UNIT >= 8 and h - (nb - 1) * per * BAND_UNIT >= 4:
            return want
        want -= 1
    return 1


# -- frames and what they convert to ------------------------------------------------------------------------------------

def frames(key, g):
    """n frames of (h, src_stride) random bytes, row padding included, each frame from a generator of its own so that
    no two are equal"""
    r = resolved(g)
    return [np.random.default_rng([int(k) for k in key] + [r.w, r.h, f]).integers(0, 256, (r.h, r.src_stride), np.uint8)
            for f in range(r.n)]


def expect(frame, w, order, triple):
    """(h, w) mosaic of one (h, src_stride) frame: the NumPy restatement of the reference loop"""
    h = frame.shape[0]
    return bayer2rgb_np.rgb2bayer(frame[:, :4 * w].reshape(h, w, 4), order, *triple).astype(np.uint8)


def rotate(i):
    """(order, triple) of case i: the orders go round every 4 cases, the triples every 24"""
    return ORDERS[i % 4], TRIPLES[(i + i // 4) % 24]


# -- the tables -----------------------------------------------------------------------------------------------------------

# every width % 4 at: below one item; around one wave's 64 items; around the tile kernel's 256-dword tile; around one
# production block (512 items)
WIDTHS_ITEM = (1, 2, 3)
WIDTHS_WAVE = (254, 255, 256, 257, 258, 259)
WIDTHS_TILE = tuple(range(1020, 1031))
WIDTHS_BLOCK = (2045, 2046, 2047, 2048, 2049, 2050, 2051)
WIDTHS = WIDTHS_ITEM + WIDTHS_WAVE + WIDTHS_TILE + WIDTHS_BLOCK
HEIGHTS = (1, 2, 3)
STRIDE_PAD = 12                 # src_stride = 4 w + 12, dst_stride = ROUND_UP_4 (w) + 12: never vec16


def sweep_cases(widths=WIDTHS):
    return [geometry(w, h) for w in widths for h in HEIGHTS]


def padded(g):
    return g._replace(src_stride=4 * g.w + STRIDE_PAD, dst_stride=round_up_4(g.w) + STRIDE_PAD)


def _factor(total, even_dwords):
    """(out_dwords, h, n) with out_dwords * h * n == total: several frames and an odd height where total allows"""
    for n, h in itertools.product((3, 2, 5, 7, 1), (3, 5, 7, 9, 1, 2, 4)):
        od, rest = divmod(total, n * h)
        if rest == 0 and od >= 1 and not (even_dwords and od & 1):
            return od, h, n
    raise ValueError(total)


def seam_steps(shape):
    """the distances from a whole number of blocks that the item count of a launch can have: one item, or with two
    items per group (PX = 8 holds only where out_dwords is even, so every count is even) one group"""
    return (-(shape.PX // 4), 0, shape.PX // 4)


def seam_cases(shape):
    """(w, h, n) whose item count is one step under, exactly, and one step over one block and two blocks of `shape`;
    width % 4 rotates where PX = 4 (PX = 8 needs vec16: width % 4 == 0)"""
    per_block = BLOCK_THREADS * shape.K * (shape.PX // 4)
    out = []
    for i, (blocks, step) in enumerate(itertools.product((1, 2), seam_steps(shape))):
        od, h, n = _factor(blocks * per_block + step, shape.PX == 8)
        out.append(geometry(4 * od - (0 if shape.PX == 8 else i % 4), h, n))
    return out


# batches of 2 to 5 odd-height frames: a block with frame boundaries inside, K-groups across rows and across frames
ODD_BATCHES = (geometry(50, 3, 2), geometry(50, 3, 3), geometry(50, 3, 4), geometry(50, 7, 5), geometry(1021, 3, 3),
               geometry(259, 5, 2))

# PX = 8: no fall-back, and one case for each of the four reasons alone
PX8_CASES = collections.OrderedDict((
    ("none", geometry(16, 3, 2)),
    ("odd_dwords", geometry(20, 3, 2, src_stride=96, dst_stride=24)),
    ("dst_stride", geometry(16, 3, 2, dst_stride=20, dst_pitch=64)),
    ("dst8", geometry(16, 3, 2, dst_off=4)),
    ("vec16", geometry(16, 3, 2, src_off=4)),
))

# vec16: each predicate false alone, and all true; n = 1 with a pitch off the grid still vec16
VEC16_CASES = collections.OrderedDict((
    ("all", (geometry(16, 3, 3), (True, True, True))),
    ("width", (geometry(18, 3, 3, src_stride=80), (False, True, True))),
    ("stride", (geometry(16, 3, 3, src_stride=76, src_pitch=240), (True, False, True))),
    ("pointer", (geometry(16, 3, 3, src_off=8), (True, True, False))),
    ("pitch", (geometry(16, 3, 3, src_pitch=196), (True, True, False))),
    ("pitch_of_one_frame", (geometry(16, 3, 1, src_pitch=196), (True, True, True))),
))

# pitches: src_frame_bytes = src_bytes + ..., dst_frame_bytes = dst_bytes + ...
SRC_PITCH_EXTRA = (4, 16, 20)
DST_PITCH_EXTRA = (4, 8, 12)
PITCH_FRAMES = (geometry(1024, 3, 3), geometry(1023, 3, 3))     # 768 items a frame: the frames end inside blocks


def pitch_cases(n):
    out = []
    for g in PITCH_FRAMES:
        r = resolved(g._replace(n=n))
        out += [r._replace(src_pitch=r.src_pitch + s, dst_pitch=r.dst_pitch + d)
                for s in SRC_PITCH_EXTRA for d in DST_PITCH_EXTRA]
    return out


# alignment: source at 0 / 4 / 8 / 12, destination at 0 / 4; w % 4 == 0 across a block seam (520 items), w % 4 == 3
ALIGN_FRAMES = (geometry(1040, 2, 1), geometry(1043, 2, 1))
ALIGN_OFFSETS = tuple(itertools.product((0, 4, 8, 12), (0, 4)))

# lists
LIST_SIZES = (1, 2, 16, 17, 33)
LIST_OFFSET_FRAMES = (5, 20)    # the frame that sits at + 4: one of the first chunk, one of the second


def list_frame(shape):
    """a frame of two blocks of `shape`, the second partial: out_dwords = 258, partial items where PX = 4"""
    per_block = BLOCK_THREADS * shape.K * (shape.PX // 4)
    return geometry(1032 if shape.PX == 8 else 1030, -(-3 * per_block // 2 // 258))


LIST_ALIGNED_WIDTH = 1032       # w % 4 == 0: a source at + 4 is what takes vec16 away


# the tile kernel, per rows-per-block R: the whole width sweep (WIDTHS_BLOCK takes a row from two tiles to three), and
# n h at -1, 0, +1 mod R around the 257th dword (the last tile holds one); odd-height frames shorter than R; the frame
# walk at its longest (h = 1, n = 40)
def tile_cases(R):
    return [geometry(1026, 2 * R - 1), geometry(1026, 2 * R), geometry(1026, 2 * R + 1), geometry(1026, 3, 5),
            geometry(5, 1, 40)]


TILE_BANDS = (-1, 0, 1, 3)      # MIBAYER_XCD_BAND

# the banded host path: the smallest frame that bands, odd height, out_dwords = 257; PX = 8 holds at 1032
BANDED_FRAME = geometry(1028, 4101)
BANDED_FRAME_PX8 = geometry(1032, 4101)
HOST_BANDS = (3, 8)             # MIBAYER_HOST_BANDS

SELECTOR_SIZES = (geometry(6, 3), geometry(1, 1))
