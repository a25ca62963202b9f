"""TEST INFRASTRUCTURE: the case tables of the strip-kernel tests (tests/test_gpu_strip_geometry.py) and the frame
builders they share.  No GPU and no library here: tests/test_strip_cases.py asserts, from these tables and the NumPy
models alone, that the widths, heights, frames and colour stages reach the branches they are meant to reach.

The strip kernels (csrc/mibayer_kernels.hip): a lane owns a group of 4 pixels, a wave a strip of 64 groups = 256 pixels
x STRIP_ROWS rows.  The last group of a row is full (width % 4 == 0) or a 2-pixel tail (width % 4 == 2); the 8-byte
pixel store swaps 16-byte pieces inside a quad of lanes, so which of its predicates bite depends on the last group's
lane & 3 and on full / tail: together width % 16.  Lanes 0 and 63 of a wave load their own edge samples, every other
lane takes them from its neighbours: the seam between two strips is a path of its own."""
import collections

import numpy as np

import colour_model as cm
import highbit_model as hm
import mhc_model as mm

STRIP_ROWS = 16                 # kStripRows
STRIP_GROUPS = 64               # lanes of a wave = 4-pixel groups of a strip
MAX_LIST = 16                   # kMaxList: frames of one list launch

ORDERS = ("bggr", "gbrg", "grbg", "rggb")
LAYOUT8 = ("RGBx", "BGRx", "xRGB", "xBGR")
LAYOUT16 = ("RGBA64", "BGRA64", "ARGB64", "ABGR64")

# bits = 0: the 8-bit mosaic (in8); colour: the fused colour kernel (one kernel, run-time arms) instead of the plain one
Arm = collections.namedtuple("Arm", "name method bits out16 colour")

# the 7 non-null entries of kStripKernels[mhc][in8][out16]
PLAIN_ARMS = (
    Arm("deep_10_to_8", "bilinear", 10, False, False),
    Arm("deep_14_to_16", "bilinear", 14, True, False),
    Arm("deep_8_to_16", "bilinear", 0, True, False),
    Arm("mhc_12_to_8", "mhc", 12, False, False),
    Arm("mhc_16_to_16", "mhc", 16, True, False),
    Arm("mhc_8_to_8", "mhc", 0, False, False),
    Arm("mhc_8_to_16", "mhc", 0, True, False),
)
# the 8 run-time arms of bayer2rgb_colour_kernel: mhc x in8 x out16
COLOUR_ARMS = (
    Arm("colour_bilinear_12_to_8", "bilinear", 12, False, True),
    Arm("colour_bilinear_16_to_16", "bilinear", 16, True, True),
    Arm("colour_bilinear_8_to_8", "bilinear", 0, False, True),
    Arm("colour_bilinear_8_to_16", "bilinear", 0, True, True),
    Arm("colour_mhc_10_to_8", "mhc", 10, False, True),
    Arm("colour_mhc_14_to_16", "mhc", 14, True, True),
    Arm("colour_mhc_8_to_8", "mhc", 0, False, True),
    Arm("colour_mhc_8_to_16", "mhc", 0, True, True),
)
ARMS = PLAIN_ARMS + COLOUR_ARMS


def strip_index(arm):
    """(mhc, in8, out16): the index into kStripKernels, and the run-time arm of the colour kernel"""
    return arm.method == "mhc", arm.bits == 0, arm.out16


# every residue mod 16 inside one wave; the last group in lanes 63, 0, 1, 2, 3 around the first seam, full and tail
# (272: lane 3 full, the one position 254 .. 270 leave out); a second seam with residues 10 and 12 behind it
WIDTHS = (20, 22, 24, 26, 28, 30, 32, 34,
          254, 256, 258, 260, 262, 264, 266, 268, 270, 272,
          510, 516, 522, 524)
# one short of a chunk, exactly one, one and two rows over -- at one chunk and at two; 3 and 4: the smallest frames
HEIGHTS = (3, 4, 15, 16, 17, 18, 31, 32, 33, 34)
SWEEP_HEIGHT = 18               # the height of the width sweep
SWEEP_WIDTHS = (266, 268)       # the widths of the height sweep: residues 10 and 12, behind the seam
# one width of each residue mod 16, all of them across the seam: converted from the weakest base-pointer alignment
ALIGN_WIDTHS = (254, 256, 258, 260, 262, 264, 266, 268)


def last_group(width):
    """where a row ends: the wave and lane that hold its last group, and whether that group is full or the tail"""
    g = (width + 3) // 4 - 1
    return {"wave": g // STRIP_GROUPS, "lane": g % STRIP_GROUPS, "full": width % 4 == 0}


Case = collections.namedtuple("Case", "w h order layout sbe dbe")


def rotate(arm, i, w, h):
    """case i of an arm: Bayer order, layout and both byte orders rotate with the index, at different periods"""
    layouts = LAYOUT16 if arm.out16 else LAYOUT8
    return Case(w, h, ORDERS[i % 4], layouts[(i // 4 + i) % 4], bool(arm.bits) and (i // 3) % 2 == 1,
                arm.out16 and (i // 5) % 2 == 1)


def geometry_cases(arm):
    """the two sweeps of an arm: every width at SWEEP_HEIGHT, every height at SWEEP_WIDTHS"""
    sizes = [(w, SWEEP_HEIGHT) for w in WIDTHS] + [(w, h) for w in SWEEP_WIDTHS for h in HEIGHTS]
    return [rotate(arm, i, w, h) for i, (w, h) in enumerate(sizes)]


def alignment_cases(arm):
    return [rotate(arm, 3 * i + 1, w, SWEEP_HEIGHT) for i, w in enumerate(ALIGN_WIDTHS)]


# -- frames --------------------------------------------------------------------------------------------------------

def depth_of(bits):
    return bits or 8


def src_row_bytes(w, bits):
    return 2 * w if bits else (w + 3) & ~3


def frame_bytes(S, bits, rng, stride=None, big_endian=False):
    """(h, w) samples -> the frame's bytes (h, stride): an 8-bit mosaic (bits = 0), or 16-bit words with random junk
    above `bits` (it must be ignored); the row padding is 0x5A"""
    S = np.asarray(S)
    h, w = S.shape
    stride = stride or src_row_bytes(w, bits)
    if not bits:
        buf = np.full((h, stride), 0x5A, np.uint8)
        buf[:, :w] = S
        return buf
    words = S | (rng.integers(0, 1 << 16, (h, w)) & ~((1 << bits) - 1) & 0xFFFF)
    buf = hm.pack(words, stride, big_endian)
    buf[:, 2 * w:] = 0x5A
    return buf


def random_frame(rng, w, h, bits, stride=None, big_endian=False):
    return frame_bytes(rng.integers(0, 1 << depth_of(bits), (h, w)), bits, rng, stride, big_endian)


def plane_frames(w, h, depth):
    """16 frames: each of the four Bayer sites constant 0 or 2^depth - 1, in all 2^4 combinations (frame n: site
    (y & 1, x & 1) is at its maximum when bit 2 (y & 1) + (x & 1) of n is set)"""
    vmax = (1 << depth) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    site = 2 * (yy & 1) + (xx & 1)
    return [((n >> site) & 1) * vmax for n in range(16)]


def pattern_frames(w, h, depth):
    """9 frames: constant 0, constant max, column stripes of period 1 and 2, row stripes of period 1 and 2, a single
    max impulse at (0, 0) and one at (h-1, w-1) on zero -- and two 3x3 blocks of max on zero, centred on sites of either
    parity of y + x: the only frame of the two sets that takes F_G and F_diag ABOVE the range (centre and the +-1
    neighbours at max, the +-2 ones at 0), which stripes, impulses and constant planes cannot"""
    vmax = (1 << depth) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    first, last, blocks = (np.zeros((h, w), np.int64) for _ in range(3))
    first[0, 0] = vmax
    last[h - 1, w - 1] = vmax
    blocks[4:7, 5:8] = vmax                 # centre (5, 6)
    blocks[10:13, 20:23] = vmax             # centre (11, 21)
    return [np.zeros((h, w), np.int64), np.full((h, w), vmax, np.int64),
            (xx & 1) * vmax, ((xx >> 1) & 1) * vmax, (yy & 1) * vmax, ((yy >> 1) & 1) * vmax, first, last, blocks]


PLANE_SIZE = (266, 18)          # the 16 plane frames: one batch launch, and once more as a list of MAX_LIST frames
PATTERN_SIZE = (34, 17)         # the 9 pattern frames


def extreme_cases():
    """section B: (arm, bits).  The plain arms at depths 8 (in8), 10 and 16; both methods of the colour kernel, each
    of its in8 x out16 arms once, with the identity matrix and the linear tone curve"""
    out = []
    for arm in PLAIN_ARMS:
        for bits in ((0,) if arm.bits == 0 else (10, 16)):
            out.append(arm._replace(name="%s_to_%d@%d" % (arm.method, 16 if arm.out16 else 8, depth_of(bits)), bits=bits))
    for method in ("bilinear", "mhc"):
        for bits, out16 in ((0, False), (0, True), (10, False), (16, True)):
            out.append(Arm("colour_%s_to_%d@%d" % (method, 16 if out16 else 8, depth_of(bits)), method, bits, out16, True))
    return out


LINEAR_TONE = tuple(256 * i for i in range(257))        # MIBAYER_TONE_LINEAR


# -- colour stages at the ends of their ranges -------------------------------------------------------------------

# tone: None = no curve; junk: has_tone = 0 with these values left in the table (they must not be looked at)
Stage = collections.namedtuple("Stage", "name black matrix tone junk")

TONE_NON_MONOTONIC = tuple((i * i * 37) & 0xFFFF for i in range(256)) + (65536,)
TONE_FLAT_TOP = tuple(256 * i for i in range(200)) + (65536,) * 57
TONE_ZERO = (0,) * 257
TONE_STEP = (0,) * 128 + (65536,) * 129
TONE_JUNK = tuple((i * 2654435761 + 12345) & 0xFFFFFFFF for i in range(257))

MATRIX_PM65535 = (65535, -65535, 3, -65535, 65535, 0, 1, -1, 65535)
MATRIX_GAIN16 = (65535, 3, 0, 0, 4096, 0, 0, 0, 4096)      # row 0 on (65535, 65535, .): 65535 * 65538 > 2^32
BLACK_MAX = 65535               # mibayer_colour.black[k] is 0 .. 65535: a black level of 2^16 does not exist


def colour_stages(depth):
    """section C.  A black level of vmax + 1 exists only below depth 16 (BLACK_MAX)"""
    vmax = (1 << depth) - 1
    stages = [
        Stage("pm65535", (0, 65535, 1), MATRIX_PM65535, None, None),
        Stage("gain16", (0, 0, 0), MATRIX_GAIN16, None, None),
        Stage("black_vmax", (vmax,) * 3, cm.IDENTITY, None, None),
    ]
    if vmax + 1 <= BLACK_MAX:
        stages.append(Stage("black_vmax_plus_1", (vmax + 1,) * 3, cm.IDENTITY, None, None))
    stages += [
        Stage("tone_non_monotonic", (0, 0, 0), cm.IDENTITY, TONE_NON_MONOTONIC, None),
        Stage("tone_flat_top", (0, 0, 0), cm.IDENTITY, TONE_FLAT_TOP, None),
        Stage("tone_zero", (0, 0, 0), cm.IDENTITY, TONE_ZERO, None),
        Stage("tone_step", (0, 0, 0), cm.IDENTITY, TONE_STEP, None),
        Stage("no_tone_junk_table", (0, 0, 0), cm.IDENTITY, None, TONE_JUNK),
    ]
    return stages


# section C runs both methods on these two: (bits, out16, layout)
STAGE_IO = ((0, False, "BGRx"), (16, True, "ARGB64"))
STAGE_SIZE = (266, 18)


def stage_frames(rng, bits):
    """a random frame and the constant-max frame, as samples"""
    w, h = STAGE_SIZE
    depth = depth_of(bits)
    return [rng.integers(0, 1 << depth, (h, w)), np.full((h, w), (1 << depth) - 1, np.int64)]


# -- expectations ------------------------------------------------------------------------------------------------

def native_rgb(arm, S, order):
    """(h, w) samples -> (h, w, 3) demosaiced values at the native depth, by the arm's method"""
    if arm.method == "mhc":
        return mm.native_rgb(S, order, depth_of(arm.bits))
    return hm.native_rgb(S, order)


def expect(arm, buf, case, stride=None, **stage):
    """the model's output rows (bytes) of frame `buf` for an arm and a case; stage: black= / matrix= / tone= of a
    colour arm"""
    stride = stride or buf.shape[1]
    if arm.colour:
        return cm.bayer2rgb_colour(buf, case.w, case.h, case.order, case.layout, bits=arm.bits, out16=arm.out16,
                                   method=arm.method, src_big_endian=case.sbe, dst_big_endian=case.dbe, stride=stride,
                                   **stage)
    assert not stage
    if arm.method == "mhc":
        return mm.bayer2rgb_mhc(buf, case.w, case.h, case.order, case.layout, bits=arm.bits, out16=arm.out16,
                                src_big_endian=case.sbe, dst_big_endian=case.dbe, stride=stride)
    return hm.bayer2rgb_highbit(buf, case.w, case.h, case.order, case.layout, depth_of(arm.bits), arm.out16,
                                case.sbe, case.dbe, stride)
