"""TEST INFRASTRUCTURE: the case tables of the statistics-kernel geometry tests (tests/test_gpu_stats_geometry.py), the
frame builders they share and a mirror of the kernel's LAUNCH GEOMETRY.  No GPU and no library here:
tests/test_stats_cases.py asserts, from these tables and the mirror alone, that the shapes reach the branches they are
meant to reach.  The mirror is not a second model of the statistics: tests/stats_model.py stays the only one.

mosaic_stats_kernel (csrc/mibayer_kernels.hip): a workgroup is 256 lanes = four waves side by side on one strip of 256
dwords of a row (four 8-bit or two 16-bit samples per dword), walking at most SEG_ROWS rows of ONE zone row:
blockIdx.y = zy * segs + seg, blockIdx.x = frame * strips + strip.  The rows of a segment go through a loop unrolled
AHEAD rows deep, then a pair at a time, the last pair possibly a single row.  Each lane adds what it has into an LDS
table of MAX_ZONES zone columns x 4 sites, one entry per lane of the workgroup."""
import collections

import numpy as np

import stats_model as sm

SEG_ROWS = 64                   # kStatsSegRows
AHEAD = 8                       # kStatsAhead: rows of one unrolled iteration
WAVE_DWORDS = 64                # dwords of a row that one wave reads
STRIP_DWORDS = 256              # ... and one workgroup
MAX_ZONES = 64                  # kStatsMaxZones

Geometry = collections.namedtuple("Geometry", "ch cw segs row_dwords strips")
Segment = collections.namedtuple("Segment", "zy seg y0 y1 full pairs single")


def vmax_of(bits):
    return (1 << (bits or 8)) - 1


def geometry(W, H, bits, zones_x, zones_y):
    """what stats_params (csrc/mibayer_abi.hip) and launch_stats compute, in their integer arithmetic; bits = 0: the
    8-bit mosaic"""
    ch = 2 * (((H + 1) // 2 + zones_y - 1) // zones_y)
    cw = 2 * ((W // 2 + zones_x - 1) // zones_x)
    row_dwords = (W + 3) // 4 if bits == 0 else W // 2
    strips = (row_dwords + STRIP_DWORDS - 1) // STRIP_DWORDS
    return Geometry(ch, cw, (ch + SEG_ROWS - 1) // SEG_ROWS, row_dwords, strips)


def segments(H, zones_y, geo):
    """every (zy, seg) of the grid's y axis: the row span [y0, y1) as the kernel clamps it (y1 <= y0: the workgroup
    returns at once), the full AHEAD-row iterations, the row pairs of the tail and whether one single row is left"""
    out = []
    for zy in range(zones_y):
        for seg in range(geo.segs):
            y0 = zy * geo.ch + seg * SEG_ROWS
            y1 = max(min(y0 + SEG_ROWS, (zy + 1) * geo.ch, H), y0)
            rest = (y1 - y0) % AHEAD
            out.append(Segment(zy, seg, y0, y1, (y1 - y0) // AHEAD, rest // 2, rest % 2 == 1))
    return out


def rows(seg):
    return seg.y1 - seg.y0


def last_segments(H, zones_y, geo):
    """the last non-empty segment of every non-empty zone row that has more than one"""
    out = []
    for zy in range(zones_y):
        live = [s for s in segments(H, zones_y, geo) if s.zy == zy and rows(s) > 0]
        if len(live) > 1:
            out.append(live[-1])
    return out


def samples_per_dword(bits):
    return 4 if bits == 0 else 2


def zone_seam_dwords(W, bits, geo):
    """the dwords of a row at which a new zone column starts"""
    return [x // samples_per_dword(bits) for x in range(geo.cw, W, geo.cw)]


# -- the tables ----------------------------------------------------------------------------------------------------

# one zone column of random data; two sample formats (W, bits, big_endian) at the same padded stride
SEG_FORMATS = ((66, 0, False), (34, 12, False))
SEG_STRIDE = 68 + 12
SEG_CASES = ((64, 1), (65, 1), (66, 1), (67, 1), (70, 1), (72, 1), (74, 1), (129, 1), (193, 1),
             (134, 2), (200, 3), (199, 3))                      # (H, zones_y)
# (lo, hi) per bits.  lo = 0: a row that is not there, read as zeroes, would be counted; lo > 0: all three outcomes
SEG_RANGES = {0: ((0, 239), (16, 255)), 12: ((0, 3839), (256, 4095))}

BATCH_HEIGHT = 5
BATCH_CASES = ((1026, 0, 3), (2050, 0, 2), (514, 16, 3))        # (W, bits, frames)
BATCH_ZONES = ((1, 1), (5, 2))
BATCH_PITCH_EXTRA = 64

# (W, H, bits, zones_x, zones_y)
ZONE_CASES = ((128, 128, 0, 64, 64), (128, 6, 16, 64, 3), (512, 6, 0, 2, 1), (2048, 6, 0, 2, 1),
              (256, 6, 12, 2, 1), (1024, 6, 12, 2, 1))


def zone_range(bits):
    """lo = 0, so that every sample is counted or clipped: no table entry that a sample reaches stays zero"""
    v = vmax_of(bits)
    return 0, v - v // 4


DEEP_BITS = (10, 12, 14, 16)
DEEP_SIZE = (130, 18)
DEEP_ZONES = (3, 2)


def deep_ranges(bits):
    v = vmax_of(bits)
    return ((0, 0), (v, v), (v // 2, v // 2), (1, v - 1))


SITE_SIZE = (520, 520)
SITE_PLANES = (65535, 65534, 32769, 3)                          # site s = 2 (y & 1) + (x & 1)


def case_seed(*key):
    """a seed of a case's own"""
    return [int(k) for k in key]


# -- frames --------------------------------------------------------------------------------------------------------

def row_bytes(W, bits):
    return 2 * W if bits else (W + 3) & ~3


def pack_words(words, bits, big_endian, stride=None, pad=0xFF):
    """(H, W) 16-bit words -> (H, stride) bytes in the given byte order, `pad` in the row padding"""
    H, W = words.shape
    raw = np.full((H, stride or 2 * W), pad, np.uint8)
    raw[:, :2 * W] = words.astype(">u2" if big_endian else "<u2").view(np.uint8).reshape(H, 2 * W)
    return raw


def random_frame(rng, W, H, bits, big_endian=False, stride=None, pad=0xFF):
    """(H, stride) bytes of a random frame: an 8-bit mosaic (bits = 0), or 16-bit words whose bits above `bits` are
    random junk (it must be ignored)"""
    if bits == 0:
        raw = np.full((H, stride or row_bytes(W, 0)), pad, np.uint8)
        raw[:, :W] = rng.integers(0, 256, (H, W))
        return raw
    return pack_words(rng.integers(0, 1 << 16, (H, W)).astype(np.uint16), bits, big_endian, stride, pad)


def samples(raw, W, H, bits, big_endian=False):
    return sm.samples(raw, W, H, raw.shape[1], bits, big_endian)


def planted(bits, lo, hi):
    """lo - 1, lo, hi and hi + 1 where the sample range has them"""
    return sorted({v for v in (lo - 1, lo, hi, hi + 1) if 0 <= v <= vmax_of(bits)})


def deep_range_frame(bits, big_endian, lo, hi):
    """a random DEEP_SIZE frame whose first row starts with planted(bits, lo, hi), each under all-ones junk above
    `bits`"""
    W, H = DEEP_SIZE
    rng = np.random.default_rng(case_seed(bits, big_endian, lo, hi))
    words = rng.integers(0, 1 << 16, (H, W)).astype(np.uint16)
    plant = planted(bits, lo, hi)
    junk = (0xFFFF << bits) & 0xFFFF
    words[0, :len(plant)] = [v | junk for v in plant]
    return pack_words(words, bits, big_endian)


def site_frame():
    """SITE_SIZE 16-bit little-endian, every site constant at its SITE_PLANES value"""
    W, H = SITE_SIZE
    yy, xx = np.mgrid[0:H, 0:W]
    return pack_words(np.asarray(SITE_PLANES, np.uint16)[2 * (yy & 1) + (xx & 1)], 16, False)


def seg_frame(fmt, H, zones_y):
    W, bits, big_endian = fmt
    return random_frame(np.random.default_rng(case_seed(W, bits, H, zones_y)), W, H, bits, big_endian, SEG_STRIDE)


def batch_frames(W, bits, frames):
    """(frames, pitch) bytes: each frame from a seed of its own, the pitch BATCH_PITCH_EXTRA bytes (of 0xFF) longer than
    the frame; and the frames alone as a list of (H, stride)"""
    raws = [random_frame(np.random.default_rng(case_seed(W, bits, f)), W, BATCH_HEIGHT, bits) for f in range(frames)]
    padded = np.full((frames, raws[0].size + BATCH_PITCH_EXTRA), 0xFF, np.uint8)
    for f, raw in enumerate(raws):
        padded[f, :raw.size] = raw.reshape(-1)
    return padded, raws


def zone_frame(W, H, bits, zones_x, zones_y):
    return random_frame(np.random.default_rng(case_seed(W, H, bits, zones_x, zones_y)), W, H, bits)
