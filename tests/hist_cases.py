"""TEST INFRASTRUCTURE: the case tables of the histogram-kernel geometry tests (tests/test_gpu_hist_geometry.py), the
frame builders they share and a mirror of the kernel's LANE STATES and LAUNCH GEOMETRY.  No GPU and no library here:
tests/test_hist_cases.py asserts, from these tables and the mirror alone, that the shapes reach the branches they are
meant to reach.  The mirror is not a second model of the histogram: tests/hist_model.py stays the only one.

mosaic_hist_kernel (csrc/mibayer_kernels.hip): a lane reads one dword of a row = four 8-bit samples s0 s1 s2 s3 (two
column pairs: `in0` says whether the first lies inside the window, `in1` the second) or two deep ones (one pair, in0
alone).  Where both pairs are inside, two equal samples of one site go as one atomic of 2: e02 (s0 == s2) and e13
(s1 == s3).  A wave is WAVE_DWORDS dwords of a row, a workgroup STRIP_DWORDS (one strip); blockIdx.x = frame * strips +
strip, blockIdx.y walks the window's rows in segments of rows_per_workgroup() rows."""
import collections

import numpy as np

import hist_model as hm
import stats_model as sm

WAVE_DWORDS = 64                # dwords of a row that one wave reads
STRIP_DWORDS = 256              # ... and one workgroup
MIN_ROWS, MAX_ROWS, SPREAD = 16, 256, 512       # kHistMinRows, kHistMaxRows, kHistSpread

Case = collections.namedtuple("Case", "name W H stride win")


def resolved(W, H, win):
    """(x0, y0, x1, y1) of a window (x0, y0, w, h); (0, 0, 0, 0) is the whole frame"""
    x0, y0, w, h = hm.window(W, H, win)
    return x0, y0, x0 + w, y0 + h


def dwords(W, H, win, bits=0):
    """[g0, g1): the dwords of a row that launch_hist hands to lanes"""
    x0, _, x1, _ = resolved(W, H, win)
    return (x0 // 4, (x1 + 3) // 4) if bits == 0 else (x0 // 2, x1 // 2)


def strips(W, H, win, bits=0):
    g0, g1 = dwords(W, H, win, bits)
    return (g1 - g0 + STRIP_DWORDS - 1) // STRIP_DWORDS


def rows_per_workgroup(h, nstrips, frames):
    """the row rule of launch_hist as its comment states it: h x strips x frames / kHistSpread, clamped to
    kHistMinRows .. kHistMaxRows, rounded up to even (the re-cut past 65535 segments is out of reach here)"""
    rows = h * nstrips * frames // SPREAD
    rows = min(max(rows, MIN_ROWS), MAX_ROWS)
    return (rows + 1) & ~1


def segments(h, rows):
    """the rows each workgroup of one strip walks"""
    return [min(rows, h - y) for y in range(0, h, rows)]


def window_counts(W, H, win):
    """samples of each site inside the window, from the window alone"""
    x0, y0, x1, y1 = resolved(W, H, win)
    cols = [len(range(x0 + ((p - x0) & 1), x1, 2)) for p in (0, 1)]
    rows = [len(range(y0 + ((p - y0) & 1), y1, 2)) for p in (0, 1)]
    return [rows[s >> 1] * cols[s & 1] for s in range(4)]


def lane_tuples(raw, W, H, win):
    """the set of (in0, in1, e02, e13) over every dword of every window row of an 8-bit frame given as (H, stride)
    bytes: e02 / e13 are the plain equalities s0 == s2 / s1 == s3 of the dword as the lane loads it, row padding
    included"""
    x0, y0, x1, y1 = resolved(W, H, win)
    g0, g1 = dwords(W, H, win)
    assert 4 * g1 <= raw.shape[1]
    out = set()
    for g in range(g0, g1):
        c0 = 4 * g
        in0 = x0 <= c0 < x1
        in1 = x0 <= c0 + 2 < x1
        assert in0 or in1
        d = raw[y0:y1, c0:c0 + 4]
        for e02, e13 in {(bool(a), bool(b)) for a, b in zip(d[:, 0] == d[:, 2], d[:, 1] == d[:, 3])}:
            out.add((in0, in1, e02, e13))
    return out


def tail_dword_lane(W, H, win):
    """(strip, wave of the strip, lane of the wave) of the last dword of the window's rows"""
    g0, g1 = dwords(W, H, win)
    i = g1 - 1 - g0
    return i // STRIP_DWORDS, i % STRIP_DWORDS // WAVE_DWORDS, i % WAVE_DWORDS


def case_seed(*key):
    """a seed of a case's own"""
    return [int(k) for k in key]


# -- A1: the arms of the pair fusion --------------------------------------------------------------------------------

FAMILIES = ("ee", "en", "ne", "nn")     # s0 == s2 / s1 == s3 inside every dword: e = equal, n = not
FUSION_WIDTHS = (6, 258, 1030)          # W % 4 == 2: the tail dword in lane 1, behind a wave seam, behind a strip seam
FUSION_HEIGHTS = (5, 17)
FUSION_OUTER = 1040                     # the frame of the inner-window form
FUSION_PAD_STRIDE = 272                 # W = 258 in rows of 272 bytes


def fusion_frame(family, stride, H):
    """(H, stride) bytes, every byte of every row by its column phase: site s = 2 (y & 1) + (x & 1) holds 20 + 50 s,
    and where the family says `n` for that column parity, the second pair of the dword holds 13 more.  Nothing marks
    where a row or a window ends: an excluded pair equals its included neighbour exactly where the family says so."""
    yy, xx = np.mgrid[0:H, 0:stride]
    v = 20 + 50 * (2 * (yy & 1) + (xx & 1))
    second = (xx >> 1) & 1
    for parity in (0, 1):
        if family[parity] == "n":
            v = v + 13 * (second & ((xx & 1) == parity))
    return v.astype(np.uint8)


def fusion_cases():
    """every lane state, at every width and height: the whole frame (last dword in0 && !in1); all dwords in0 && in1;
    first dword !in0 && in1 with either kind of last dword; a 2-column window that is an in0 pair alone, one that is an
    in1 pair alone; the inner windows of a wider frame; one padded stride"""
    out = []
    for H in FUSION_HEIGHTS:
        for W in FUSION_WIDTHS:
            s = (W + 3) & ~3
            out += [Case("whole", W, H, s, (0, 0, 0, 0)),
                    Case("both", W, H, s, (0, 0, W - 2, H)),
                    Case("in1-first-in0-last", W, H, s, (2, 1, W - 2, H - 1)),
                    Case("in1-first-both-last", W, H, s, (2, 0, W - 4, H)),
                    Case("in0-pair", W, H, s, (W - 2, 0, 2, H)),
                    Case("in1-pair", W, H, s, (W - 4, 1, 2, H - 1))]
        for W in FUSION_WIDTHS[1:]:
            out += [Case("inner-in0-last", FUSION_OUTER, H, FUSION_OUTER, (0, 0, W, H)),
                    Case("inner-in1-first-in0-last", FUSION_OUTER, H, FUSION_OUTER, (2, 1, W - 2, H - 1))]
        out.append(Case("padded-stride", 258, H, FUSION_PAD_STRIDE, (0, 0, 0, 0)))
    return out


# -- A2: every value of every depth ---------------------------------------------------------------------------------

DEEP_BITS = (10, 12, 14, 16)
VALUE_SIZE = (512, 512)                 # four site planes of 256 x 256 = 65536 samples
VALUE_BIN = 256                         # 65536 samples over 256 bins
EDGE_SIZE = (128, 16)


def pack_words(words, big_endian):
    """(H, W) 16-bit words -> (H, 2 W) bytes in the given byte order"""
    H, W = words.shape
    return words.astype(">u2" if big_endian else "<u2").view(np.uint8).reshape(H, 2 * W)


def junk_above(rng, shape, bits):
    return (rng.integers(0, 1 << 16, shape) << bits) & 0xFFFF


def value_frame(bits, big_endian=False):
    """VALUE_SIZE: every site plane holds every value 0 .. 2^bits - 1 exactly 2^(16 - bits) times, shuffled; deep
    samples (bits > 8) under random junk above `bits`; bits = 8: a frame of bytes"""
    W, H = VALUE_SIZE
    rng = np.random.default_rng(case_seed(bits, big_endian))
    S = np.zeros((H, W), np.int64)
    for s in range(4):
        S[s >> 1::2, s & 1::2] = rng.permutation(np.arange(1 << 16) & ((1 << bits) - 1)).reshape(H // 2, W // 2)
    if bits == 8:
        return S.astype(np.uint8)
    return pack_words(S | junk_above(rng, S.shape, bits), big_endian)


def boundary_values(bits):
    """k << shift and (k << shift) - 1 for every bin boundary k = 1 .. 255"""
    shift = bits - 8
    return sorted({(k << shift) - d for k in range(1, 256) for d in (0, 1)})


def boundary_frame(bits, big_endian):
    """EDGE_SIZE: samples at boundary_values(bits) only, each at least once, random junk above"""
    W, H = EDGE_SIZE
    rng = np.random.default_rng(case_seed(bits, big_endian, 1))
    vals = np.asarray(boundary_values(bits))
    S = rng.permutation(np.resize(vals, W * H)).reshape(H, W)
    return pack_words(S | junk_above(rng, S.shape, bits), big_endian)


def extremes_frame(bits, big_endian):
    """EDGE_SIZE: 0 and 2^bits - 1 only, under all-ones junk"""
    W, H = EDGE_SIZE
    rng = np.random.default_rng(case_seed(bits, big_endian, 2))
    S = rng.integers(0, 2, (H, W)) * ((1 << bits) - 1)
    return pack_words(S | ((0xFFFF << bits) & 0xFFFF), big_endian)


# -- A3: frame x strip x segment x window, small --------------------------------------------------------------------

BatchCase = collections.namedtuple("BatchCase", "W H bits big_endian stride frames extra")
SPLIT_CASES = (BatchCase(1030, 35, 0, False, 1056, 3, 64), BatchCase(518, 35, 12, True, 2 * 518 + 12, 3, 64))
SPLIT_WINDOWS = {1030: ((2, 1, 1026, 33), (0, 0, 0, 0)), 518: ((2, 1, 514, 33), (0, 0, 0, 0))}
SPLIT_PAD, SPLIT_GAP = 0x5A, 0xC3       # in the row padding; between the frames
SPLIT_OFFSET = 4                        # the batch once more from a base at 4 mod 16


def random_frame(rng, W, H, bits, big_endian=False, stride=None, pad=0xFF):
    """(H, stride) bytes: random bytes, or random 16-bit words (junk above `bits` included), `pad` in the row padding"""
    row = 2 * W if bits else W
    raw = np.full((H, stride or (row + 3) & ~3), pad, np.uint8)
    if bits:
        raw[:, :row] = pack_words(rng.integers(0, 1 << 16, (H, W)).astype(np.uint16), big_endian)
    else:
        raw[:, :row] = rng.integers(0, 256, (H, W))
    return raw


def split_frames(case):
    """(frames, pitch) bytes with SPLIT_GAP between the frames, and the frames alone as a list of (H, stride)"""
    raws = [random_frame(np.random.default_rng(case_seed(case.W, case.bits, f)), case.W, case.H, case.bits,
                         case.big_endian, case.stride, SPLIT_PAD) for f in range(case.frames)]
    padded = np.full((case.frames, raws[0].size + case.extra), SPLIT_GAP, np.uint8)
    for f, raw in enumerate(raws):
        padded[f, :raw.size] = raw.reshape(-1)
    return padded, raws


def samples(raw, W, H, bits=0, big_endian=False):
    return sm.samples(raw, W, H, raw.shape[1], bits, big_endian)


def depth(bits):
    return bits or 8


# -- A4: rows per workgroup without megabytes -----------------------------------------------------------------------

# (W, H, frames) -> rows per workgroup and the rows of a frame's workgroups
ROWS_CASES = {(4, 40, 512): (40, [40]), (4, 21, 512): (22, [21]), (4, 600, 512): (256, [256, 256, 88]),
              (4, 257, 512): (256, [256, 1]), (1028, 40, 128): (20, [20, 20])}


def rows_frames(W, H, frames):
    """(frames, H, W) random bytes"""
    return np.random.default_rng(case_seed(W, H, frames)).integers(0, 256, (frames, H, W)).astype(np.uint8)


def histograms(raws):
    """(frames, 4, 256): the model over a (frames, H, W) batch of whole 8-bit frames, all at once"""
    n, H, W = raws.shape
    out = np.zeros((n, 4, hm.BINS), np.uint32)
    for s in range(4):
        v = raws[:, s >> 1::2, s & 1::2].reshape(n, -1).astype(np.int64) + hm.BINS * np.arange(n)[:, None]
        out[:, s] = np.bincount(v.reshape(-1), minlength=n * hm.BINS).reshape(n, hm.BINS)
    return out


# -- A5: a second call; the host path -------------------------------------------------------------------------------

REPEAT_CASE = ("ee", Case("whole", 258, 17, 260, (0, 0, 0, 0)))
HOST_CASE = ("en", Case("in1-first-in0-last", 258, 17, 260, (2, 1, 256, 16)))
