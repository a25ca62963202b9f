"""The case table of the noise reduction kernel's own geometry (csrc/mibayer_kernels.hip: mosaic_nr_kernel, launch_nr),
restated here so that a CPU test can say what each case reaches (tests/test_nr_cases.py) before the GPU tests
(tests/test_gpu_nr.py) run them.

The geometry is the defect pass's (tests/dpc_cases.py): a lane owns one dword of a row -- 4 samples of an 8-bit mosaic, 2
of a deep one; a wave spans 64 dwords, a workgroup 256 = one strip; a row whose width is 2 mod 4 ends, in an 8-bit
mosaic, in a half dword that is stored as 16 bits.  A workgroup walks a segment of rows: as many as 64, cut down to 16
until the launch has 1024 workgroups.  A lane takes the samples two and four columns away from the dwords up to two left
and right of its own, reflected at a row's ends, and the rows two and four above and below from a window of nine rows
whose row index is reflected at the frame's top and bottom."""
import collections

import numpy as np

import nr_model as nm

WAVE_DWORDS = 64
STRIP_DWORDS = 256
MAX_ROWS, MIN_ROWS, SPREAD = 64, 16, 1024       # kNrMaxRows, kNrMinRows, kNrSpread
REACH = 4                                        # columns and rows a sample looks to either side

Case = collections.namedtuple("Case", "w h bits sbe nframes")

# noise amplitude A and constant threshold t of the frames of a depth: t is about 2 A / 3
NOISE = {8: (12, 8), 10: (50, 33), 12: (200, 130), 14: (800, 520), 16: (3000, 2047)}


def depth(case):
    return case.bits or 8


def per_dword(bits):
    return 2 if bits else 4


def row_dwords(w, bits):
    return w // 2 if bits else (w + 3) // 4


def strips(w, bits):
    return (row_dwords(w, bits) + STRIP_DWORDS - 1) // STRIP_DWORDS


def has_tail(w, bits):
    """the row ends in half a dword"""
    return not bits and w % 4 == 2


def seg_rows(w, bits, nframes, y0, y1):
    """rows a workgroup walks (launch_nr)"""
    h = y1 - y0
    rows = h * strips(w, bits) * nframes // SPREAD
    rows = min(max(rows, MIN_ROWS), MAX_ROWS)
    if (h + rows - 1) // rows > 65535:
        rows = (h + 65534) // 65535
    return rows


def segments(w, h, bits, nframes=1, y0=0, y1=None):
    """[(ya, yb)]: the row ranges of the workgroups of one strip"""
    y1 = h if y1 is None else y1
    rows = seg_rows(w, bits, nframes, y0, y1)
    return [(ya, min(ya + rows, y1)) for ya in range(y0, y1, rows)]


def column_seams(w, bits):
    """{name: [first column right of the seam]}: between the lanes at a row's two ends, between waves, between strips"""
    n, per = row_dwords(w, bits), per_dword(bits)
    lanes = sorted({d for d in (1, 2, n - 2, n - 1) if 0 < d < n})
    return {"lane": [d * per for d in lanes],
            "wave": [d * per for d in range(WAVE_DWORDS, n, WAVE_DWORDS) if d % STRIP_DWORDS],
            "strip": [d * per for d in range(STRIP_DWORDS, n, STRIP_DWORDS)]}


def seam_columns(w, bits):
    """the columns four on either side of every seam of column_seams, and the first and last four of the row"""
    cols = set(range(REACH)) | set(range(w - REACH, w))
    for seams in column_seams(w, bits).values():
        for x in seams:
            cols |= set(range(x - REACH, x + REACH))
    return sorted(c for c in cols if 0 <= c < w)


def seam_rows(w, h, bits, nframes=1, cuts=()):
    """the rows four on either side of every segment seam (and of every row in `cuts`), and the first and last four"""
    rows = set(range(REACH)) | set(range(h - REACH, h))
    for y in [ya for ya, _ in segments(w, h, bits, nframes)[1:]] + list(cuts):
        rows |= set(range(y - REACH, y + REACH))
    return sorted(r for r in rows if 0 <= r < h)


def row_cuts(band_rows, h, halo):
    """the rows at which a frame launched in the bands `band_rows` ([(y0, y1)], tests/band_cases.py) cuts its noise
    reduction launches (csrc/mibayer_abi.hip: enqueue_frame_banded): a band denoises up to the last row its own
    demosaic reads, y1 + halo, and the last one up to h"""
    return [y1 + halo for _, y1 in band_rows[:-1] if y1 + halo < h]


def curve_of(case):
    """the constant curve of the case's frames"""
    return [NOISE[depth(case)][1]] * nm.NODES


def seam_samples(case, f=0):
    """frame f of a case: a diagonal ramp of a quarter of a level per pixel at 8 bits (so that same-site neighbours lie
    within t of each other before the noise) with a per-site offset, plus uniform noise of +-A; the first sample's
    neighbours to the right and below lie exactly t and t + 1 above it"""
    d = depth(case)
    vmax = (1 << d) - 1
    amp, _ = NOISE[d]
    rng = np.random.default_rng([77, case.w, case.h, d, f])
    y, x = np.mgrid[0:case.h, 0:case.w]
    S = vmax // 4 + (x + 2 * y + 5 * f) * (vmax // 4) // max(case.w + 2 * case.h + 5 * case.nframes, 256) \
        + (vmax // 16) * (2 * (y & 1) + (x & 1))
    S = S + rng.integers(-amp, amp + 1, S.shape)
    # |d| = t and |d| = t + 1 by construction too: a frame of 30 samples has neither by chance at 16 bits
    S[0, 2] = S[0, 0] + NOISE[d][1]
    S[2, 0] = S[0, 0] + NOISE[d][1] + 1
    return S


def boundary_samples(case, at_max):
    """(S, centres): a frame of 0 (or max) in which every centre -- one per 8 x 10 cell -- has the neighbour two columns
    to its right exactly t away and the one two to its left t + 1 away, and the ones two rows above and below likewise:
    the first of each pair is included, the second is not"""
    d = depth(case)
    vmax = (1 << d) - 1
    t = NOISE[d][1]
    base, sign = (vmax, -1) if at_max else (0, 1)
    S = np.full((case.h, case.w), base, np.int64)
    centres = [(x, y) for y in range(2, case.h - 2, 10) for x in range(2, case.w - 2, 8)]
    for x, y in centres:
        S[y, x + 2] = base + sign * t
        S[y, x - 2] = base + sign * (t + 1)
        S[y - 2, x] = base + sign * t
        S[y + 2, x] = base + sign * (t + 1)
    return S, centres


def reaches(case):
    """what the case exercises, for tests/test_nr_cases.py"""
    seams = column_seams(case.w, case.bits)
    segs = segments(case.w, case.h, case.bits, case.nframes)
    return {"tail": has_tail(case.w, case.bits), "wave_seam": bool(seams["wave"]), "strip_seam": bool(seams["strip"]),
            "segments": len(segs), "short_last_segment": segs[-1][1] - segs[-1][0] < MIN_ROWS,
            "odd_height": bool(case.h & 1), "batch": case.nframes > 1,
            "reflections_overlap": case.h < 9 or case.w < 9}


# the minimum frames, a width of 2 mod 4 across a wave seam and a strip seam at a height a few rows past a segment seam
# (8-bit 1030 x 37, deep 518 x 37), a whole last dword, one segment, batches, every depth and both byte orders
CASES = [Case(6, 5, 0, False, 1), Case(6, 6, 0, False, 1), Case(8, 5, 0, False, 1), Case(10, 7, 0, False, 1),
         Case(1030, 37, 0, False, 1), Case(1032, 33, 0, False, 1), Case(258, 16, 0, False, 3),
         Case(6, 5, 16, True, 1), Case(6, 6, 12, False, 1), Case(8, 9, 10, False, 1), Case(518, 37, 12, False, 1),
         Case(518, 37, 10, True, 1), Case(516, 21, 16, False, 1), Case(130, 35, 14, False, 3),
         Case(70, 19, 16, True, 2)]


# long batches of narrow frames: the launches whose workgroups walk more than MIN_ROWS rows, the shapes of
# tests/dpc_cases.py (what each reaches: tests/test_nr_cases.py)
LONG_CASES = [Case(10, 35, 0, False, 512), Case(6, 70, 0, False, 256), Case(10, 52, 0, False, 512),
              Case(8, 33, 16, True, 800), Case(10, 45, 0, False, 1000), Case(10, 64, 0, False, 1024),
              Case(6, 67, 12, False, 1000), Case(14, 131, 0, False, 512), Case(262, 35, 0, False, 512)]
WIDE_LONG_CASE = LONG_CASES[-1]


def unclamped_rows(case):
    """what the rule gives before it is clamped to MIN_ROWS .. MAX_ROWS"""
    return case.h * strips(case.w, case.bits) * case.nframes // SPREAD


def segment_of(case, row):
    """(ya, yb) of the workgroups that walk `row`, for a failure message"""
    return next(s for s in segments(case.w, case.h, case.bits, case.nframes) if s[0] <= row < s[1])


def segment_blind(S, segs, curve, d):
    """nr_model.denoise as a kernel would compute it whose window stops at its segment: every segment's rows denoised as
    a frame of their own, the rows off its ends reflected back into it (and, in a segment of fewer than five rows, held
    at its end)"""
    S = np.asarray(S, np.int64)
    out = S.copy()
    for ya, yb in segs:
        n = yb - ya
        t = np.arange(-REACH, n + REACH)
        t = np.clip(np.where(t < 0, -t, np.where(t >= n, 2 * (n - 1) - t, t)), 0, n - 1)
        out[ya:yb] = nm.denoise(S[ya + t], curve, d)[REACH:n + REACH]
    return out


def case_id(c):
    return "%dx%d_%s%s_x%d" % (c.w, c.h, c.bits or 8, "be" if c.sbe else "", c.nframes)
