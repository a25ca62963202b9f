"""The launch rule of the lens shading kernel (csrc/mibayer_kernels.hip: mosaic_shade_kernel, launch_shade) and the table
of its long launches, restated here so that a CPU test can say what each case reaches (tests/test_shading_cases.py)
before the GPU tests (tests/test_gpu_shading.py) run them.

The geometry: a lane owns one dword of a row -- 4 samples of an 8-bit mosaic, 2 of a deep one; a workgroup spans 256
dwords = one strip and walks a segment of rows: as many as 64, cut down to 16 until the launch has 1024 workgroups, and
even.  Rows are counted from the even row at or under y0, so every segment starts on an even row.  Inside a segment the
walk goes cell row by cell row (a cell is 1 << ky rows), kShadeAhead rows at a time: a segment that starts inside a cell
row begins with the vertical weight fy = ya mod (1 << ky), and one that crosses a cell-row seam reads a new row of nodes
there."""
import collections

import numpy as np

import shading_model as shm

STRIP_DWORDS = 256
AHEAD, MIN_ROWS, MAX_ROWS, SPREAD = 8, 16, 64, 1024     # kShadeAhead, kShadeMinRows, kShadeMaxRows, kShadeSpread

Case = collections.namedtuple("Case", "w h bits sbe nframes kx ky")


def row_dwords(w, bits):
    return w // 2 if bits else (w + 3) // 4


def strips(w, bits):
    return (row_dwords(w, bits) + STRIP_DWORDS - 1) // STRIP_DWORDS


def seg_rows(w, bits, nframes, y0, y1):
    """rows a workgroup walks (launch_shade)"""
    h = y1 - (y0 & ~1)
    rows = h * strips(w, bits) * nframes // SPREAD
    rows = min(max(rows, MIN_ROWS), MAX_ROWS)
    if (h + rows - 1) // rows > 65535:
        rows = (h + 65534) // 65535
    return (rows + 1) & ~1


def segments(w, h, bits, nframes=1, y0=0, y1=None):
    """[(ya, yb)]: the row ranges of the workgroups of one strip; the first one's rows under y0 are not written"""
    y1 = h if y1 is None else y1
    rows = seg_rows(w, bits, nframes, y0, y1)
    return [(ya, min(ya + rows, y1)) for ya in range(y0 & ~1, y1, rows)]


def case_segments(case):
    return segments(case.w, case.h, case.bits, case.nframes)


def segment_of(case, row):
    """(ya, yb) of the workgroups that walk `row`, for a failure message"""
    return next(s for s in case_segments(case) if s[0] <= row < s[1])


def cell_phases(case, ky=None):
    """the set of ya mod (1 << ky) over the case's segments: the vertical weights a segment starts with"""
    ky = case.ky if ky is None else ky
    return {ya & ((1 << ky) - 1) for ya, _ in case_segments(case)}


def crosses_a_cell_seam(case, seg):
    ya, yb = seg
    return (ya >> case.ky) != ((yb - 1) >> case.ky)


def site_planes(w, h, kx, ky, rng=None):
    """four visibly different site planes (a swapped site or row parity shows), each a ramp in both directions"""
    nx, ny = shm.nodes(w, h, kx, ky)
    j, i = np.mgrid[0:ny, 0:nx]
    t = np.stack([base + 37 * s + (90 + 20 * s) * i + (150 - 30 * s) * j for s, base in enumerate((3000, 5200, 7100, 9400))])
    if rng is not None:
        t = t + rng.integers(0, 64, t.shape)
    assert t.max() <= shm.MAX_ENTRY
    return t.astype(np.uint16)


def apply_with(S, table, kx, ky, black, depth, j, fy):
    """shading_model.apply with the node row j and the vertical weight fy of every row given, (H,) each: what a kernel
    computes that has them wrong"""
    H, W = S.shape
    nx, ny = shm.nodes(W, H, kx, ky)
    g = np.asarray(table).astype(np.int64).reshape(4, ny, nx)
    cw, ch, vmax = 1 << kx, 1 << ky, (1 << depth) - 1
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    j, fy = np.asarray(j)[:, None], np.asarray(fy)[:, None]
    i, fx = x >> kx, x & (cw - 1)
    s = 2 * (y & 1) + (x & 1)
    top = g[s, j, i] * (cw - fx) + g[s, j, i + 1] * fx
    bot = g[s, j + 1, i] * (cw - fx) + g[s, j + 1, i + 1] * fx
    G = (top * (ch - fy) + bot * fy + (1 << (kx + ky - 1))) >> (kx + ky)
    bl = np.asarray(black, np.int64)[s]
    return np.clip(bl + (((S.astype(np.int64) - bl) * G + 2048) >> 12), 0, vmax)


def rows_of(case, variant=None):
    """(j, fy) of every row: the definition's; "restart": the vertical weight counted from the segment's first row;
    "stale": the node rows of the segment's first cell row kept for the whole segment"""
    ch = 1 << case.ky
    y = np.arange(case.h)
    j, fy = y >> case.ky, y & (ch - 1)
    for ya, yb in case_segments(case):
        if variant == "restart":
            fy[ya:yb] = (y[ya:yb] - ya) & (ch - 1)
        elif variant == "stale":
            j[ya:yb] = ya >> case.ky
    return j, fy


# the shapes of tests/dpc_cases.py LONG_CASES, each with a grid (what they reach together: tests/test_shading_cases.py):
# cells of 4 rows under 18-row segments (a segment starts two rows before a seam) and under 44-row ones (every segment
# seam is a cell seam); cells of 8 rows under 18, 26 and 44; cells of 32 under 26; one cell row for the whole frame; cells
# of 4 columns, a dword per cell column
LONG_CASES = [Case(10, 35, 0, False, 512, 2, 2), Case(6, 70, 0, False, 256, 2, 3), Case(10, 52, 0, False, 512, 3, 3),
              Case(8, 33, 16, True, 800, 2, 5), Case(10, 45, 0, False, 1000, 3, 3), Case(10, 45, 0, False, 1000, 2, 2),
              Case(10, 64, 0, False, 1024, 4, 8), Case(6, 67, 12, False, 1000, 2, 4), Case(14, 131, 0, False, 512, 3, 8),
              Case(262, 35, 0, False, 512, 5, 2)]
WIDE_LONG_CASE = LONG_CASES[-1]


def case_id(c):
    return "%dx%d_%s%s_x%d_k%d%d" % (c.w, c.h, c.bits or 8, "be" if c.sbe else "", c.nframes, c.kx, c.ky)
