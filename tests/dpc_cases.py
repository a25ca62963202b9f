"""The case table of the defective pixel correction kernels' own geometry (csrc/mibayer_kernels.hip: mosaic_dpc_kernel,
mosaic_dpc_list_kernel, launch_dpc), restated here so that a CPU test can say what each case reaches
(tests/test_dpc_cases.py) before the GPU tests (tests/test_gpu_dpc.py) run them.

The geometry: a lane owns one dword of a row -- 4 samples of an 8-bit mosaic, 2 of a deep one; a wave spans 64 dwords, a
workgroup 256 = one strip; a row whose width is 2 mod 4 ends, in an 8-bit mosaic, in a half dword that is stored as 16
bits.  A workgroup walks a segment of rows: as many as 64, cut down to 16 until the launch has 1024 workgroups.  A lane
takes the samples two columns away from the dwords left and right of its own, the first and the last dword of a row from
the other side, and the rows two above and below from a window that is mirrored at the frame's top and bottom."""
import collections
import functools

import numpy as np

WAVE_DWORDS = 64
STRIP_DWORDS = 256
MAX_ROWS, MIN_ROWS, SPREAD = 64, 16, 1024       # kDpcMaxRows, kDpcMinRows, kDpcSpread

Case = collections.namedtuple("Case", "w h bits sbe nframes")


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
    """rows a workgroup walks (launch_dpc)"""
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
    """the columns two on either side of every seam of column_seams, and the first and last two of the row"""
    cols = {0, 1, w - 2, w - 1}
    for seams in column_seams(w, bits).values():
        for x in seams:
            cols |= {x - 2, x - 1, x, x + 1}
    return sorted(c for c in cols if 0 <= c < w)


def seam_rows(w, h, bits, nframes=1, cuts=()):
    """the rows two on either side of every segment seam (and of every row in `cuts`), and the first and last two"""
    rows = {0, 1, h - 2, h - 1}
    for y in [ya for ya, _ in segments(w, h, bits, nframes)[1:]] + list(cuts):
        rows |= {y - 2, y - 1, y, y + 1}
    return sorted(r for r in rows if 0 <= r < h)


@functools.lru_cache(maxsize=None)
def _planted(w, h, bits, nframes, cuts):
    return np.array([(x, y) for y in seam_rows(w, h, bits, nframes, cuts) for x in seam_columns(w, bits)], np.uint32)


def planted(w, h, bits, nframes=1, cuts=()):
    """(n, 2) of (x, y): a defect at every crossing of a seam column and a seam row"""
    return _planted(w, h, bits, nframes, tuple(cuts)).copy()


def plant(S, where, vmax):
    """S with the samples at `where` stuck at 0 or vmax in turn"""
    S = np.array(S, np.int64)
    where = np.asarray(where, np.int64).reshape(-1, 2)
    S[where[:, 1], where[:, 0]] = np.where(np.arange(len(where)) % 2 == 0, vmax, 0)
    return S


def phase_of(where):
    """0 .. 3 per coordinate: the planted samples of one phase lie at least four columns or rows apart, so none is a
    neighbour of another and the detection must find every one of them"""
    where = np.asarray(where, np.int64).reshape(-1, 2)
    return 2 * ((where[:, 1] >> 1) & 1) + ((where[:, 0] >> 1) & 1)


def texture(case, f=0):
    """what makes the replacement of a planted sample depend on the rows two above and below it: same-site columns
    0, 1, 2 steps of max / 32 up in turn (the gradient of H is one or two steps), rows a sawtooth of period 8 (the
    gradient of V is 4 max / 255 everywhere: under H's and not 0), so that V or a diagonal wins and R is the mean of two
    rows that a window cut off at a segment seam does not have.  Both move with the frame"""
    vmax = (1 << (case.bits or 8)) - 1
    y, x = np.mgrid[0:case.h, 0:case.w]
    return (vmax // 32) * (((x >> 1) + f) % 3) + (vmax // 255) * ((y + f) % 8)


def seam_samples(case, f=0, phase=None):
    """frame f of a case: a gentle ramp with per-site offsets and the texture above (same-site steps under max / 8) and
    stuck samples planted on both sides of every lane, wave, strip and segment seam and on the first and last two rows
    and columns: all of them (phase None; neighbours then hide each other from the detection), or those of one phase_of"""
    vmax = (1 << (case.bits or 8)) - 1
    where = planted(case.w, case.h, case.bits, case.nframes)
    if phase is not None:
        where = where[phase_of(where) == phase]
    y, x = np.mgrid[0:case.h, 0:case.w]
    S = vmax // 4 + (x + 2 * y + 5 * f) * (vmax // 3) // (case.w + 2 * case.h + 5 * case.nframes) \
        + (vmax // 16) * (2 * (y & 1) + (x & 1)) + texture(case, f)
    return plant(S, np.roll(where, f, axis=0), vmax)


def segment_of(case, row):
    """(ya, yb) of the workgroups that walk `row`, for a failure message"""
    return next(s for s in segments(case.w, case.h, case.bits, case.nframes) if s[0] <= row < s[1])


def segment_blind(S, segs, hot, cold):
    """dpc_model.correct as a kernel would compute it whose window stops at its segment: every segment's rows corrected
    as a frame of their own, the rows off its ends mirrored back into it (and, in a segment of fewer than three rows,
    held at its end)"""
    import dpc_model as dm
    S = np.asarray(S, np.int64)
    out = S.copy()
    for ya, yb in segs:
        n = yb - ya
        t = np.arange(-2, n + 2)
        t = np.clip(np.where(t < 0, t + 4, np.where(t >= n, t - 4, t)), 0, n - 1)
        out[ya:yb] = dm.correct(S[ya + t], hot, cold)[2:n + 2]
    return out


def long_list(case, rng, n=300):
    """a defect list for a long case: every planted seam position and random other ones, more than 256 and fewer than
    512 after the library has sorted it -- two workgroups of the list kernel per frame, the second partial"""
    where = planted(case.w, case.h, case.bits, case.nframes)
    n = max(min(n, case.w * case.h - 4), len(where))
    rest = sorted({(x, y) for y in range(case.h) for x in range(case.w)} - {tuple(p) for p in where.tolist()})
    more = rng.permutation(len(rest))[:n - len(where)]
    lst = np.concatenate([where, np.asarray(rest, np.uint32).reshape(-1, 2)[more]])
    return lst[rng.permutation(len(lst))]


def reaches(case):
    """what the case exercises, for tests/test_dpc_cases.py"""
    seams = column_seams(case.w, case.bits)
    segs = segments(case.w, case.h, case.bits, case.nframes)
    return {"one_lane": row_dwords(case.w, case.bits) == 1, "tail": has_tail(case.w, case.bits),
            "wave_seam": bool(seams["wave"]), "strip_seam": bool(seams["strip"]), "segments": len(segs),
            "short_last_segment": segs[-1][1] - segs[-1][0] < MIN_ROWS, "batch": case.nframes > 1,
            "mirror_overlaps": case.h < 6 or case.w < 6}


# the degenerate frames, a width of 2 mod 4 across a wave seam and a strip seam at a height a few rows past a segment seam
# (8-bit 1030 x 37, deep 518 x 37), a whole last dword, one segment, a batch
CASES = [Case(4, 4, 0, False, 1), Case(6, 5, 0, False, 1), Case(1030, 37, 0, False, 1), Case(1032, 33, 0, False, 1),
         Case(258, 16, 0, False, 3), Case(4, 4, 12, False, 1), Case(6, 5, 16, True, 1), Case(518, 37, 12, False, 1),
         Case(518, 37, 10, True, 1), Case(130, 35, 14, False, 3)]


# long batches of narrow frames: the launches whose workgroups walk more than MIN_ROWS rows (what each reaches:
# tests/test_dpc_cases.py).  17 with odd seams, a last segment of one row and a half-dword tail; 17 five times; 26 twice,
# no short segment; 25; 43; 64 as the rule gives it, one segment; 64 clamped from 65 with a short last segment; 64 clamped,
# three segments; and 17 across a wave seam with a tail, the one wide case
LONG_CASES = [Case(10, 35, 0, False, 512), Case(6, 70, 0, False, 256), Case(10, 52, 0, False, 512),
              Case(8, 33, 16, True, 800), Case(10, 45, 0, False, 1000), Case(10, 64, 0, False, 1024),
              Case(6, 67, 12, False, 1000), Case(14, 131, 0, False, 512), Case(262, 35, 0, False, 512)]
WIDE_LONG_CASE = LONG_CASES[-1]


def unclamped_rows(case):
    """what the rule gives before it is clamped to MIN_ROWS .. MAX_ROWS"""
    return case.h * strips(case.w, case.bits) * case.nframes // SPREAD


def case_id(c):
    return "%dx%d_%s%s_x%d" % (c.w, c.h, c.bits or 8, "be" if c.sbe else "", c.nframes)
